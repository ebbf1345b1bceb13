"""The slot-state harness itself, on the CPU (tests/slot_model.py; its GPU run is tests/test_gpu_slot_state.py): the random
generator is deterministic and legal, the hand-written scenarios cover every (kind of cached state, mutator, role) cell but the
listed ones, DESIGN.md's table is the model's, every sequence passes the checker on the numpy FakeContext -- and the checker
FAILS, at the first search after the mutation, when the fake answers one search from the slot's contents before it: the proof
that the GPU test notices a stale index, with no GPU and no wrong kernel.  The fake with the aligns' former rule for the output
slot's segment table fails the key comparison of the shard scenarios the same way."""
import importlib
import os
import re

import pytest

import slot_model as M
from conftest import PKG, ROOT

SMALL, MEDIUM = 257, 700                       # scan sizes of the matrix and of the hand-written scenarios here (the GPU test runs both at 3 000)
SMALL_PROLOGUE = M.PROLOGUE + [("upload", dict(slot=0, cloud="v1:700")), ("upload", dict(slot=1, cloud="v0:700")), ("upload", dict(slot=2, cloud="v2:257"))]
HAND_WRITTEN = tuple(n for n in M.named_scenarios() if not n.startswith(("dst-", "src-")))


@pytest.fixture(scope="module")
def env(built):
    import oracle
    return M.Env(importlib.import_module(PKG), oracle)


def checker(env, cls=M.Checker, **fake):
    return cls(lambda clean=False: M.FakeContext(env.mvr, ref=env.ref, **({} if clean else fake)), env,
               export_keys=lambda ctx, s, t: ctx.fake_forward_keys(s, t))


def test_op_table_names_every_entry_of_the_issue():
    assert set(M.MUTATORS) == {"upload", "clear", "reserve", "copy", "append", "set_global_base", "append_range", "transform", "transform_f32",
                               "transform_batch", "upload_normals", "estimate_normals", "denoise", "voxel_grid", "statistical_outlier_removal",
                               "radius_outlier_removal", "extract_indices", "segment_plane", "mls", "iss_keypoints", "icp_align",
                               "icp_align_rejected", "icp_align_gicp", "align_prerejective", "ring_step", "seq_run"}
    assert set(M.BUILDERS) == {"nn", "knn", "correspondences", "pair_moments2", "pair_moments2_batch", "fpfh", "boundary", "pose_scores", "fitness"}
    assert M.NOT_BIT_REPRODUCIBLE == ()
    for name, op in M.OPS.items():              # every public method the table calls exists on the package's Context
        assert name in ("upload", "probe") or hasattr(importlib.import_module(PKG).Context, name), name


@pytest.mark.parametrize("seed", M.SEEDS[:3])
def test_random_sequences_are_deterministic_and_legal(env, seed):
    a = checker(env).run_random(seed, steps=14, prologue=SMALL_PROLOGUE)
    b = checker(env).run_random(seed, steps=14, prologue=SMALL_PROLOGUE)
    assert M.fmt(a.seq) == M.fmt(b.seq) and len(a.seq) == len(SMALL_PROLOGUE) + 14
    # legal: every call satisfies its preconditions against the model as it stood before the call (the replay keeps its own model)
    model = M.Model()
    fake = M.FakeContext(env.mvr, ref=env.ref)
    for name, args in a.seq:
        pre = model.snapshot()
        assert M.OPS[name].legal(pre, args) is None, (name, args)
        M.OPS[name].run(fake, args, pre, env)
        for s in M.OPS[name].writes(args):
            sl = fake._get(s)
            model.slots[s] = M.Slot(sl.pts, sl.nrm, M.segs_after(name, args, pre, s), M.dirty_after(name, args, pre, s, env))
    # ... and pasted back as a scenario it runs again
    assert eval(M.fmt(a.seq)) == a.seq
    checker(env).run(a.seq)
    assert M.fmt(checker(env).run_random(seed + 1000, steps=14, prologue=SMALL_PROLOGUE).seq) != M.fmt(a.seq)


def test_coverage_matrix_is_complete():
    """for each kind of cached state and each mutator some named scenario builds that state on a slot and applies the mutator
    with the slot as destination, and -- where the mutator has a distinct source -- as source; nothing is left out but
    INAPPLICABLE, and nothing listed there is covered after all"""
    cells = set()
    for seq in M.named_scenarios().values():
        cells |= M.coverage(seq)
    need = M.required_cells()
    assert len(need) == 6 * (len(M.MUTATORS) + sum(1 for m in M.MUTATORS if M.OPS[m].src_role))
    assert sorted(need - cells - set(M.INAPPLICABLE)) == []
    assert sorted(set(M.INAPPLICABLE) & cells) == []
    assert set(M.INAPPLICABLE) <= need and all(M.INAPPLICABLE.values())
    # the smaller clouds of this file's runs change nothing about it
    small = set()
    for seq in M.matrix_scenarios(SMALL, SMALL).values():
        small |= M.coverage(seq)
    assert need - small - set(M.INAPPLICABLE) == set()
    # the cases the aligns must cover: out = another slot, out == src, out = -1, out = a slot that was a shard
    sc = M.named_scenarios()
    for al in M.ALIGNS:
        outs = {(a["out"] == a["src"], a["out"] == -1) for seq in sc.values() for n, a in seq if n == al}
        assert outs == {(True, False), (False, True), (False, False)}, al
        shard = sc["shard-" + al]
        k = [n for n, _ in shard].index(al)
        assert ("set_global_base", dict(slot=shard[k][1]["out"], base=5000)) in shard[:k], al
    uploads = {a["cloud"] for seq in sc.values() for n, a in seq if n == "upload"}
    assert {"empty", "v1:3", "dirty:700"} <= uploads and {int(c.split(":")[1]) for c in uploads if ":" in c} >= set(M.SIZES)


def test_design_table_is_the_models():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 22. What a writing entry leaves on its destination slot"):]
    rows = {}
    for line in sec.splitlines():
        m = re.match(r"\| `([^`]+)` \|(.*)\|$", line)
        if m:
            rows[m.group(1)] = tuple(c.strip() for c in m.group(2).split("|"))
    assert rows == M.KEEPS
    head = [c.strip() for c in re.search(r"\| entry \|(.*)\|", sec).group(1).split("|")]
    assert tuple(head) == M.COLUMNS
    assert {k.split(" (")[0] for k in M.KEEPS} == set(M.MUTATORS)
    # the table's last column and segs_after say the same for the plain cases: a shard source, a shard destination
    pre = M.Model()
    pre.slots[0], pre.slots[1] = M.Slot(M.np.zeros((5, 4), M.F32), segs=[(0, 5, 100)]), M.Slot(M.np.zeros((7, 4), M.F32), segs=[(0, 7, 900)])
    for name in ("copy", "transform", "transform_f32") + M.ALIGNS:
        a = dict(dst=1, src=0, out=1, tgt=2)
        assert M.KEEPS[name][6] == "src" and M.segs_after(name, a, pre, 1) == [(0, 5, 100)], name
        if name != "copy":
            a = dict(dst=1, src=1, out=1, tgt=2)
            assert M.KEEPS[name + " (in place)"][6] == "keep" and M.segs_after(name, a, pre, 1) == [(0, 7, 900)], name
    for name in ("voxel_grid", "mls", "upload", "clear"):
        assert M.KEEPS[name][6] == "drop" and M.segs_after(name, dict(dst=1, src=0, slot=1), pre, 1) == [], name
    assert M.segs_after("append", dict(dst=1, src=0), pre, 1) == [(0, 7, 900), (7, 5, 907)]
    assert M.segs_after("append_range", dict(dst=2, src=0, begin=1, count=3, base=50), pre, 2) == [(0, 3, 50)]


@pytest.mark.parametrize("name", sorted(M.matrix_scenarios()))
def test_matrix_scenarios_pass_on_the_fake(env, name):
    checker(env).run(M.matrix_scenarios(SMALL, SMALL)[name])


@pytest.mark.parametrize("name", HAND_WRITTEN)
def test_hand_written_scenarios_pass_on_the_fake(env, name):
    c = checker(env).run(M.named_scenarios(MEDIUM)[name])
    if name.startswith("shard-"):
        assert any(s.segs for s in c.model.slots.values())


class Armed(M.Checker):
    """arms the fake's stale switch right before the step under test"""
    arm_at, arm = None, None

    def before_step(self, k, ctx):
        if k == self.arm_at:
            ctx.stale = self.arm


def _at(seq, name):
    return max(k for k, (n, _) in enumerate(seq) if n == name)


def _stale_run(env, seq, search, slot, at=None):
    c = checker(env, cls=Armed)
    c.arm_at, c.arm = len(seq) - 1 if at is None else at, (search, slot)
    with pytest.raises(M.CheckFailure) as e:
        c.run(seq)
    return e.value


@pytest.mark.parametrize("mutator", [m for m in M.MUTATORS if m not in M.NO_OUTPUT_SLOT])
def test_a_stale_search_after_each_mutator_fails_the_checker(env, mutator):
    """the mutator rewrites the slot under test (or leaves its points alone, after an earlier call rewrote them: reserve,
    set_global_base, the two normals entries); from that step on the fake's nn answers for that slot from the contents before
    the last rewrite.  The checker fails AT that step, in its nn search of that slot."""
    seq = M.matrix_scenarios(SMALL, SMALL)["dst-" + mutator]
    k = _at(seq, mutator)
    assert M.S in M.OPS[mutator].writes(seq[k][1]) and [n for n, _ in seq[k + 1:]] == ["probe"]
    f = _stale_run(env, seq, "nn", M.S, k)
    assert f.step == k and (f.what.startswith("search: nn") and "-> %d" % M.S in f.what or f.what in ("search: size of slot %d" % M.S, "search: nn in the empty slot %d" % M.S)), str(f)[:300]


@pytest.mark.parametrize("mutator", [m for m in M.MUTATORS if M.OPS[m].src_role and m not in M.NO_OUTPUT_SLOT])
def test_a_stale_search_of_the_output_of_each_mutator_fails_the_checker(env, mutator):
    """the same for the slot the mutator writes when the slot under test is its SOURCE"""
    seq = M.matrix_scenarios(SMALL, SMALL)["src-" + mutator]
    k = _at(seq, mutator)
    out = M.OPS[mutator].writes(seq[k][1])[0]
    assert out != M.S
    if out == M.FILTER_DST:                       # (the checker's own radius filter rewrites the filter destination: a probe of it proves nothing)
        seq = seq[:k] + [(mutator, dict(seq[k][1], dst=M.X))] + seq[k + 1:]
        out = M.X
    f = _stale_run(env, seq, "nn", out, k)
    assert f.step == k and f.what.startswith("search"), str(f)[:300]


@pytest.mark.parametrize("search,what", [("nn", "search: nn"), ("knn", "search: knn"), ("correspondences", "search: correspondences"),
                                         ("radius", "search: the filter destination after radius_outlier_removal")])
def test_each_search_of_the_checker_notices(env, search, what):
    seq = M.matrix_scenarios(SMALL, SMALL)["dst-transform"][:-2] + [("transform", dict(dst=M.S, src=M.S, pose="turn"))]
    f = _stale_run(env, seq, search, M.S)          # (a rigid motion keeps every neighbour count: the stale radius filter keeps the right indices, of the wrong points)
    assert f.step == len(seq) - 1 and f.what.startswith(what), str(f)[:300]
    assert "the sequence up to it" in str(f) and eval(str(f).split("the sequence up to it:\n")[1]) == seq


def test_a_stale_seed_or_pair_record_fails_the_probe(env):
    """what no search reads: from the mutator on the fake's aligns answer for the slot under test from its contents before the
    rewrite (what a stale seed or pair record does); the probe that ends every matrix scenario differs from its clean room"""
    for mutator in ("upload", "extract_indices", "transform", "icp_align"):
        seq = M.matrix_scenarios(SMALL, SMALL)["dst-" + mutator]
        k = _at(seq, mutator)
        f = _stale_run(env, seq, "align", M.S, k)
        assert seq[f.step][0] == "probe" and f.step > k and f.what == "clean room: return values differ", (mutator, str(f)[:300])
    # ... and coverage() counts a seed or pair-record cell only where such a consumer follows the mutator
    seq = M.matrix_scenarios()["dst-upload"]
    assert (4, "upload", "dst") in M.coverage(seq) and (4, "upload", "dst") not in M.coverage(seq[:-1])
    assert (5, "upload", "dst") not in M.coverage(seq[:-1]) and (1, "upload", "dst") in M.coverage(seq[:-1])


def test_sequences_pass_without_the_checkers_searches(env):
    for name in ("extend-1025+700", "append-pairs"):
        c = M.Checker(lambda clean=False: M.FakeContext(env.mvr, ref=env.ref), env, searches=False)
        c.run(M.named_scenarios(MEDIUM)[name])


@pytest.mark.parametrize("align", M.ALIGNS)
def test_the_former_rule_for_an_aligns_output_table_fails_the_key_comparison(env, align):
    """the fake with the library's rule from before finish_align_out -- the output slot of an align keeps the table of the shard
    it was -- fails the shard scenario at the align, in the comparison of the exported keys with the model's numbering"""
    seq = M.named_scenarios(MEDIUM)["shard-" + align]
    k = [n for n, _ in seq].index(align)
    with pytest.raises(M.CheckFailure) as e:
        checker(env, align_keeps_table=True).run(seq)
    assert e.value.step == k and e.value.what.startswith("search: nn_forward_keys"), str(e.value)[:300]


def test_an_untouched_slot_that_changes_fails_the_checker(env):
    class Leaky(M.FakeContext):
        def transform(self, d, s, T, dtype=M.F64):
            super().transform(d, s, T, dtype)
            if d != s and self.size(9):
                self.s[9].pts = self.s[9].pts + M.F32(1.0)
    c = M.Checker(lambda clean=False: Leaky(env.mvr, ref=env.ref), env)
    seq = M.PROLOGUE + [("upload", dict(slot=0, cloud="v1:65")), ("transform", dict(dst=1, src=0, pose="nudge"))]
    with pytest.raises(M.CheckFailure) as e:
        c.run(seq)
    assert e.value.step == 3 and e.value.what == "untouched slot 9 changed"


def test_a_result_that_depends_on_history_fails_the_clean_room(env):
    class Sticky(M.FakeContext):
        calls = 0

        def fitness(self, s, t, T, **kw):
            Sticky.calls += 1
            return super().fitness(s, t, T) + (1e-9 if self.prev.get(t) is not None and len(self.prev[t]) else 0.0)
    c = M.Checker(lambda clean=False: Sticky(env.mvr, ref=env.ref), env)
    seq = M.PROLOGUE + [("upload", dict(slot=0, cloud="v1:65")), ("upload", dict(slot=1, cloud="v0:65")), ("upload", dict(slot=1, cloud="v0:257")),
                        ("fitness", dict(src=0, tgt=1, pose="nudge"))]
    with pytest.raises(M.CheckFailure) as e:
        c.run(seq)
    assert e.value.step == 5 and e.value.what == "clean room: return values differ"
