"""GPU tests of the sample-consensus rejector (rules C1-C12 at mvr_reject_sample_consensus in include/mvr_hip.h) where its
arithmetic and its stops decide, on the hardening cases of tests/reject_sac_cases.py (their preconditions are asserted on the
reference alone in tests/test_reject_sac_host.py):
  1. graded lists near the origin and 1e3 .. 1e6 mm from it, many-to-one matches, non-finite points: the trace replayed by
     reject_sac_ref.verify, check (c) in far frames as a displacement against what a cast to f32 can do;
  2. valid counts on the counting kernel's tile edges; every chunk size, and so every register count, without and with fma;
  3. thresholds put on a d2 on purpose: an exact tie, and one between a pair's plain and fma d2, through three entries;
  4. C10 round by round: max_iterations = 1 .. R* + 1 and none, every (T_r, I_r) against the round before;
  5. the unit of length: 2^k times the points and the threshold changes no decision and no bit of a rotation;
  6. C11's truncation through the C entry; last_sample_consensus() after two stages in one chain."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import reject_sac_cases as SC
import reject_sac_ref as R
from align_ref import kabsch
from conftest import PKG

pytestmark = pytest.mark.gpu

S, T_ = 20, 21
CHUNKS = (1, 2, 63, 64, 65, 128, 129, 256)
bits = R.bits


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def hard():
    return SC.build_hard()


@pytest.fixture(scope="module")
def ctx(mvr):
    with mvr.Context(0) as c:
        yield c
        c.tune(rej_sac_chunk=0)


@pytest.fixture(scope="module")
def small():
    pair = SC.small_motion(SC.SMALL_SEED)
    q, m, d = SC.small_list(pair)
    return dict(pair, q=q, m=m, d=d, max_iterations=0, refine=False)


def rej_of(mvr, case, **kw):
    a = dict(max_iterations=case["max_iterations"], refine=case["refine"], seed=case["seed"])
    a.update(kw)
    return mvr.rejector("sample_consensus", a.pop("value", case["value"]), **a)


def load(ctx, case):
    ctx.upload(S, case["src"])
    ctx.upload(T_, case["tgt"])


def run(mvr, ctx, case, trace=True, **kw):
    return ctx.reject_sample_consensus(S, T_, case["q"], case["m"], case["d"], rej_of(mvr, case, **kw), return_trace=trace)


def verify(case, got, **kw):
    a = dict(value=case["value"], max_iterations=case["max_iterations"], refine=case["refine"], seed=case["seed"])
    a.update({k: kw.pop(k) for k in tuple(kw) if k in a})
    return R.verify(case["src"], case["tgt"], case["q"], case["m"], case["d"], a["value"], a["max_iterations"], a["refine"], a["seed"], got, **kw)


RESULT_KEYS = ("found", "live", "valid", "inliers", "ransac_inliers", "iterations", "attempts", "skipped", "best_attempt", "refine_rounds", "k")


def same_result(a, b, what):
    for k in RESULT_KEYS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert np.array_equal(bits(a["T"]), bits(b["T"])) and np.array_equal(bits(a["ransac_T"]), bits(b["ransac_T"])), what


def same_list(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2])), what


def same_run(a, b, what):
    same_list(a, b, what)
    same_result(a[3], b[3], what)
    for k in ("status", "query", "match", "inliers"):
        assert np.array_equal(a[4][k], b[4][k]), (what, k)
    assert np.array_equal(bits(a[4]["T"]), bits(b[4]["T"])) and np.array_equal(a[4]["k"].view(np.uint64), b[4]["k"].view(np.uint64)), what


def pairs_of(case):
    q, m, d = R.sort_list(case["q"], case["m"], case["d"])
    return q, m, d, case["src"][q, :3], case["tgt"][m, :3]


# ------------------------------------------------------------------ 1. graded lists

@pytest.mark.parametrize("name", SC.GRADED_NAMES + ("graded_shared", "graded_non_finite"))
def test_graded_lists_replayed_from_their_trace(mvr, ctx, hard, name):
    case = hard[name]
    load(ctx, case)
    got = run(mvr, ctx, case)
    far = case["far"] > 0
    fig = verify(case, got, check_c=True, far=far)
    res = got[3]
    if far:
        print("%s: %d attempts (%d counted, %.0f %% well conditioned); worst displacement of T against f64 Kabsch %.3g mm, the cast's bar %.3g mm; %d of %d kept"
              % (name, res["attempts"], fig["counted"], 100 * fig["well"], fig["worst_disp"], fig["bar"], res["inliers"], res["valid"]))
    else:
        print("%s: %d attempts (%d counted, %.0f %% well conditioned), T within %.2g / %.2g of Kabsch; %d of %d kept"
              % (name, res["attempts"], fig["counted"], 100 * fig["well"], fig["worst_rot"], fig["worst_trans"], res["inliers"], res["valid"]))
    assert res["found"] and res["attempts"] > 256 and fig["well"] >= 0.9, name
    assert 0.15 * res["valid"] < res["inliers"] < 0.3 * res["valid"], name
    if name == "graded_non_finite":
        assert res["valid"] < res["live"] == 3000
    assert np.array_equal(bits(ctx.download(S)), bits(case["src"])) and np.array_equal(bits(ctx.download(T_)), bits(case["tgt"]))


# ------------------------------------------------------------------ 2. tile and register edges

@pytest.mark.parametrize("name", SC.EDGE_NAMES)
def test_valid_counts_on_the_tile_edges(mvr, ctx, hard, name):
    case = hard[name]
    load(ctx, case)
    got = run(mvr, ctx, case)
    fig = verify(case, got, check_c=True)
    q, m, d, _, _ = pairs_of(case)
    keep = case["planted"]
    assert got[3]["valid"] == int(name.split("_")[1]) and fig["well"] >= 0.9
    same_list(got, (q[keep], m[keep], d[keep]), name)


def test_every_chunk_size_gives_the_same_bits(mvr, ctx, hard):
    case = hard["graded_100000"]
    load(ctx, case)
    ctx.tune(rej_sac_chunk=0)
    base = run(mvr, ctx, case)
    assert base[3]["attempts"] > 256      # so a chunk of 256 is consumed whole: all four registers
    for chunk in CHUNKS:
        ctx.tune(rej_sac_chunk=chunk)
        same_run(run(mvr, ctx, case), base, chunk)
    ctx.tune(rej_sac_chunk=0)


def test_every_chunk_size_with_fma(mvr, ctx, small):
    """correspondences_rejected(fma=True) is the one way to the counting kernel's fma instantiations.  It has no trace; the
    dedicated entry's (same list, same seed, so the same samples and the same T of every attempt) stands in: the host counts
    with C5's fma form under the traced T, replays the loop, and so knows which attempt must win and what must survive."""
    load(ctx, small)
    q, m, P, Q = small["q"], small["m"], small["src"][small["q"], :3], small["tgt"][small["m"], :3]
    for value, cap in ((small["value"], 0), (SC.SMALL_TIGHT, SC.SMALL_TIGHT_CAP)):
        ctx.tune(rej_sac_chunk=0)
        rej = rej_of(mvr, small, value=value, max_iterations=cap)
        traced = run(mvr, ctx, small, value=value, max_iterations=cap)
        tr = traced[4]
        Ts = [t.reshape(4, 4).T for t in tr["T"]]
        counts = [int(R.inlier_mask(T, P, Q, value, fma=True).sum()) if s == R.COUNTED else 0 for T, s in zip(Ts, tr["status"])]
        lp = R.replay_loop(tr["status"], counts, len(q), cap or 1000)       # (asserts that the fma loop consumes the traced attempts)
        keep = R.inlier_mask(Ts[lp["best"]], P, Q, value, fma=True)
        if cap:
            assert lp["attempts"] == cap + 1 and lp["best"] >= 0
        base = ctx.correspondences_rejected(S, T_, small["max_dist"], [rej], reciprocal=False, fma=True)
        last = ctx.last_sample_consensus()
        assert np.array_equal(base[0], q[keep]) and np.array_equal(base[1], m[keep]), value
        assert (last["best_attempt"], last["ransac_inliers"], last["attempts"], last["live"]) == (lp["best"], lp["best_count"], lp["attempts"], len(q))
        assert np.array_equal(bits(last["T"]), bits(Ts[lp["best"]])) and abs(last["k"] - lp["k"][-1]) <= 1e-12 * lp["k"][-1]
        for chunk in CHUNKS:
            ctx.tune(rej_sac_chunk=chunk)
            got = ctx.correspondences_rejected(S, T_, small["max_dist"], [rej], reciprocal=False, fma=True)
            same_list(got, base, (value, chunk))
            same_result(ctx.last_sample_consensus(), last, (value, chunk))
            assert got[3] == base[3]
    ctx.tune(rej_sac_chunk=0)


# ------------------------------------------------------------------ 3. thresholds on a d2

@pytest.fixture(scope="module")
def pass_one(mvr, ctx, small):
    """pass 1: the dedicated entry at the working threshold, for T[0] and T[1] (which do not depend on the threshold)"""
    load(ctx, small)
    ctx.tune(rej_sac_chunk=0)
    found = ctx.correspondences(S, T_, small["max_dist"], reciprocal=False)
    same_list(found, (small["q"], small["m"], small["d"]), "the search returns the planted pairs")
    got = run(mvr, ctx, small)
    verify(small, got, check_c=True)
    assert got[3]["attempts"] == 2 and got[3]["best_attempt"] == 0 and got[3]["inliers"] >= 0.966 * len(small["q"])
    Ts = [t.reshape(4, 4).T for t in got[4]["T"]]
    P, Q = small["src"][small["q"], :3], small["tgt"][small["m"], :3]
    return Ts, P, Q, R.d2_f32(Ts[0], P, Q), R.d2_f32(Ts[0], P, Q, fma=True)


def test_a_threshold_exactly_on_a_d2_is_strict(mvr, ctx, small, pass_one):
    Ts, P, Q, plain, _ = pass_one
    load(ctx, small)
    i, value = R.find_tie(plain, R.candidates(plain))
    assert value * value == float(plain[i])                      # the tie exists in the reference's d2
    tied = int((bits(plain) == bits(plain[i:i + 1])[0]).sum())
    up = float(np.nextafter(value, math.inf))
    at = run(mvr, ctx, small, value=value)                        # pass 2
    verify(small, at, value=value)
    above = run(mvr, ctx, small, value=up)
    verify(small, above, value=up)
    for got in (at, above):
        assert np.array_equal(bits(got[4]["T"][0].reshape(4, 4).T), bits(Ts[0])) and got[3]["attempts"] == 2 and got[3]["best_attempt"] == 0
    print("tie: pair %d, value %.17g, attempt 0 counts %d at it and %d one ulp above (%d pairs have that d2)"
          % (i, value, at[4]["inliers"][0], above[4]["inliers"][0], tied))
    assert small["q"][i] not in at[0] and small["q"][i] in above[0]
    assert above[4]["inliers"][0] - at[4]["inliers"][0] == tied >= 1


def test_a_threshold_between_plain_and_fma_d2(mvr, ctx, small, pass_one):
    Ts, P, Q, plain, fused = pass_one
    load(ctx, small)
    q, m = small["q"], small["m"]
    i, value = R.find_between(plain, fused, R.candidates(plain))
    want = {fma: R.inlier_mask(Ts[0], P, Q, value, fma=fma) for fma in (False, True)}
    assert want[False][i] != want[True][i] and want[False].sum() != want[True].sum()      # the two reference answers differ
    for fma in (False, True):      # attempt 0 wins under both arithmetics, so the survivors are the inliers of T[0]
        assert int(R.inlier_mask(Ts[1], P, Q, value, fma=fma).sum()) < int(want[fma].sum())
    ded = run(mvr, ctx, small, value=value)                       # the dedicated entry: no fma, by rule C5
    verify(small, ded, value=value)
    assert ded[4]["inliers"][0] == want[False].sum() and np.array_equal(ded[0], q[want[False]])
    rej = rej_of(mvr, small, value=value)
    for fma in (True, False):
        got = ctx.correspondences_rejected(S, T_, small["max_dist"], [rej], reciprocal=False, fma=fma)
        last = ctx.last_sample_consensus()
        assert last["best_attempt"] == 0 and np.array_equal(bits(last["T"]), bits(Ts[0])), fma
        assert np.array_equal(got[0], q[want[fma]]) and np.array_equal(got[1], m[want[fma]]) and last["ransac_inliers"] == want[fma].sum(), fma
    print("between: pair %d, plain d2 %.9g, fma d2 %.9g, value %.17g: %d survive plain, %d with fma"
          % (i, plain[i], fused[i], value, want[False].sum(), want[True].sum()))


# ------------------------------------------------------------------ 4. C10 round by round

@pytest.mark.parametrize("name", ["creeping", "shedding"])
def test_refinement_round_by_round(mvr, ctx, hard, name):
    case = hard[name]
    load(ctx, case)
    q, m, d, P, Q = pairs_of(case)
    ref = R.run(case["src"], case["tgt"], case["q"], case["m"], case["d"], case["value"], 0, True, case["seed"])
    full = run(mvr, ctx, case)                                     # no cap: stops by set equality
    verify(case, full, check_c=True)
    star = full[3]["refine_rounds"]
    print("%s: %d refine rounds on the GPU, %d in the reference; survivors %d" % (name, star, ref["refine_rounds"], full[3]["inliers"]))
    assert star == ref["refine_rounds"] >= 4
    runs = [run(mvr, ctx, case, refine=False)]                     # run 0
    verify(case, runs[0], refine=False)
    sizes = [runs[0][3]["inliers"]]
    for r in range(1, star + 2):
        got = run(mvr, ctx, case, max_iterations=r)
        verify(case, got, max_iterations=r)
        res, prev = got[3], runs[-1]
        # the loop is the same for every cap (the host test shows that it consumes two attempts at most)
        assert np.array_equal(bits(res["ransac_T"]), bits(full[3]["ransac_T"])) and res["ransac_inliers"] == full[3]["ransac_inliers"], r
        assert (res["attempts"], res["best_attempt"]) == (full[3]["attempts"], full[3]["best_attempt"]), r
        assert res["refine_rounds"] == min(r, star), (r, res["refine_rounds"])
        mask = R.inlier_mask(res["T"], P, Q, case["value"])
        same_list(got, (q[mask], m[mask], d[mask]), r)                # its own T's inliers
        if r <= star:
            pm = np.isin(q, prev[0])
            ok, dr, dt = R.close_to(res["T"], kabsch(P[pm].astype(np.float64), Q[pm].astype(np.float64))[0])
            assert ok, (r, dr, dt)                                      # the refit of the round before's survivors
            assert np.array_equal(got[0], prev[0]) == (r == star), r    # the set changes until round R*, and not in it
        else:
            same_run(got, runs[star], "a cap beyond the last round")
        # the stage record of a chain: the device's count word, after an odd and an even number of rounds
        ch = ctx.reject_correspondences(S, T_, case["q"], case["m"], case["d"], [rej_of(mvr, case, max_iterations=r)])
        same_list(ch, got, r)
        assert (ch[3][0]["n_in"], ch[3][0]["n_out"], float(ch[3][0]["threshold"])) == (res["live"], res["inliers"], 0.0), r
        same_result(ctx.last_sample_consensus(), res, r)
        runs.append(got)
        sizes.append(res["inliers"])
    same_run(full, runs[star], "the uncapped run is run R*")
    print("%s: survivors after rounds 0 .. %d: %s (reference %s)" % (name, star + 1, sizes, [int(k.sum()) for _, k in ref["rounds"]]))
    assert sizes[:star + 1] == [int(k.sum()) for _, k in ref["rounds"]]
    if name == "shedding":
        assert sum(1 for a, b in zip(runs, runs[1:star]) if set(b[0]) < set(a[0])) >= 2      # rounds that only lose pairs


def test_rounding_level_threshold(mvr, ctx, hard):
    case = hard["rounding_level"]
    load(ctx, case)
    got = run(mvr, ctx, case)
    verify(case, got, check_c=False, check_refit=False)              # (a), (b), (d), (e), (f): the checks that need no reference
    res = got[3]
    print("rounding level: %d attempts, %d of %d after RANSAC, %d after %d refine rounds" % (res["attempts"], res["ransac_inliers"], res["valid"], res["inliers"], res["refine_rounds"]))
    again = run(mvr, ctx, case)
    same_run(again, got, "twice")


# ------------------------------------------------------------------ 5. the unit of length

@pytest.mark.parametrize("name", ["planted_257", "graded_100000", "creeping"])
def test_the_unit_of_length_changes_nothing(mvr, ctx, hard, name):
    case = SC.build()[name] if name == "planted_257" else hard[name]
    load(ctx, case)
    base = run(mvr, ctx, case)
    assert base[3]["found"]
    for k in SC.UNITS:
        sc = SC.scaled(case, k)
        load(ctx, sc)
        got = run(mvr, ctx, sc)
        f = np.float32(2.0) ** k
        for key in RESULT_KEYS:
            assert got[3][key] == base[3][key], (name, k, key, got[3][key], base[3][key])
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and np.array_equal(bits(got[2]), bits(base[2] * f * f)), (name, k)
        for key in ("status", "query", "match", "inliers"):
            assert np.array_equal(got[4][key], base[4][key]), (name, k, key)
        assert np.array_equal(got[4]["k"].view(np.uint64), base[4]["k"].view(np.uint64)), (name, k)
        Tg, Tb = got[4]["T"].reshape(-1, 4, 4), base[4]["T"].reshape(-1, 4, 4)      # column-major: [:, 3, :3] is the translation
        unit = np.ones((4, 4), np.float32)
        unit[3, :3] = f
        assert np.array_equal(bits(Tg), bits(Tb * unit)), (name, k, "the traced T")
        for key in ("T", "ransac_T"):
            assert np.array_equal(bits(got[3][key]), bits(base[3][key] * unit.T)), (name, k, key)


# ------------------------------------------------------------------ 6. truncation, and the last of two stages

def test_outputs_truncate_at_their_caps(mvr, ctx, hard):
    case = hard["planted_1023"]
    load(ctx, case)
    full = run(mvr, ctx, case)
    n, kept, att = len(case["q"]), len(full[0]), full[3]["attempts"]
    assert kept > 100 and att > 8
    lib, rej = mvr._lib, rej_of(mvr, case)
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    qi, mi, di = (np.ascontiguousarray(case[k]) for k in ("q", "m", "d"))

    def call(cap, trace_cap, with_trace=True):
        q, m, d = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7.0, np.float32)
        tr = (mvr.RejSacTrace * (att + 1))()
        C.memset(tr, 0x5A, C.sizeof(tr))
        res, cnt = mvr.RejSacResult(), C.c_size_t(12345)
        rc = lib.mvr_reject_sample_consensus(ctx._h, S, T_, qi.ctypes.data_as(i32p), mi.ctypes.data_as(i32p), di.ctypes.data_as(fp), n, C.byref(rej),
                                             C.byref(res), q.ctypes.data_as(i32p), m.ctypes.data_as(i32p), d.ctypes.data_as(fp), cap, C.byref(cnt),
                                             tr if with_trace else None, trace_cap)
        assert rc == 0
        return q, m, d, res, cnt.value, bytes(tr)

    rec = C.sizeof(mvr.RejSacTrace)
    q0, m0, d0, res0, cnt0, tr0 = call(n, att)
    assert cnt0 == kept and np.array_equal(q0[:kept], full[0]) and (q0[kept:] == -7).all() and tr0[att * rec:] == b"\x5A" * rec
    same_result(ctx.last_sample_consensus(), full[3], "the full run")
    for cap, trace_cap in ((kept - 1, att), (1, att - 1), (0, 1), (kept, 0), (7, 3)):
        q, m, d, res, cnt, tr = call(cap, trace_cap)
        assert cnt == kept, (cap, cnt)                                      # *m may exceed cap
        assert bytes(res) == bytes(res0), (cap, trace_cap)
        c = min(cap, kept)
        assert np.array_equal(q[:c], q0[:c]) and np.array_equal(m[:c], m0[:c]) and np.array_equal(bits(d[:c]), bits(d0[:c])), cap
        assert (q[c:] == -7).all() and (m[c:] == -7).all() and (d[c:] == -7.0).all(), cap      # the element past the cap keeps its sentinel
        t = min(trace_cap, att)
        assert tr[:t * rec] == tr0[:t * rec] and tr[t * rec:] == b"\x5A" * ((att + 1 - t) * rec), trace_cap


def test_last_sample_consensus_is_the_second_of_two_stages(mvr, ctx, hard):
    case = hard["planted_2049"]
    load(ctx, case)
    first, second = rej_of(mvr, case, value=2.0, seed=5), rej_of(mvr, case, refine=True, seed=9)
    a = ctx.reject_sample_consensus(S, T_, case["q"], case["m"], case["d"], first)
    b = ctx.reject_sample_consensus(S, T_, a[0], a[1], a[2], second)
    assert a[3]["inliers"] > b[3]["inliers"] >= 3 and a[3]["live"] > b[3]["live"] == a[3]["inliers"]
    ch = ctx.reject_correspondences(S, T_, case["q"], case["m"], case["d"], [first, second])
    same_list(ch, b, "the chain")
    same_result(ctx.last_sample_consensus(), b[3], "the second stage")
    assert [(s["n_in"], s["n_out"]) for s in ch[3]] == [(a[3]["live"], a[3]["inliers"]), (b[3]["live"], b[3]["inliers"])]
