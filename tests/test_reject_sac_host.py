"""CPU tests of the sample-consensus rejector: the numpy reference (tests/reject_sac_ref.py) against itself on the planted cases
of tests/reject_sac_cases.py -- the planted pairs recovered, the loop's arithmetic, the share of well-conditioned samples that
check (c) of the GPU test relies on --, the layout of the new and the extended structs against the Python bindings, the
arguments refused before any device is touched, and the exported symbols; and what each hardening case of
reject_sac_cases.build_hard was built for (the second half of the file).  No GPU compute here."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import reject_sac_cases as SC
import reject_sac_ref as R
from conftest import PKG, ROOT
from sac_ref import K_MARGIN


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def cases():
    return SC.build()


@pytest.fixture(scope="module")
def ran(cases):
    return {name: R.run(c["src"], c["tgt"], c["q"], c["m"], c["d"], c["value"], c["max_iterations"], c["refine"], c["seed"])
            for name, c in cases.items() if name in SC.HOST_NAMES}


def test_case_names_and_sizes(cases):
    assert tuple(cases) == SC.NAMES
    assert {0, 2, 3, 65, 257, 1025, 1500, SC.RC.BIG} <= {len(c["q"]) for c in cases.values()}


def test_reference_keeps_exactly_the_planted_pairs(cases, ran):
    seen = 0
    for name, r in ran.items():
        c = cases[name]
        q, m, d = R.sort_list(c["q"], c["m"], c["d"])
        assert r["found"] == c["found"], name
        assert r["min_margin"] >= K_MARGIN, (name, r["min_margin"])
        if c["planted"] is None:
            assert np.array_equal(r["q"], q) and np.array_equal(r["m"], m) and np.array_equal(R.bits(r["d"]), R.bits(d)), name
            assert r["inliers"] == len(q) and np.array_equal(r["T"], np.eye(4, dtype=np.float32))
            continue
        seen += 1
        keep = c["planted"]
        assert np.array_equal(r["q"], q[keep]) and np.array_equal(r["m"], m[keep]) and np.array_equal(R.bits(r["d"]), R.bits(d[keep])), name
        assert r["inliers"] == r["ransac_inliers"] == len(keep) >= 3, name
        ok, dr, dt = R.close_to(r["T"], c["motion"])
        assert ok or name in ("three", "duplicates"), (name, dr, dt)
    assert seen >= 10
    half = cases["planted_1500"]
    assert len(half["planted"]) == 750 and half["value"] == 0.05 and len(half["q"]) == 1500
    assert ran["planted_1500_refine"]["refine_rounds"] >= 1 and ran["planted_30"]["refine_rounds"] >= 1
    assert ran["all_inliers"]["attempts"] == ran["all_inliers"]["iterations"] == 1
    u = ran["unrelated"]
    assert not u["found"] and u["iterations"] == u["attempts"] == 71 and u["inliers"] == 400        # PCL's off-by-one: max_iterations + 1
    assert ran["few_valid"]["valid"] == 2 and ran["few_valid"]["attempts"] == 0 and ran["two"]["attempts"] == 0
    assert ran["non_finite"]["valid"] < ran["non_finite"]["live"] == 257


def test_most_samples_are_well_conditioned_where_check_c_is_asserted(cases, ran):
    n = 0
    for name, r in ran.items():
        if cases[name]["check_c"]:
            assert r["iterations"] >= 1 and r["well"] >= 0.9, (name, r["well"])
            n += 1
    assert n >= 8
    big = cases["big"]
    rb = R.run(big["src"], big["tgt"], big["q"], big["m"], big["d"], big["value"], big["max_iterations"], big["refine"], big["seed"])
    assert rb["well"] >= 0.9 and rb["min_margin"] >= K_MARGIN and np.array_equal(rb["q"], big["planted"])


def test_loop_arithmetic():
    # an all-inlier first attempt: w = 1, pno clamps to DBL_EPSILON, k = log(0.01) / log(eps) < 1: the loop stops after one attempt
    lp = R.replay_loop([1], [300], 300, 1000)
    assert lp["iterations"] == 1 and lp["k"][0] == math.log(0.01) / math.log(np.finfo(np.float64).eps) < 1.0
    # half inliers: k = log(0.01) / log(1 - 1 / 8)
    k = math.log(0.01) / math.log(1.0 - 0.125)
    st, cn = [1] * 35, [0] * 34 + [0]
    cn[3] = 50
    lp = R.replay_loop(st, cn, 100, 1000)
    assert lp["best"] == 3 and lp["iterations"] == 35 == math.ceil(k) and lp["k"][-1] == k and lp["k"][2] > 1e15
    # strictly greater: the first of equal counts stays; a skipped attempt counts towards nothing but `skipped`
    lp = R.replay_loop([1, 0, 1] + [1] * 33, [50, 0, 50] + [3] * 33, 100, 1000)
    assert (lp["best"], lp["best_count"], lp["iterations"], lp["skipped"], lp["attempts"]) == (0, 50, 35, 1, 36)
    lp = R.replay_loop([0, 1, 1], [0, 0, 0], 10, 1)
    assert (lp["iterations"], lp["skipped"], lp["attempts"], lp["best"], lp["best_count"]) == (2, 1, 3, 1, 0)      # max_iterations + 1 counted
    lp = R.replay_loop([0] * 10, [0] * 10, 10, 1)
    assert (lp["iterations"], lp["skipped"]) == (0, 10)                                                              # skipped < 10 * max_iterations
    with pytest.raises(AssertionError):
        R.replay_loop([1, 1], [300, 0], 300, 1000)                                                                     # one attempt too many


def test_reference_arithmetic_is_f32_in_the_rules_order():
    rng = np.random.default_rng(0)
    P, Q = rng.uniform(0, 10, (50, 3)).astype(np.float32), rng.uniform(0, 10, (50, 3)).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3] = rng.standard_normal((3, 4)).astype(np.float32)
    d2 = R.d2_f32(T, P, Q)
    f = np.float32
    for i in (0, 7, 49):
        x, y, z = P[i]
        t = [f(f(f(f(T[r, 0] * x) + f(T[r, 1] * y)) + f(T[r, 2] * z)) + T[r, 3]) for r in range(3)]
        dx, dy, dz = f(t[0] - Q[i, 0]), f(t[1] - Q[i, 1]), f(t[2] - Q[i, 2])
        assert d2[i] == f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
    exact = ((P.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3] - Q) ** 2).sum(1)
    assert np.abs(R.d2_f32(T, P, Q, fma=True) - exact).max() <= 1e-4 * exact.max()
    # strictly below value * value, the product taken in f64
    one = np.array([[1.0, 0, 0]], np.float32)
    assert not R.inlier_mask(np.eye(4, dtype=np.float32), one, one + np.float32([0.25, 0, 0]), 0.25)[0]
    assert R.inlier_mask(np.eye(4, dtype=np.float32), one, one + np.float32([0.25, 0, 0]), np.nextafter(0.25, 1.0))[0]


def test_struct_layout_equals_the_bindings(mvr, tmp_path):
    src = tmp_path / "layout.c"
    fields = (["sizeof(mvr_rejector)"] + ["offsetof(mvr_rejector, %s)" % f for f in ("kind", "value", "min_correspondences", "max_iterations", "refine", "seed")]
              + ["sizeof(mvr_rej_sac_result)"] + ["offsetof(mvr_rej_sac_result, %s)" % f for f in
                                                 ("found", "live", "valid", "inliers", "ransac_inliers", "iterations", "attempts", "skipped", "best_attempt",
                                                  "refine_rounds", "k", "T", "ransac_T")]
              + ["sizeof(mvr_rej_sac_trace)"] + ["offsetof(mvr_rej_sac_trace, %s)" % f for f in ("status", "query", "match", "T", "inliers", "k")]
              + ["(size_t)MVR_REJ_SAMPLE_CONSENSUS"])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mvr_hip.h"\nint main(void) {\n  size_t v[] = {%s};\n'
                   '  for (size_t k = 0; k < sizeof v / sizeof v[0]; ++k) printf("%%zu ", v[k]);\n'
                   '  mvr_rejector r = {MVR_REJ_TRIMMED, 0.8, 12u};\n'
                   '  printf("%%d %%u %%d %%llu\\n", r.kind, r.max_iterations, r.refine, (unsigned long long)r.seed);\n  return 0;\n}\n' % ", ".join(fields))
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    exp = []
    for S in (mvr.Rejector, mvr.RejSacResult, mvr.RejSacTrace):
        exp += [C.sizeof(S)] + [getattr(S, f[0]).offset for f in S._fields_]
    assert got == exp + [mvr.REJ_SAMPLE_CONSENSUS, mvr.REJ_TRIMMED, 0, 0, 0]      # (a positional initialiser of the old three fields)
    assert mvr.REJ_SAMPLE_CONSENSUS == 5 and mvr.REJ_KINDS["sample_consensus"] == 5
    # the old fields have not moved
    assert (mvr.Rejector.kind.offset, mvr.Rejector.value.offset, mvr.Rejector.min_correspondences.offset) == (0, 8, 16)
    r = mvr.rejector("sample_consensus", 0.05, max_iterations=200, refine=True, seed=2 ** 40 + 3)
    assert (r.kind, r.value, r.min_correspondences, r.max_iterations, r.refine, r.seed) == (5, 0.05, 0, 200, 1, 2 ** 40 + 3)
    r = mvr.rejector("trimmed", 0.8, 12)
    assert (r.kind, r.value, r.min_correspondences, r.max_iterations, r.refine, r.seed) == (mvr.REJ_TRIMMED, 0.8, 12, 0, 0, 0)


def test_symbols_are_exported(mvr):
    for name in ("mvr_reject_sample_consensus", "mvr_ctx_last_sample_consensus"):
        assert getattr(mvr._lib, name) is not None
    for name in ("RejSacResult", "RejSacTrace", "REJ_SAMPLE_CONSENSUS"):
        assert hasattr(mvr, name)
    assert hasattr(mvr.Context, "reject_sample_consensus") and hasattr(mvr.Context, "last_sample_consensus")


def test_null_context_and_null_arguments_are_refused(mvr):
    lib = mvr._lib
    r = mvr.rejector("sample_consensus", 0.05)
    res = mvr.RejSacResult()
    res.found, res.inliers, res.k = 7, 77, 7.5
    cnt = C.c_size_t(77)
    q = (C.c_int32 * 3)(0, 1, 2)
    d = (C.c_float * 3)(1.0, 1.0, 1.0)
    out = (C.c_int32 * 3)(9, 9, 9)
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def call(ctx, rej, result, m):
        return lib.mvr_reject_sample_consensus(ctx, 0, 1, C.cast(q, i32p), C.cast(q, i32p), C.cast(d, fp), 3, rej, result, C.cast(out, i32p),
                                               C.cast(out, i32p), None, 3, m, None, 0)
    assert call(None, C.byref(r), C.byref(res), C.byref(cnt)) == mvr.E_ARG
    assert lib.mvr_ctx_last_sample_consensus(None, C.byref(res)) == mvr.E_ARG
    assert (res.found, res.inliers, res.k) == (7, 77, 7.5) and cnt.value == 77 and list(out) == [9, 9, 9]      # nothing written


def test_kernels_use_no_scratch_and_fit_four_blocks_per_cu(built, tmp_path):
    assert "mvr_reject_sac.hip" in built.HIP_SOURCES
    src = os.path.join(ROOT, PKG, "csrc", "mvr_reject_sac.hip")
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "mvr_reject_sac.o"),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    use = [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
            int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
           for b in blocks]
    print(use)
    for kernel, times in (("rsac_valid_kernel", 1), ("rsac_gather_kernel", 1), ("rsac_hypotheses_kernel", 1), ("rsac_flag_kernel", 2)):
        assert sum(kernel in n for n, _, _, _ in use) == times, (kernel, use)
    # the shared counting kernel (mvr_ransac.h) over this file's model: (1, 2, 4 registers) x fma
    count = sorted(l for n, _, _, l in use if "19ransac_count_kernel" in n and "RigidModel" in n)
    assert len(count) == sum("count_kernel" in n for n, _, _, _ in use) == 6, use
    assert all(s == 0 for _, _, s, _ in use), use
    assert count == [256, 256, 512, 512, 1024, 1024]  # one counter per attempt of the chunk
    # four blocks of 256 threads per CU are four waves per SIMD: 512 / 4 = 128 VGPRs a wave
    assert all(v <= 128 for _, v, _, _ in use)


# ------------------------------------------------------------------ the hardening cases: what they were chosen for, on the reference alone

def ref_run(c, **kw):
    a = dict(value=c["value"], max_iterations=c["max_iterations"], refine=c["refine"], seed=c["seed"])
    a.update(kw)
    return R.run(c["src"], c["tgt"], c["q"], c["m"], c["d"], **a)


@pytest.fixture(scope="module")
def hard():
    return SC.build_hard()


@pytest.fixture(scope="module")
def hard_ran(hard):
    return {name: ref_run(c, check_margin=name != "rounding_level") for name, c in hard.items()}


def test_hard_case_names_and_shapes(hard, hard_ran):
    assert tuple(hard) == SC.HARD_NAMES
    for name in SC.GRADED_NAMES + ("graded_shared", "graded_non_finite"):
        c, r = hard[name], hard_ran[name]
        assert len(c["q"]) == 3000 and r["found"] and r["min_margin"] >= K_MARGIN, name
        # the loop reads every register of the counting kernel's chunk; about a fifth of the pairs count at best
        assert r["attempts"] > 256 and 0.15 < r["ransac_inliers"] / r["valid"] < 0.3, (name, r["attempts"], r["ransac_inliers"])
    sh = hard["graded_shared"]
    assert len(np.unique(sh["q"])) == 3000 and len(np.unique(sh["m"])) == 3000 - 600 and np.array_equal(sh["m"][0::5], sh["m"][1::5])
    nf, rn = hard["graded_non_finite"], hard_ran["graded_non_finite"]
    assert rn["valid"] < rn["live"] == 3000 and not np.isfinite(nf["src"][nf["q"][-1], :3]).all() and nf["q"][-1] == nf["q"].max()
    for name in SC.EDGE_NAMES:
        c, r = hard[name], hard_ran[name]
        assert r["valid"] == r["live"] == len(c["q"]) == int(name.split("_")[1]) and r["min_margin"] >= K_MARGIN
        q, m, d = R.sort_list(c["q"], c["m"], c["d"])
        assert np.array_equal(r["q"], q[c["planted"]]) and r["well"] >= 0.9, name


@pytest.mark.parametrize("far", [f for f in SC.FARS if f > 0])
def test_far_frames_tell_the_rule_from_contracted_arithmetic(hard, hard_ran, far):
    """the point of the far cases: on at least one counted attempt the loop consumes, C4 as the rule writes it and C4 with its
    products contracted into fmas give different counts; near the origin (and on every earlier case) they give the same"""
    c, r = hard["graded_%g" % far], hard_ran["graded_%g" % far]
    q, m, _ = R.sort_list(c["q"], c["m"], c["d"])
    P, Q = c["src"][q, :3], c["tgt"][m, :3]
    flipped = attempts = 0
    for st, T, n in zip(r["status"], r["Ts"], r["counts"]):
        if st != R.COUNTED:
            continue
        a, b = R.inlier_mask(T, P, Q, c["value"]), R.inlier_mask(T, P, Q, c["value"], contracted=True)
        assert a.sum() == n
        flipped += int((a != b).sum())
        attempts += int(a.sum() != b.sum())
    print("far %g: %d decisions flipped, the count of %d of %d attempts changed" % (far, flipped, attempts, r["iterations"]))
    assert attempts >= 1, far


def test_contracted_reference_is_what_it_says():
    rng = np.random.default_rng(1)
    P = (rng.uniform(0, 10, (40, 3)) + 1e5).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3] = rng.standard_normal((3, 4)).astype(np.float32)
    x = R.transform_f32(T, P, contracted=True)[0]
    L, f = np.longdouble, np.float32
    for i in (0, 13, 39):
        inner = f(L(T[0, 1]) * L(P[i, 1]) + L(f(T[0, 0] * P[i, 0])))
        assert x[i] == f(f(L(T[0, 2]) * L(P[i, 2]) + L(inner)) + T[0, 3])
    assert (np.stack(R.transform_f32(T, P)) != np.stack(R.transform_f32(T, P, contracted=True))).any()


def _small(hard=None):
    pair = SC.small_motion(SC.SMALL_SEED)
    q, m, d = SC.small_list(pair)
    return pair, q, m, d


def test_small_motion_pairs_are_the_nearest_neighbours():
    pair, q, m, d = _small()
    s, t = pair["src"][:, :3].astype(np.float64), pair["tgt"][:, :3].astype(np.float64)
    D = ((s[:, None, :] - t[None, :, :]) ** 2).sum(2)
    assert 1600 < len(s) < 1800 and np.array_equal(D.argmin(1), pair["match_of"])
    two = np.partition(D, 1, axis=1)
    # the planted target within the search distance by a wide margin, every other target beyond it
    assert np.sqrt(two[:, 0].max()) < 0.7 * pair["max_dist"] and np.sqrt(two[:, 1].min()) > pair["max_dist"]
    assert 890.0 < np.linalg.norm(s.mean(0)) < 910.0


def test_thresholds_on_a_d2_exist_and_split_the_arithmetics():
    """section 3's searches on the reference's own T of attempt 0: an exact tie, and a threshold between a pair's plain and fma
    d2; at both the loop consumes the same two attempts, attempt 0 wins by far and no stop decision is near k"""
    pair, q, m, d = _small()
    P, Q = pair["src"][q, :3], pair["tgt"][m, :3]
    r0 = R.run(pair["src"], pair["tgt"], q, m, d, pair["value"], 0, False, pair["seed"])
    assert r0["attempts"] == 2 and r0["best_attempt"] == 0 and r0["ransac_inliers"] >= 0.966 * len(q)
    T0, T1 = r0["Ts"]
    plain, fused = R.d2_f32(T0, P, Q), R.d2_f32(T0, P, Q, fma=True)
    differ = int((R.bits(plain) != R.bits(fused)).sum())
    among = R.candidates(plain)
    assert differ >= 10 and len(among) >= 20
    i, value = R.find_tie(plain, among)
    assert value * value == float(plain[i])                       # the tie exists
    up = float(np.nextafter(value, np.inf))
    assert not R.inlier_mask(T0, P, Q, value)[i] and R.inlier_mask(T0, P, Q, up)[i]
    assert R.inlier_mask(T0, P, Q, up).sum() - R.inlier_mask(T0, P, Q, value).sum() == (R.bits(plain) == R.bits(plain[i:i + 1])[0]).sum()
    j, between = R.find_between(plain, fused, among)
    a, b = R.inlier_mask(T0, P, Q, between), R.inlier_mask(T0, P, Q, between, fma=True)
    assert a[j] != b[j] and a.sum() != b.sum()                     # the two reference answers differ
    print("small motion: %d of %d pairs differ between plain and fma; tie on pair %d at %.17g, between on pair %d at %.17g"
          % (differ, len(q), i, value, j, between))
    for v in (value, up, between):
        for fma in (False, True):
            counts = [int(R.inlier_mask(T, P, Q, v, fma).sum()) for T in (T0, T1)]
            lp = R.replay_loop([1, 1], counts, len(q), 1000)
            assert lp["best"] == 0 and lp["attempts"] == 2 and lp["min_margin"] >= K_MARGIN, (v, fma, counts)
            assert counts[0] >= 0.966 * len(q) and counts[0] - counts[1] >= 20, (v, fma, counts)
    # the tight threshold: both arithmetics run to the cap, so the fma route consumes the attempts the dedicated entry traces
    for fma in (False, True):
        rt = R.run(pair["src"], pair["tgt"], q, m, d, SC.SMALL_TIGHT, SC.SMALL_TIGHT_CAP, False, pair["seed"], fma=fma)
        assert rt["attempts"] == rt["iterations"] == SC.SMALL_TIGHT_CAP + 1 and rt["k"] > SC.SMALL_TIGHT_CAP + 50 and rt["found"], (fma, rt["k"])


def _set_changes(r):
    return [(int((b & ~a).sum()), int((a & ~b).sum())) for (_, a), (_, b) in zip(r["rounds"], r["rounds"][1:])]


def _decision_margin(c, r):
    q, m, _ = R.sort_list(c["q"], c["m"], c["d"])
    P, Q = c["src"][q, :3], c["tgt"][m, :3]
    return min(float(np.abs(np.sqrt(R.d2_f32(T, P, Q).astype(np.float64)) - c["value"]).min()) for T, _ in r["rounds"])


@pytest.mark.parametrize("name", ["creeping", "shedding"])
def test_refinement_takes_rounds_that_change_the_set(hard, hard_ran, name):
    c, r = hard[name], hard_ran[name]
    ch = _set_changes(r)
    rounds = r["refine_rounds"]
    print(name, "rounds", rounds, "gained / lost per round", ch, "sizes", [int(k.sum()) for _, k in r["rounds"]])
    assert len(r["rounds"]) == rounds + 1 and rounds >= 4
    assert all(g + l > 0 for g, l in ch[:-1]) and ch[-1] == (0, 0)          # at least three rounds change the set; the last does not
    if name == "shedding":      # rounds in which the set only loses pairs, before the last: what the "entries that differ" counter must see
        assert sum(1 for g, l in ch[:-1] if g == 0 and l > 0) >= 2
    else:
        assert sum(1 for g, l in ch[:-1] if g > 0) >= 3
    # no pair of any round within a cast's reach of the threshold: the rounds do not depend on the estimator's last bit
    assert _decision_margin(c, r) >= R.cast_bar(r["T"], c["src"][:, :3]), name
    assert r["min_margin"] >= K_MARGIN and r["ransac_inliers"] >= 0.966 * len(c["q"])
    # the identical loop for every cap; the cap of the loop is the cap of the rounds
    for cap in (1, 2, 3, 4, 5, 6, 8, 1000):
        rc = ref_run(c, max_iterations=cap)
        assert (rc["attempts"], rc["iterations"], rc["best_attempt"], rc["ransac_inliers"]) == (r["attempts"], r["iterations"], r["best_attempt"], r["ransac_inliers"])
        assert rc["attempts"] <= 2 and rc["min_margin"] >= K_MARGIN and rc["refine_rounds"] == min(cap, rounds), (name, cap)
        Tc, Ic = r["rounds"][min(cap, rounds)]
        assert np.array_equal(R.bits(rc["T"]), R.bits(Tc)) and rc["inliers"] == Ic.sum()


def test_rounding_level_case_goes_where_no_other_does(hard, hard_ran):
    c, r = hard["rounding_level"], hard_ran["rounding_level"]
    assert c["value"] == 2.0 ** -14 == float(np.spacing(np.float32(900.0))) and c["refine"]
    sizes = [int(k.sum()) for _, k in r["rounds"]]
    print("rounding level:", r["attempts"], "attempts,", r["refine_rounds"], "rounds, sizes", sizes)
    assert r["found"] and r["refine_rounds"] >= 2 and min(sizes) < 0.5 * max(sizes)      # a refit that loses most of what it was made from


def test_units_scale_exactly(hard):
    for name in ("planted_257", "graded_100000", "creeping"):
        c = SC.build()[name] if name == "planted_257" else hard[name]
        for k in SC.UNITS:
            s = SC.scaled(c, k)
            f = 2.0 ** k
            assert np.array_equal(s["src"][:, :3].astype(np.float64), c["src"][:, :3].astype(np.float64) * f)
            assert np.array_equal(s["tgt"][:, :3].astype(np.float64), c["tgt"][:, :3].astype(np.float64) * f)
            assert np.array_equal(s["d"].astype(np.float64), c["d"].astype(np.float64) * f * f) and s["value"] == c["value"] * f
            assert np.array_equal(s["src"][:, 3], c["src"][:, 3]) and (s["value"] * s["value"]) == (c["value"] * c["value"]) * f * f
