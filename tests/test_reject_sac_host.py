"""CPU tests of the sample-consensus rejector: the numpy reference (tests/reject_sac_ref.py) against itself on the planted cases
of tests/reject_sac_cases.py -- the planted pairs recovered, the loop's arithmetic, the share of well-conditioned samples that
check (c) of the GPU test relies on --, the layout of the new and the extended structs against the Python bindings, the
arguments refused before any device is touched, and the exported symbols.  No GPU compute here."""
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
    for kernel, times in (("rsac_valid_kernel", 1), ("rsac_gather_kernel", 1), ("rsac_hypotheses_kernel", 1), ("rsac_count_kernel", 6), ("rsac_flag_kernel", 2)):
        assert sum(kernel in n for n, _, _, _ in use) == times, (kernel, use)      # count: (1, 2, 4 registers) x fma
    assert all(s == 0 for _, _, s, _ in use), use
    count = sorted(l for n, _, _, l in use if "rsac_count_kernel" in n)
    assert count == [256, 256, 512, 512, 1024, 1024]  # one counter per attempt of the chunk
    # four blocks of 256 threads per CU are four waves per SIMD: 512 / 4 = 128 VGPRs a wave
    assert all(v <= 128 for _, v, _, _ in use)
