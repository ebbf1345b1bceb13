"""Host tests of the PFH reference (tests/pfh_ref.py), of the cases the GPU tests run (tests/pfh_cases.py) and of what
mvr_cloud_pfh, mvr_feature_knn and mvr_align_prerejective_dim refuse before they touch a GPU."""
import contextlib
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref as AR
import fpfh_cases as FC
import pfh_cases as PC
import pfh_ref as PR
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@contextlib.contextmanager
def align_ref_width(dim):
    """align_ref.feature_knn / eligible reshape their tables to align_ref.DIM floats per row"""
    old, AR.DIM = AR.DIM, dim
    try:
        yield AR
    finally:
        AR.DIM = old


_cases = {}


def case_counts(name, mvr):
    """the reference counts of a case (the queries it is checked on), computed once"""
    if name in _cases:
        return _cases[name]
    queries = None
    if name == "view":
        p = PC.view(mvr)
        hoods = (p, FC.ref_normals(p, PC.VIEW_NORMAL_RADIUS), PC.VIEW_RADIUS)
    elif name == "invalid":
        p = PC.view(mvr)
        q, m, bad = PC.with_invalid(p, FC.ref_normals(p, PC.VIEW_NORMAL_RADIUS))
        hoods = (q, m, PC.VIEW_RADIUS)
    elif name == "box":
        hoods = PC.box()
    elif name == "duplicates":
        hoods = PC.duplicates()
    elif name == "blob":
        hoods, queries = PC.blob(), np.array(PC.BLOB_QUERIES)
    elif name == "patch":
        p = PC.patch(mvr)
        hoods = (p, FC.ref_normals(p, PC.patch_normal_radius(p)), PC.patch_radius(p))
    elif name.startswith("k"):
        p, nrm = PC.knn_cloud()
        _cases[name] = (p, nrm, PR.pfh(p, nrm, k=int(name[1:]))[1])
        return _cases[name]
    p, nrm, radius = hoods
    _cases[name] = (p, nrm, PR.pfh(p, nrm, radius=radius, queries=queries)[1])
    return _cases[name]


CASES = ["view", "invalid", "box", "duplicates", "blob", "patch"] + ["k%d" % k for k in PC.KS]


@pytest.mark.parametrize("name", CASES)
def test_slack_pairs_stay_under_the_cap(name, mvr):
    """a condition on the cases, not a measurement: the GPU tests cannot hide behind slack"""
    p, nrm, c = case_counts(name, mvr)
    share = c["slack"].sum() / max(c["pairs"], 1)
    print("%s: %d points, %d queries, %.1f neighbours (max %d), %d pairs, slack share %.4f, %d of 125 bins used"
          % (name, len(p), len(c["n"]), c["n"].mean(), c["n"].max(), c["pairs"], share, int((c["full"].sum(0) > 0).sum())))
    assert c["pairs"] <= 5.5e6 and share <= PC.SLACK_CAP
    assert (c["sure"] <= c["full"]).all() and (c["full"] <= c["sure"] + c["maybe"]).all()
    assert (c["full"].sum(1) == c["feat"]).all() and (c["feat"] <= c["m"]).all()
    assert c["m"].sum() == c["pairs"]


def test_cases_reach_what_they_are_for(mvr):
    assert (case_counts("blob", mvr)[2]["n"] == PC.BLOB_N).all() and PC.BLOB_N > PC.STAGE
    c = case_counts("box", mvr)[2]
    assert (c["full"].sum(0) > 0).sum() >= 100                           # the joint bins of random normals
    c = case_counts("duplicates", mvr)[2]
    assert (c["feat"] < c["m"]).any()                                    # pairs at f4 == 0 count in m_i alone
    p, nrm, c = case_counts("k1", mvr)
    assert (c["n"] == 0).sum() == 11 and c["n"].max() == 1               # point 0 (invalid) and its ten copies, pushed out by it
    c = case_counts("k64", mvr)[2]
    assert (c["n"][c["valid"]] >= 63).all() and (c["n"][~c["valid"]] == 0).all()      # (an entry with a NaN normal leaves the list)
    assert (~case_counts("invalid", mvr)[2]["valid"]).sum() > 20


@pytest.mark.parametrize("name", ["box", "duplicates"])
def test_vectorised_reference_equals_the_naive_loop(name, mvr):
    p, nrm, radius = PC.box() if name == "box" else PC.duplicates()
    hoods = PR.hoods_radius(p, nrm, radius)
    queries = np.sort(np.random.default_rng(1).choice(len(p), 25, replace=False))
    if name == "duplicates":
        queries = np.unique(np.concatenate([queries, [0, 3, 4]]))       # point 0 and its copies, a point and its copy
    c = PR.counts(p, nrm, hoods, queries)
    assert np.array_equal(PR.naive(p, nrm, hoods, queries), c["full"])
    assert np.array_equal(PR.counts(p, nrm, PR.hoods_radius(p, nrm, radius, brute=True), queries)["full"], c["full"])


def test_vectorised_reference_equals_the_naive_loop_on_tiny_clouds_and_in_k_mode():
    for n in FC.TINY_SIZES:
        p, nrm, radius = PC.tiny(n)
        for r in (radius, 2.5, 100.0):
            hoods = PR.hoods_radius(p, nrm, r, brute=True)
            c = PR.counts(p, nrm, hoods)
            assert np.array_equal(PR.naive(p, nrm, hoods, np.arange(n)), c["full"])
            if r == radius:
                assert (c["n"] == 1).all() and (c["full"] == 0).all()
    p, nrm, radius = PC.tiny(5)
    for k in (1, 2, 16):
        hoods = PR.hoods_knn(p, nrm, *PR.knn_lists(p, k))
        c = PR.counts(p, nrm, hoods)
        assert list(c["n"]) == [min(k, 5)] * 5
        assert np.array_equal(PR.naive(p, nrm, hoods, np.arange(5)), c["full"])


def test_rows_sum_to_the_share_of_pairs_with_features(mvr):
    for name in ("box", "duplicates", "k16"):
        p, nrm, c = case_counts(name, mvr)
        rows = PR.rows_from_counts(c["full"], c["n"], c["valid"])
        live = c["m"] > 0
        want = 100.0 * c["feat"][live] / c["m"][live]
        assert np.abs(rows[live].astype(F64).sum(1) - want).max() < 1e-3
        assert (rows[c["n"] == 1] == 0).all() and np.isnan(rows[c["n"] == 0]).all()
    # (float)c * (100.0f / (float)m) on a hand-made row
    r = PR.rows_from_counts(np.array([[3, 0, 7] + [0] * 122]), np.array([5]), np.array([True]))
    assert r[0, 0] == F32(3) * (F32(100) / F32(10)) and r[0, 2] == F32(7) * (F32(100) / F32(10))


def test_reference_is_invariant_under_rigid_motion():
    p, nrm, radius = PC.box()
    p, nrm = p[:1200], nrm[:1200]
    q, m = FC.moved(p, nrm)
    a, ca = PR.pfh(p, nrm, radius=6.0)
    b, cb = PR.pfh(q, m, radius=6.0)
    same = ca["n"] == cb["n"]                                             # (a neighbour at the rim may fall either way)
    d = np.abs(a[same].astype(F64) - b[same].astype(F64)).sum(1)
    other = np.abs(a[same].astype(F64) - a[same][::-1].astype(F64)).sum(1)
    print("same neighbour count %d of %d; L1 distance of a row before and after: median %.4f, max %.3f (of 200; unrelated "
          "points %.1f)" % (same.sum(), len(same), np.median(d), d.max(), np.median(other)))
    assert same.mean() > 0.9 and np.median(d) < 0.5 and np.median(d) < 0.02 * np.median(other)


# ------------------------------------------------------------------ the matcher and the aligner at 125 floats per row

def m1_scalar(q, t):
    acc = F32(0)
    for b in range(len(q)):
        diff = F32(q[b]) - F32(t[b])
        acc = F32(acc + F32(diff * diff))
    return acc


def test_reference_matcher_and_replay_at_width_125():
    rng = np.random.default_rng(8)
    q = (rng.uniform(0, 100, (9, 125)) * rng.uniform(0, 1, (9, 125)) ** 4).astype(F32)
    t = (rng.uniform(0, 100, (40, 125)) * rng.uniform(0, 1, (40, 125)) ** 4).astype(F32)
    t[7, 100] = np.nan
    q[4, 124] = np.inf
    with align_ref_width(125) as A:
        idx, d2 = A.feature_knn(q, t, 3)
        pts = np.ones((9, 4), F32)
        pts[:, :3] = rng.uniform(-5, 5, (9, 3))
        elig = A.eligible(pts, q)
    assert AR.DIM == 33
    assert list(elig) == [0, 1, 2, 3, 5, 6, 7, 8]
    assert (idx[4] == AR.NONE).all() and np.isinf(d2[4]).all() and not (idx == 7).any()
    for i in (0, 3, 8):                                                   # the stand-in: M1 as a scalar loop over all 125 components
        D = np.array([m1_scalar(q[i], t[j]) for j in range(40)], F32)
        D[7] = np.inf
        o = np.lexsort((np.arange(40), D.view(np.uint32)))[:3]
        assert list(idx[i]) == list(o) and np.array_equal(d2[i].view(np.uint32), D[o].view(np.uint32))
    # the last 92 components decide: the 33-float prefix alone gives other lists
    assert not np.array_equal(AR.feature_knn(q[:, :33], t[:, :33], 3)[0], idx)
    tp = np.ones((40, 4), F32)
    tp[:, :3] = rng.uniform(-5, 5, (40, 3))
    status, src, tgt = AR.replay(pts, tp, elig, idx[elig], 50, 3, 11, 0.3)
    assert set(status) <= {0, 1} and (status == 1).any() and (status == 0).any()
    for i in range(50):
        assert len(set(src[i])) == 3 and all(tgt[i, j] in idx[src[i, j]] for j in range(3))


# ------------------------------------------------------------------ the C-ABI and the wrapper

def test_library_exports_the_new_symbols(mvr):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    for name in ("mvr_cloud_pfh", "mvr_align_prerejective_dim"):
        assert name in mvr.SIGNATURES and re.search(r" T %s$" % name, r.stdout, re.M), name
    assert C.sizeof(mvr.PfhParams) == 16 and mvr.PFH_DIM == 125 == PC.DIM and mvr.PFH_STAGE == PC.STAGE
    hdr = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    assert re.search(r"#define MVR_PFH_DIM 125\b", hdr) and re.search(r"#define MVR_PFH_STAGE %d\b" % PC.STAGE, hdr)
    assert hasattr(mvr.Context, "pfh")


def test_refusals_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                                    # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    out, cnt, nb = (C.c_float * 125)(*[9.0] * 125), (C.c_uint32 * 125)(*[9] * 125), (C.c_uint32 * 1)(9)
    f = L.mvr_cloud_pfh
    ok = mvr.PfhParams(2.5, 0, 0)
    assert f(None, 0, C.byref(ok), out, cnt, nb) == mvr.E_ARG
    assert f(ctx, 0, None, out, cnt, nb) == mvr.E_ARG
    for slot in (-1, mvr.MAX_SLOTS, 1 << 20):
        assert f(ctx, slot, C.byref(ok), out, cnt, nb) == mvr.E_ARG
    bad = [(0.0, 0), (2.5, 16), (-1.0, 0), (math.nan, 0), (math.inf, 0), (math.nan, 16), (0.0, -1), (0.0, 65), (0.0, 1 << 20), (-2.0, 8)]
    for radius, k in bad:
        for fma in (0, 1):
            assert f(ctx, 0, C.byref(mvr.PfhParams(radius, k, fma)), out, cnt, nb) == mvr.E_ARG, (radius, k)
    assert list(out) == [9.0] * 125 and list(cnt) == [9] * 125 and nb[0] == 9
    # the matcher: 33 and 125 alone; the aligner's new entry the same
    rows = (C.c_float * 250)(*[1.0] * 250)
    idx, d2 = (C.c_uint32 * 4)(*[9] * 4), (C.c_float * 4)(*[9.0] * 4)
    for dim in (0, 3, 32, 34, 66, -33, 124, 126, 128, 250, -125):
        assert L.mvr_feature_knn(ctx, rows, 1, rows, 1, dim, 1, idx, d2) == mvr.E_ARG
    for k in (0, 65):
        assert L.mvr_feature_knn(ctx, rows, 1, rows, 1, 125, k, idx, d2) == mvr.E_ARG
    assert L.mvr_feature_knn(None, rows, 1, rows, 1, 125, 1, idx, d2) == mvr.E_ARG
    assert list(idx) == [9] * 4 and list(d2) == [9.0] * 4
    al = L.mvr_align_prerejective_dim
    res = mvr.PrerejResult()
    res.inliers = 77
    prm = mvr.PrerejParams(10, 3, 2, 0.5, 2.0, 0.25, 1, 0)
    for dim in (0, 32, 34, 124, 126, -125):
        assert al(ctx, 0, 1, rows, rows, dim, C.byref(prm), None, C.byref(res), None) == mvr.E_ARG
    assert al(None, 0, 1, rows, rows, 125, C.byref(prm), None, C.byref(res), None) == mvr.E_ARG
    assert al(ctx, 0, 1, rows, rows, 125, None, None, C.byref(res), None) == mvr.E_ARG
    assert al(ctx, 0, 1, None, rows, 125, C.byref(prm), None, C.byref(res), None) == mvr.E_ARG
    assert al(ctx, 0, mvr.MAX_SLOTS, rows, rows, 125, C.byref(prm), None, C.byref(res), None) == mvr.E_ARG
    assert al(ctx, 0, 1, rows, rows, 125, C.byref(mvr.PrerejParams(10, 9, 2, 0.5, 2.0, 0.25, 1, 0)), None, C.byref(res), None) == mvr.E_ARG
    assert res.inliers == 77
    assert fake.raw == b"\0" * 256


def test_wrapper_refuses_its_arguments_itself(mvr):
    c = mvr.Context.__new__(mvr.Context)                                   # no device: the checks come before any use of it
    for kw in (dict(), dict(radius=2.5, k=16), dict(k=0), dict(k=65), dict(k=-3), dict(radius=0.0), dict(radius=-1.0),
               dict(radius=math.nan), dict(radius=math.inf)):
        with pytest.raises(ValueError):
            mvr.Context.pfh(c, 0, **kw)


# ------------------------------------------------------------------ the kernels' resources

def test_pfh_kernels_use_no_scratch(built, tmp_path):
    from test_fpfh_host import _usage
    assert "mvr_pfh.hip" in built.HIP_SOURCES
    use = _usage(built, tmp_path, "mvr_pfh.hip")
    print([(re.sub(r"^_ZN3mvr(12_GLOBAL__N_1)?\d+", "", n), v, s, l) for n, v, s, l in use])
    assert len(use) == 1 + 2 + 2 + 1 + 4, use      # normals, staged x fma, tiled x fma, the k mode, the 125-float matcher per bucket
    assert all(s == 0 for _, _, s, _ in use), [(n, s) for n, _, s, _ in use if s]
    record, hist = 2 * 16, 128 * 4
    assert all(l == PC.STAGE * record + hist for n, _, _, l in use if "pfh_radius_kernel" in n)
    assert all(l == 2 * PC.STAGE * record + hist for n, _, _, l in use if "pfh_tiled_kernel" in n)
    assert all(l == 64 * record + hist for n, _, _, l in use if "pfh_knn_kernel" in n)
    assert all(l == 64 * 128 * 4 for n, _, _, l in use if "feature_knn_kernel" in n)      # one tile of 64 rows padded to 128 floats
    assert all(v <= 64 for n, v, _, _ in use if "pfh_" in n)              # eight waves per SIMD as far as registers go
    assert all(v <= 256 for _, v, _, _ in use)
