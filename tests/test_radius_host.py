"""CPU tests of the radius search's reference (tests/radius_ref.py) and of what mvr_radius_search refuses before it touches a GPU.

The reference's SETS equal scipy's cKDTree.query_ball_point in f64 wherever no pair lies within 1e-6 (relative) of r2.  Measured
on tests/walk_cases.py at the fraction_of_a_cell and several_cells radii, self and cross: on the cases used here (CASES below) no
row has such a pair -- an excluded share of 0, asserted.  Rows with one (of the rows of the side; all at several_cells), on cases
NOT used for that reason: duplicates_41 8 / 5000 and 7 / 1200, every_target_duplicated 16 / 6000, exactly_257_and_1025 2 / 1025,
huge_coordinates 6 / 2200 and 1 / 600, one_query and queries_far_from_everything 6 / 2500, patch_at_0 2 / 6000 and 2 / 1500,
planar_sheet 3 / 1500."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import normals_ref as N
import radius_ref as R
import walk_cases as W
from conftest import PKG, ROOT

F32 = np.float32
CASES = ("patch_far_1e5", "patch_far_1e6", "collinear", "size_65", "size_257", "size_1025")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_sets_equal_the_kd_tree_in_f64(mvr, name):
    from scipy.spatial import cKDTree
    q, t = W.get(name, mvr)
    tree = cKDTree(t[:, :3].astype(np.float64))
    bar = 1.0e-6
    for side, qq in (("self", t), ("cross", q)):
        Q = qq[:, :3].astype(np.float64)
        for tag in ("fraction_of_a_cell", "several_cells"):
            r = W.radii(name, t)[tag]
            r2 = float(R.clamp_r2(r))
            o, idx, d2 = R.radius_search(qq, t, r)
            mine = R.rows(o, idx)
            wide = tree.query_ball_point(Q, np.sqrt(r2 * (1.0 + bar)) * (1.0 + 1e-12))
            narrow = tree.query_ball_point(Q, np.sqrt(r2 * (1.0 - bar)) * (1.0 - 1e-12))
            excluded = 0
            for i in range(len(qq)):
                if len(wide[i]) != len(narrow[i]):               # a pair within `bar` of r2: the f32 rule may differ
                    excluded += 1
                    continue
                assert sorted(mine[i].tolist()) == sorted(wide[i]), (name, side, tag, i)
            print("%s %s %s: %d of %d rows excluded" % (name, side, tag, excluded, len(qq)))
            assert excluded == 0, (name, side, tag, excluded)


@pytest.mark.parametrize("fma", [False, True])
def test_max_nn_rows_are_the_prefix_of_the_knn_list(mvr, fma):
    for name in ("duplicates_41", "size_65", "lattice_3d"):
        q, t = W.get(name, mvr)
        q = q[:400]
        ki, kd = N.knn_brute(q, t, 64, fma=fma)
        for tag, r in W.radii(name, t).items():
            r2 = R.clamp_r2(r)
            full = R.radius_search(q, t, r, fma=fma)
            for mx in (1, 9, 64):
                o, idx, d2 = R.radius_search(q, t, r, max_nn=mx, fma=fma)
                inside = (ki[:, :mx] != N.NONE) & (kd[:, :mx] <= r2)
                assert np.array_equal(np.diff(o.astype(np.int64)), inside.sum(1)), (name, tag, mx)
                assert np.array_equal(idx, ki[:, :mx][inside]) and np.array_equal(bits(d2), bits(kd[:, :mx][inside])), (name, tag, mx)
                assert np.array_equal(np.diff(o.astype(np.int64)), np.minimum(np.diff(full[0].astype(np.int64)), mx))
            # chunking changes nothing
            assert all(np.array_equal(a, b) for a, b in zip(full, R.radius_search(q, t, r, fma=fma, chunk=7)))


def test_lattice_row_lengths_in_closed_form(mvr):
    """d2 == r2 counts (RS1): at one lattice step a point has one neighbour per axis on a face of the lattice and two inside, plus
    itself; at the in-plane diagonal (float)(r * r) is 0.125 exactly and the diagonals of every pair of axes come in"""
    _, t = W.get("lattice_3d", mvr)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(15), np.arange(14), indexing="ij"), -1).reshape(-1, 3)
    inner = [((g[:, a] > 0) & (g[:, a] < d - 1)).astype(np.int64) for a, d in enumerate((16, 15, 14))]
    step = 3 + sum(inner) + 1
    diag = step + sum((1 + inner[a]) * (1 + inner[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    for tag, want in (("lattice_distance", step), ("lattice_diagonal", diag)):
        r = W.radii("lattice_3d", t)[tag]
        for fma in (False, True):
            o, idx, d2 = R.radius_search(t, t, r, fma=fma)
            assert np.array_equal(np.diff(o.astype(np.int64)), want), (tag, fma)
            assert (d2 == R.clamp_r2(r)).any() and d2.max() == R.clamp_r2(r)
            own = o[:-1].astype(np.int64)
            assert np.array_equal(idx[own], np.arange(len(t))) and not d2[own].any()      # the point itself leads its row


def test_non_finite_rule():
    rng = np.random.default_rng(2)
    t = W.cloud(rng.standard_normal((300, 3)))
    q = W.cloud(rng.standard_normal((100, 3)))
    t[[5, 17], 0] = np.nan; t[40, 1] = np.inf; t[41, :3] = -np.inf
    q[[3, 9], 2] = (np.nan, np.inf)
    for fma in (False, True):
        o, idx, d2 = R.radius_search(q, t, 50.0, fma=fma)
        lens = np.diff(o.astype(np.int64))
        assert lens[3] == 0 and lens[9] == 0 and (np.delete(lens, [3, 9]) == 296).all()
        assert not np.isin(idx, [5, 17, 40, 41]).any() and np.isfinite(d2).all()
        # a pair of finite points whose d2 overflows is no pair, whatever the radius
        far = np.concatenate([t[:3], W.cloud([[3.0e19, 0.0, 0.0]])])
        o, idx, d2 = R.radius_search(far, far, 1.0e30, fma=fma)
        assert np.diff(o.astype(np.int64)).tolist() == [3, 3, 3, 1]
    o, idx, d2 = R.radius_search(q, t[:0], 1.0)
    assert len(o) == 101 and not o.any() and len(idx) == 0
    o, idx, d2 = R.radius_search(q[:0], t, 1.0)
    assert o.tolist() == [0]


def test_the_arithmetic_of_the_total_bound(mvr):
    """RS8 (the refusal itself needs 2^31 entries and is not run)"""
    assert mvr.RADIUS_MAX_TOTAL == 2 ** 31 - 1
    assert R.max_total_ok(2 ** 31 - 1, 0, True) and not R.max_total_ok(2 ** 31, 0, True)
    assert R.max_total_ok(10, 2 ** 31, False) and not R.max_total_ok(10, 2 ** 31, True) and R.max_total_ok(10, 2 ** 31 - 1, True)


def test_library_exports_and_refuses_before_the_gpu(mvr):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    for name in ("mvr_radius_search", "mvr_radius_default_params"):
        assert name in mvr.SIGNATURES and re.search(r" T %s$" % name, r.stdout, re.M), name
    hdr = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    assert re.search(r"#define MVR_RADIUS_STAGE %d\b" % mvr.RADIUS_STAGE, hdr) and re.search(r"#define MVR_RADIUS_MAX_TOTAL 0x7FFFFFFFull", hdr)
    assert C.sizeof(mvr.RadiusParams) == 24 and hasattr(mvr.Context, "radius_search")
    prm = mvr.RadiusParams(9.0, 9, 9, 9)
    mvr._lib.mvr_radius_default_params(C.byref(prm))
    assert (prm.radius, prm.max_nn, prm.sorted, prm.fma_dist) == (0.0, 0, 1, 0)
    mvr._lib.mvr_radius_default_params(None)
    f = mvr._lib.mvr_radius_search
    o, idx, d2, total = (C.c_uint64 * 4)(*[9] * 4), (C.c_uint32 * 4)(*[9] * 4), (C.c_float * 4)(*[9.0] * 4), C.c_size_t(9)
    for prm in (mvr.RadiusParams(2.5, 0, 1, 0), mvr.RadiusParams(-1.0, 0, 1, 0)):      # without a context: nothing to search, nothing written
        for qs, ts in ((0, 1), (-1, 0), (0, mvr.MAX_SLOTS)):
            assert f(None, qs, ts, C.byref(prm), o, idx, d2, 4, C.byref(total)) == mvr.E_ARG
    assert f(None, 0, 1, None, o, idx, d2, 4, C.byref(total)) == mvr.E_ARG
    assert list(o) == [9] * 4 and list(idx) == [9] * 4 and list(d2) == [9.0] * 4 and total.value == 9


def test_wrapper_refuses_its_arguments_itself(mvr):
    c = mvr.Context.__new__(mvr.Context)                                   # no device: the checks come before any use of it
    for args, kw in (((0, 1, 0.0), {}), ((0, 1, -1.0), {}), ((0, 1, float("nan")), {}), ((0, 1, float("inf")), {}), ((0, 1, 1.0), dict(max_nn=-1)),
                     ((0, 1, 1.0), dict(max_nn=1 << 32)), ((-1, 1, 1.0), {}), ((0, mvr.MAX_SLOTS, 1.0), {}), ((0, 1, 0.0), dict(count_only=True))):
        with pytest.raises(ValueError):
            mvr.Context.radius_search(c, *args, **kw)


# ------------------------------------------------------------------ the kernels' resources

def test_radius_kernels_use_no_scratch(built, mvr, tmp_path):
    from test_fpfh_host import _usage
    assert "mvr_radius.hip" in built.HIP_SOURCES
    use = [u for u in _usage(built, tmp_path, "mvr_radius.hip") if "radius_" in u[0]]      # (hipCUB's kernels are not ours to bound)
    print([(re.sub(r"^_ZN3mvr(12_GLOBAL__N_1)?\d+", "", n), v, s, l) for n, v, s, l in use])
    assert len(use) == 2 + 2 + 2 + 1, use              # count x fma, fill x fma, long x fma, the long rows' write
    assert all(s == 0 for _, _, s, _ in use), [(n, s) for n, _, s, _ in use if s]
    assert all(l == mvr.RADIUS_STAGE * 8 for n, _, _, l in use if "radius_fill_kernel" in n)       # the staged keys: 20 waves per compute unit
    assert all(l == 0 for n, _, _, l in use if "radius_fill_kernel" not in n)
    assert all(v <= 64 for _, v, _, _ in use)          # eight waves per SIMD as far as registers go
