"""CPU tests of the moving-least-squares smoothing that need no device: the two f64 routes of the numpy reference
(tests/mls_ref.py) agree, also after rounding to f32, the reference's error against the generator's noise-free points is what its
docstring records, the inputs of the GPU tests exclude no point from value comparisons, the library exports mvr_cloud_mls and rejects bad arguments before touching the
GPU, and the kernels of csrc/mvr_mls.hip use no scratch memory while those of csrc/mvr_knn.hip keep their registers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mls_cases as K
import mls_ref as R
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64


synth = K.synth


@pytest.fixture(scope="module")
def view200k(mvr):
    return synth(mvr, 0, 200000)


def rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


def along_normal(xyz64, clean, true_n):
    return ((xyz64 - clean[:, :3].astype(F64)) * true_n[:, :3].astype(F64)).sum(1)


# ------------------------------------------------------------------ the reference against the ground truth

def test_reference_reproduces_the_ground_truth_figures(view200k):
    """View 0 of config 3 at 200 000 points, 3 000 sampled queries, errors rms along the true normal, measured here:

        radius 2.5 mm (111.4 neighbours, at least 46): input 0.1002 mm, order 1 0.0240 mm, order 2 0.0198 mm;
                      smallest gap 0.195, largest condition 323, the two routes 1.1e-13 apart
        radius 1.0 mm (18.6 neighbours, at least 6):   order 1 0.0276 mm, order 2 0.0501 mm (too few neighbours overfit);
                      smallest gap 0.053, largest condition 1.5e5, the two routes 1.1e-13 apart
    """
    p, true_n, clean = view200k
    rows = K.sample_rows(len(p), K.VIEW_SEED)
    e_in = rms(along_normal(p[rows, :3].astype(F64), clean[rows], true_n[rows]))
    got = {}
    for radius in (2.5, 1.0):
        F = R.fit(p, radius, rows=rows)
        assert F["keep"].all() and F["count"].min() >= 6 and F["fit"].all()
        for order in (1, 2):
            res = R.result(p, F, order, rows=rows)
            got[radius, order] = rms(along_normal(res["xyz64"], clean[rows], true_n[rows]))
            assert R.excluded(F, order).sum() == 0
        diff = max(np.nanmax(F["diff_plane"]), np.nanmax(F["diff_poly"]))
        print("radius %g: %.1f neighbours (at least %d), input %.4f, order 1 %.4f, order 2 %.4f mm; smallest gap %.3g, largest "
              "condition %.3g, routes apart %.2e mm" % (radius, F["count"].mean(), F["count"].min(), e_in, got[radius, 1], got[radius, 2],
                                                     F["gap"].min(), F["cond"].max(), diff))
        assert diff <= 1e-11                              # two f64 routes: rounding at |z| = 917 is 1.1e-13
        assert F["gap"].min() > 0.04 and F["cond"].max() < 1e6
    assert abs(e_in - 0.1002) < 0.0005
    assert abs(got[2.5, 1] - 0.0240) < 0.0005 and abs(got[2.5, 2] - 0.0198) < 0.0005
    assert got[1.0, 2] > got[1.0, 1] > got[2.5, 1]        # at 18 neighbours the quadratic overfits


def test_the_two_routes_agree_after_rounding(view200k):
    """every 40th point of the 200k view at radius 2.5 mm: the two routes' f64 coordinates, 1e-13 mm apart, round to the same f32
    in every coordinate, for the plane projection and for the polynomial alike"""
    p = view200k[0]
    rows = np.arange(0, len(p), 40)
    F = R.fit(p, 2.5, rows=rows)
    assert F["keep"].all() and F["fit"].all()
    assert np.nanmax(F["diff_poly"]) <= 1e-11 and np.nanmax(F["diff_plane"]) <= 1e-11
    for a, b in (("plane", "plane_b"), ("poly", "poly_b")):
        assert np.array_equal(F[a].astype(F32).view(np.uint32), F[b].astype(F32).view(np.uint32)), a
    assert not np.array_equal(F["plane"].astype(F32).view(np.uint32), F["poly"].astype(F32).view(np.uint32))


@pytest.mark.parametrize("radius", [2.5, 1.0])
def test_the_gpu_tests_inputs_exclude_nothing(view200k, radius):
    """the excluded share of the inputs tests/test_gpu_mls.py compares values on, against its cap of 0.  Measured: radius 2.5:
    0 of 200 000, smallest gap 0.162, largest condition 463, routes 1.1e-13 mm apart; radius 1.0: 0 of 199 999 (one point has
    fewer than 3 neighbours), smallest gap 0.0058, largest condition 1.1e9, routes 7.3e-11 mm apart, 1 curvature the reference
    cannot pin; the fma chain changes no neighbour set at either radius"""
    p = view200k[0]
    F = R.fit(p, radius)
    for order in (1, 2):
        bad = R.excluded(F, order)
        print("radius %g order %d: %d of %d kept points excluded (share %.2e); smallest gap %.3g, largest condition %.3g, routes "
              "apart %.2e" % (radius, order, int(bad.sum()), int(F["keep"].sum()), bad.sum() / max(1, F["keep"].sum()),
                              np.nanmin(F["gap"][F["keep"]]), np.nanmax(F["cond"][F["keep"]]), np.nanmax(np.where(F["keep"], F["diff_poly"], 0.0))))
        assert bad.sum() == 0
    flat = R.curvature_unpinned(F)
    print("radius %g: %d points whose curvature the reference cannot pin, neighbour counts %s" % (radius, int(flat.sum()), sorted(set(F["count"][flat]))))
    assert (F["curv"][flat] < 1e-6).all()                 # (nearly) coplanar neighbours only: three points always are
    assert (F["count"][flat] <= 4).all()                  # ... and on a noisy scan only the sparsest neighbourhoods
    print("radius %g: the fma chain changes a neighbour set: %s" % (radius, R.membership_differs(p, radius)))


def test_the_view_with_non_finite_points_excludes_nothing(mvr):
    """the 20k view with 60 non-finite points, at the radii and distance chains tests/test_gpu_mls.py runs it with.  Measured:
    nothing excluded; curvatures the reference cannot pin: 5 300 of 10 454 kept points at 1 mm (half the kept points have exactly 3
    neighbours), 18 of 19 936 at 2.5 mm"""
    p, bad = K.with_non_finite(synth(mvr, 0, 20000)[0])
    for radius, fma in K.NON_FINITE_RUNS:
        F = R.fit(p, radius, fma=fma)
        ex, flat = R.excluded(F, 2), R.curvature_unpinned(F)
        print("radius %g fma %d: %d of %d kept points excluded, %d curvatures not pinned; smallest gap %.3g, largest condition %.3g"
              % (radius, fma, int(ex.sum()), int(F["keep"].sum()), int(flat.sum()), np.nanmin(F["gap"][F["keep"]]), np.nanmax(F["cond"][F["keep"]])))
        assert ex.sum() == 0 and not F["keep"][bad].any() and (F["curv"][flat] < 1e-6).all()


def test_the_merged_objects_sampled_queries_exclude_nothing(mvr):
    """the 3 000 sampled queries of the twelve views merged under their true poses (2.4 M points), radius 2.5 mm.  Measured: 789
    neighbours, nothing excluded, every curvature pinned, smallest gap 0.395, largest condition 77"""
    p, _, _ = K.merged_object(mvr)
    rows = K.sample_rows(len(p), K.MERGED_SEED)
    F = R.fit(p, 2.5, rows=rows)
    print("merged object: %.0f neighbours, %d of %d excluded, %d curvatures not pinned; smallest gap %.3g, largest condition %.3g"
          % (F["count"].mean(), int(R.excluded(F, 2).sum()), int(F["keep"].sum()), int(R.curvature_unpinned(F).sum()), F["gap"].min(), F["cond"].max()))
    assert F["keep"].all() and R.excluded(F, 2).sum() == 0 and R.curvature_unpinned(F).sum() == 0


# ------------------------------------------------------------------ the reference, by hand

def cloud(xyz):
    p = np.ones((len(xyz), 4), F32)
    p[:, :3] = np.asarray(xyz, F32)
    return p


def test_reference_recovers_an_exact_quadric():
    """points ON z = 900 + 0.02 x^2 - 0.01 x y + 0.015 y^2 + 0.03 x (a polynomial of total degree 2 over a plane stays one over
    any other plane only approximately -- but a quadric sampled finely is fitted to far below the step): the projected point
    lies on the surface, the normal is the surface normal"""
    g = np.stack(np.meshgrid(np.linspace(-3, 3, 61), np.linspace(-3, 3, 61), indexing="ij"), -1).reshape(-1, 2)
    z = 900 + 0.02 * g[:, 0] ** 2 - 0.01 * g[:, 0] * g[:, 1] + 0.015 * g[:, 1] ** 2 + 0.03 * g[:, 0]
    p = cloud(np.c_[g, z])
    mid = np.nonzero((np.abs(g) < 1.0).all(1))[0]
    F = R.fit(p, 1.5, rows=mid)
    res = R.result(p, F, 2, rows=mid)
    x, y = res["xyz64"][:, 0], res["xyz64"][:, 1]
    on = 900 + 0.02 * x ** 2 - 0.01 * x * y + 0.015 * y ** 2 + 0.03 * x
    assert np.abs(res["xyz64"][:, 2] - on).max() < 2e-4  # (f32 storage of z at 900: 6e-5)
    nt = np.c_[-(0.04 * x - 0.01 * y + 0.03), -(-0.01 * x + 0.03 * y), np.ones_like(x)]
    nt /= np.linalg.norm(nt, axis=1, keepdims=True)
    assert np.abs(np.abs((res["normal"].astype(F64) * nt).sum(1)) - 1).max() < 1e-6
    assert (((0 - p[mid, :3]) * res["normal"]).sum(1) >= 0).all()        # towards the viewpoint at the origin


def test_reference_counts_and_drops():
    line = cloud([[x, 3.0, 900.0] for x in (0, 1, 2, 3, 4, 14, 40)])
    assert list(R.counts(line, 1.0)) == [2, 3, 3, 3, 2, 1, 1] and list(R.kept_index(line, 1.0)) == [1, 2, 3]
    line[2, 1] = np.nan
    assert list(R.counts(line, 1.0)) == [2, 2, 0, 2, 2, 1, 1] and len(R.kept_index(line, 1.0)) == 0
    F = R.fit(line, 2.0)
    assert list(F["count"]) == [2, 3, 0, 3, 2, 1, 1] and list(R.result(line, F, 2)["index"]) == [1, 3]
    for n in (0, 1, 2):
        assert len(R.kept_index(line[:n], 100.0)) == 0
    none = np.full((5, 4), np.nan, F32)
    assert len(R.kept_index(none, 1.0)) == 0 and not R.fit(none, 1.0)["keep"].any()


def test_within_one_ulp():
    a = F32([1.0, -1.0, 0.0, 917.0])
    assert R.within_one_ulp(a, a).all()
    assert R.within_one_ulp(np.nextafter(a, F32(np.inf)), a).all() and R.within_one_ulp(np.nextafter(a, F32(-np.inf)), a).all()
    two = np.nextafter(np.nextafter(a, F32(np.inf)), F32(np.inf))
    assert not R.within_one_ulp(two, a).any()


# ------------------------------------------------------------------ the C-ABI

def test_library_exports_mvr_cloud_mls(mvr):
    assert "mvr_cloud_mls" in mvr.SIGNATURES
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    assert re.search(r" T mvr_cloud_mls$", r.stdout, re.M)
    assert C.sizeof(mvr.MlsParams) == 48                  # double, int, double, int, int, float[3], int: the header's layout


def test_mls_rejects_bad_arguments_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                    # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    n = C.c_size_t(7)
    idx = (C.c_uint32 * 4)(9, 9, 9, 9)
    curv = (C.c_float * 4)(9, 9, 9, 9)

    def prm(radius=2.5, order=2, g=0.0, normals=0, orient=0, vp=(0.0, 0.0, 0.0), fma=0):
        return mvr.MlsParams(radius, order, g, normals, orient, (C.c_float * 3)(*vp), fma)

    f = L.mvr_cloud_mls
    assert f(None, 0, 1, C.byref(prm()), C.byref(n), idx, curv) == mvr.E_ARG
    assert f(ctx, 0, 1, None, C.byref(n), idx, curv) == mvr.E_ARG
    for d, s in ((-1, 0), (0, -1), (mvr.MAX_SLOTS, 0), (0, mvr.MAX_SLOTS)):
        assert f(ctx, d, s, C.byref(prm()), C.byref(n), idx, curv) == mvr.E_ARG
    for r in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert f(ctx, 0, 1, C.byref(prm(radius=r)), C.byref(n), idx, curv) == mvr.E_ARG
    for g in (-1.0, math.nan, math.inf, -math.inf):
        assert f(ctx, 0, 1, C.byref(prm(g=g)), C.byref(n), idx, curv) == mvr.E_ARG
    for o in (-1, 3, 1 << 20):
        assert f(ctx, 0, 1, C.byref(prm(order=o)), C.byref(n), idx, curv) == mvr.E_ARG
    for o in (-1, 2):
        assert f(ctx, 0, 1, C.byref(prm(orient=o)), C.byref(n), idx, curv) == mvr.E_ARG
    for vp in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf)):
        assert f(ctx, 0, 1, C.byref(prm(vp=vp)), C.byref(n), idx, curv) == mvr.E_ARG
    assert n.value == 7 and list(idx) == [9] * 4 and list(curv) == [9.0] * 4
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the kernels' resources

def _usage(built, tmp_path, name):
    """[(kernel, VGPRs, scratch bytes per lane)] from the compiler's remarks for one source file (device code only)"""
    src = os.path.join(ROOT, PKG, "csrc", name)
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / (name + ".o")),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    return [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
             int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))) for b in blocks]


def test_mls_kernels_use_no_scratch(built, tmp_path):
    use = _usage(built, tmp_path, "mvr_mls.hip")
    own = [(n, v, s) for n, v, s in use if "mls_" in n]
    print(own)
    assert len(own) == 5, own                             # the fit x fma x order 2, the curvature gather
    assert all(s == 0 for _, _, s in use), [(n, s) for n, _, s in use if s]


def test_knn_kernels_keep_their_registers(built, tmp_path):
    """Moments, the Jacobi rotation and the eigenvector pick moved into csrc/mvr_plane.h: the kernels of mvr_knn.hip are
    allocated what they were before the move (the counts of the parent commit, gfx950)"""
    before = {"knn_kernelILi8E": 100, "knn_kernelILi16E": 150, "knn_kernelILi32E": 116, "knn_kernelILi64E": 181,
              "normals_knn_kernelILi8E": 100, "normals_knn_kernelILi16E": 151, "normals_knn_kernelILi32E": 117,
              "normals_knn_kernelILi64E": 182, "normals_radius_kernelIL": 54}
    use = _usage(built, tmp_path, "mvr_knn.hip")
    assert len(use) == 18 and all(s == 0 for _, _, s in use)
    for name, v, _ in use:
        key = [k for k in before if re.search(r"\d+" + re.escape(k), name)]
        assert len(key) == 1, name
        assert v == before[key[0]], (name, v, before[key[0]])
