"""CPU tests of the ISS keypoints that need no device: the numpy reference (tests/iss_ref.py) checked against itself and against
a second implementation, the conditions on the shared inputs (tests/iss_cases.py) under which the GPU test compares flags
exactly, the exported symbol and its argument refusals, and the resources of the kernels of csrc/mvr_iss.hip (no scratch memory).

Measured here on the reference: view 19 951 salient / 1 715 keypoints (29.1 and 12.0 neighbours per ball), closest ratio 3.4e-4
from its threshold, closest pair of neighbouring saliencies 1.1e-6 apart; view_tight 14 263 / 1 734, 2.8e-6, 1.1e-6; box
2 974 / 142, 1.2e-4, 5.4e-5; non_finite 5 916 / 434, 3.5e-4, 1.9e-6.  The smallest e3 / e1 of a salient point is 1.5e-4.  The
second implementation (cyclic Jacobi, shuffled order of the sums) gives the same flags and saliencies within 1e-12 relative.
On the targets of the walk cases (iss_cases.WALK) every point is decided except all 5 000 of
planar_sheet (rank-deficient; none is salient) -- every_target_duplicated at 5 grid edges: at 3.5 it has 20 balls of three
distinct points twice, rank 2, 8 of which the reference calls salient on rounding alone; keypoints: 68 / 66 / 63 on the patches at 0 / 1e5 / 1e6 mm (10 exact saliency ties between
neighbours at 1e6), 132 on lattice_3d (1 832 ties), 6 and 12 on the two cluster cases, 1 to 4 elsewhere."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fpfh_cases as FC
import iss_cases as IC
import iss_ref as R
import mls_cases as K
import normals_ref as NR
from conftest import PKG, ROOT
from outlier_ref import finite_mask, within_r2

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ the reference against itself

def test_brute_force_neighbourhoods_equal_the_kd_trees():
    p = K.with_non_finite(FC.box(700)[0], count=20)[0]
    fin = np.nonzero(finite_mask(p))[0]
    for radius, fma in ((3.0, False), (2.0, True)):
        flat, offs = NR.radius_sets(p, radius, fma)
        r2 = F32(radius * radius)
        for i in range(len(p)):
            mine = fin[within_r2(p[i, :3], p[fin, :3], r2, fma)] if finite_mask(p[i:i + 1])[0] else fin[:0]
            assert np.array_equal(flat[offs[i]:offs[i + 1]], mine), i
    assert (np.diff(offs)[~finite_mask(p)] == 0).all() and not np.isin(flat, np.nonzero(~finite_mask(p))[0]).any()


def jacobi_eigenvalues(S):
    """the library's solver restated (csrc/mvr_plane.h: scatter_eigenvalues), vectorised over the matrices: descending"""
    A = S.copy()
    for _ in range(12):
        off = A[:, 0, 1] ** 2 + A[:, 0, 2] ** 2 + A[:, 1, 2] ** 2
        dia = A[:, 0, 0] ** 2 + A[:, 1, 1] ** 2 + A[:, 2, 2] ** 2
        live = off > 1e-40 * dia
        if not live.any():
            break
        for P, Q, Rr in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[:, P, Q]
            go = live & (apq != 0)
            safe = np.where(go, apq, 1.0)
            theta = (A[:, Q, Q] - A[:, P, P]) / (2.0 * safe)
            t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            t, s, c = np.where(go, t, 0.0), np.where(go, s, 0.0), np.where(go, c, 1.0)
            A[:, P, P] -= t * apq
            A[:, Q, Q] += t * apq
            arp, arq = A[:, Rr, P].copy(), A[:, Rr, Q].copy()
            A[:, P, Q] = A[:, Q, P] = np.where(go, 0.0, apq)
            A[:, Rr, P] = A[:, P, Rr] = c * arp - s * arq
            A[:, Rr, Q] = A[:, Q, Rr] = s * arp + c * arq
    return np.sort(np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), axis=1)[:, ::-1]


@pytest.mark.parametrize("name", ["view", "box"])
def test_a_second_implementation_gives_the_same_flags(name, mvr):
    """the library's Jacobi instead of eigvalsh and the sums in a shuffled order: what two correct implementations differ by"""
    c, r = IC.reference(name, mvr)
    (flat, offs), n_sets = r["sets"]
    rng = np.random.default_rng(1)
    owner = np.repeat(np.arange(len(c["p"])), np.diff(offs))
    o = np.lexsort((rng.random(len(flat)), owner))                       # shuffled within every neighbourhood
    S, cnt = R.scatter(c["p"], flat[o], offs)
    w = jacobi_eigenvalues(S)
    with np.errstate(invalid="ignore", divide="ignore"):
        sal = (cnt >= c["min_neighbors"]) & np.isfinite(w).all(1) & (w[:, 2] >= 0) & (w[:, 1] / w[:, 0] < c["gamma_21"]) & \
              (w[:, 2] / w[:, 1] < c["gamma_32"]) & (w[:, 2] > 0)
    assert np.array_equal(sal, r["salient"])
    mine = np.where(sal, w[:, 2], 0.0)
    rel = np.abs(mine - r["saliency"])[sal] / r["saliency"][sal]
    print("%s: saliencies of the two implementations agree within %.1e relative" % (name, rel.max()))
    assert rel.max() < 1e-12
    assert np.array_equal(R.nms(mine, n_sets[0], n_sets[1], c["min_neighbors"])[1], r["keypoint"])


# ------------------------------------------------------------------ the conditions of an exact comparison

@pytest.mark.parametrize("name", IC.EXACT)
def test_conditions_of_an_exact_comparison_hold(name, mvr):
    """conditions on the inputs: where one fails the input changes, not GAP.  Beside the two gaps, every salient point has
    e3 > 1e-6 e1: the solvers round e3 to about 1e-16 e1, so its relative error stays four orders under GAP / 4"""
    for fma in (False, True) if name in IC.FMA_CASES else (False,):
        c, r = IC.reference(name, mvr, fma)
        m = R.margins(r)
        print("%s fma=%d: %d points, %d salient, %d keypoints, %.1f / %.1f neighbours; closest ratio %.2e, closest pair %.2e, %d ties, "
              "smallest e3 / e1 %.2e" % (name, fma, len(c["p"]), r["salient"].sum(), r["keypoint"].sum(), r["salient_count"].mean(),
                                         r["nms_count"][r["salient"]].mean(), m["ratio"], m["pair"], m["ties"], m["e3"]))
        assert m["ratio"] > R.GAP and m["pair"] > R.GAP and m["ties"] == 0 and m["e3"] > 1e-6
        assert R.decided(r).all()
        assert r["salient"].sum() > 0.5 * finite_mask(c["p"]).sum() and 100 < r["keypoint"].sum() < 0.15 * len(c["p"])
        assert (r["saliency"][~r["valid"]] == 0).all() and (r["salient_count"][~r["valid"]] == 0).all() and not r["keypoint"][~r["valid"]].any()


def test_the_view_is_the_one_measured(mvr):
    c, r = IC.reference("view", mvr)
    assert (int(r["salient"].sum()), int(r["keypoint"].sum())) == (19951, 1715)
    assert (r["r32"][r["salient_count"] >= 5] < 0.09).all()               # gamma_32 never rejects at the defaults ...
    c, t = IC.reference("view_tight", mvr)
    ok = t["salient_count"] >= 5
    rej21 = ok & ~(t["r21"] < c["gamma_21"])
    rej32 = ok & ~rej21 & ~(t["r32"] < c["gamma_32"])
    assert rej21.sum() > 1000 and rej32.sum() > 1000                      # ... and both reject a visible share here
    assert not np.array_equal(t["keypoint"], r["keypoint"])


def test_the_other_cases_reach_the_edges(mvr):
    for n in FC.TINY_SIZES:
        c, r = IC.reference("tiny_%d" % n, mvr)
        assert len(r["saliency"]) == n and (r["salient_count"] == 1).all() and not r["salient"].any() and len(r["index"]) == 0
    c, r = IC.reference("duplicates", mvr)
    assert R.margins(r)["ties"] >= 600 and r["keypoint"].sum() > 50        # exact copies: equal saliencies, both kept
    p = c["p"]
    twins = np.nonzero((p[4::5, :3] == p[3::5, :3][:len(p[4::5])]).all(1))[0]
    assert np.array_equal(r["saliency"][4::5][twins], r["saliency"][3::5][twins])
    c, r = IC.reference("all_identical", mvr)
    assert (r["e"] == 0).all() and not r["salient"].any() and R.decided(r).all()
    for name in ("collinear", "regular_grid_midpoints"):
        c, r = IC.reference(name, mvr)
        assert not R.decided(r).all()                                     # rank-deficient scatters: e3 is rounding, nothing to compare but the counts
    c, r = IC.reference("huge_coordinates", mvr)
    assert r["salient"].sum() > 1000 and R.decided(r).all()


@pytest.mark.parametrize("name", IC.WALK)
def test_what_the_reference_decides_on_the_walk_cases(name, mvr):
    """a record, and two conditions the GPU test leans on: every point is decided (iss_ref.decided) except on the two sets named
    below, and the patches, the lattice and the clusters have keypoints to suppress"""
    c, r = IC.reference(name, mvr)
    m = R.margins(r)
    und = int((~R.decided(r)).sum())
    print("%s: %d points, radii %.4g / %.4g, %d salient, %d keypoints, %.1f / %.1f neighbours, %d undecided, %d ties, closest ratio %.2e, "
          "closest pair %.2e" % (name, len(c["p"]), c["salient_radius"], c["non_max_radius"], r["salient"].sum(), r["keypoint"].sum(),
                                 r["salient_count"].mean(), r["nms_count"].mean(), und, m["ties"], m["ratio"], m["pair"]))
    assert not c["exact"]
    if name == "planar_sheet":
        assert und == len(c["p"])                                          # rank-deficient: e3 is rounding, the counts and the suppression remain
    else:
        assert und == 0
    assert not (~R.decided(r) & r["salient"]).any()                        # what the GPU's saliency is held to is decided
    if name == "every_target_duplicated":
        assert r["salient_count"].min() >= 7 and m["ties"] > 1000          # no ball of three distinct points twice; twins tie
    if name.startswith("patch_"):
        assert 50 <= r["keypoint"].sum() <= 80
    if name in IC.WALK_RADII_MM:
        assert 4 <= r["keypoint"].sum() <= 16
    if name == "lattice_3d":
        assert m["ties"] > 1000                                            # equal saliencies by symmetry: K5 is strict, both stay
    if name == "patch_far_1e6":
        assert m["ties"] > 0


# ------------------------------------------------------------------ the C-ABI

def test_library_exports_mvr_cloud_iss_keypoints(mvr):
    assert "mvr_cloud_iss_keypoints" in mvr.SIGNATURES
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    assert re.search(r" T mvr_cloud_iss_keypoints$", r.stdout, re.M)
    assert C.sizeof(mvr.IssParams) == 40                                # four doubles, two ints: the header's layout
    assert [f[0] for f in mvr.IssParams._fields_] == ["salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors", "fma_dist"]
    assert hasattr(mvr.Context, "iss_keypoints")


def test_iss_rejects_bad_arguments_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                                  # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    n_out = C.c_size_t(9)
    idx, sc, nc = (C.c_uint32 * 1)(9), (C.c_uint32 * 1)(9), (C.c_uint32 * 1)(9)
    sal = (C.c_double * 1)(9.0)
    f = L.mvr_cloud_iss_keypoints
    good = (4.0, 2.5, 0.975, 0.975, 5, 0)

    def call(c, dst, src, p):
        return f(c, dst, src, C.byref(mvr.IssParams(*p)) if p is not None else None, C.byref(n_out), idx, sal, sc, nc)

    assert call(None, 1, 0, good) == mvr.E_ARG
    assert call(ctx, 1, 0, None) == mvr.E_ARG
    for s in (-1, mvr.MAX_SLOTS, 1 << 20):
        assert call(ctx, 1, s, good) == mvr.E_ARG
    for d in (-2, mvr.MAX_SLOTS, 1 << 20):
        assert call(ctx, d, 0, good) == mvr.E_ARG
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(ctx, 1, 0, (bad,) + good[1:]) == mvr.E_ARG
        assert call(ctx, -1, 0, good[:1] + (bad,) + good[2:]) == mvr.E_ARG
    for bad in (math.nan, math.inf, -math.inf):
        assert call(ctx, 1, 0, good[:2] + (bad,) + good[3:]) == mvr.E_ARG
        assert call(ctx, 1, 0, good[:3] + (bad,) + good[4:]) == mvr.E_ARG
    assert call(ctx, 1, 0, good[:4] + (-1, 0)) == mvr.E_ARG
    assert n_out.value == 9 and idx[0] == 9 and sc[0] == 9 and nc[0] == 9 and sal[0] == 9.0
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the kernels' resources

def test_iss_kernels_use_no_scratch(built, tmp_path):
    assert "mvr_iss.hip" in built.HIP_SOURCES
    src = os.path.join(ROOT, PKG, "csrc", "mvr_iss.hip")
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "mvr_iss.o"),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    use = [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
            int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
           for b in blocks]
    print([(re.sub(r"^_ZN3mvr12_GLOBAL__N_1\d+", "", n), v, s, l) for n, v, s, l in use])
    assert len(use) == 4, use                                            # saliency x fma, non-maximum suppression x fma
    assert sum("iss_saliency_kernel" in n for n, _, _, _ in use) == 2 and sum("iss_nms_kernel" in n for n, _, _, _ in use) == 2
    assert all(s == 0 and l == 0 for _, _, s, l in use), use
    assert all(v <= 64 for _, v, _, _ in use)                            # eight waves per SIMD
