"""CPU tests of the FPFH descriptors that need no device: the numpy reference (tests/fpfh_ref.py) checked against itself, the
condition on the shared inputs (tests/fpfh_cases.py) that at most 0.30 of the queries have a slack pair, the exported symbol and
its argument refusals, and the resources of the kernels of csrc/mvr_fpfh.hip (no scratch memory).

Measured here: share of queries with a slack pair 0.221 on the view (44.7 neighbours, 894 168 pairs, 5 192 of them slack) and
0.192 on the box (37.1 neighbours); the box fills all 33 bins, the view 28.  On the targets of the walk cases (fpfh_cases.WALK,
random unit normals): the patches 0.111 / 0.105 / 0.111 at 0 / 1e5 / 1e6 mm (20 neighbours; 0.066 / 0.066 / 0.071 with the
normals of their surface), lattice_3d 0.080, the two cluster cases 0.149 / 0.155 (29 and 30 neighbours in a ball of 0.5 mm),
duplicates_41 0.102, every_target_duplicated 0.102, planar_sheet 0.079, the sizes 3 to 1 025 between 0.000 and 0.235 (size_1025,
48 neighbours)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fpfh_cases as FC
import fpfh_ref as R
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def box_ref():
    p, nrm, radius = FC.box()
    return p, nrm, radius, R.fpfh(p, nrm, radius)


@pytest.fixture(scope="module")
def view_ref(mvr):
    p = FC.view(mvr)
    nrm = FC.ref_normals(p)
    return p, nrm, FC.VIEW_RADIUS, R.fpfh(p, nrm, FC.VIEW_RADIUS)


# ------------------------------------------------------------------ the reference against itself

def test_brute_force_neighbours_agree_with_the_kd_tree():
    p, nrm, radius = FC.box(700)
    for q, m in ((p, nrm), FC.with_invalid(p, nrm)[:2]):
        a, b = R.spfh_counts(q, m, radius, brute=True), R.spfh_counts(q, m, radius)
        assert np.array_equal(a["I"], b["I"]) and np.array_equal(a["J"], b["J"])
        assert np.array_equal(a["sure"], b["sure"]) and np.array_equal(a["slack"], b["slack"]) and np.array_equal(a["n"], b["n"])
    assert a["n"][~a["valid"]].sum() == 0 and not np.isin(a["J"], np.nonzero(~a["valid"])[0]).any()


@pytest.mark.parametrize("case", ["box", "view"])
def test_blocks_sum_to_100_and_counts_add_up(case, box_ref, view_ref):
    p, nrm, radius, (f, s, c) = box_ref if case == "box" else view_ref
    n_i = c["n"]
    pairs = c["full"].sum(2)                                            # pairs with features, per feature
    assert (pairs <= np.maximum(n_i - 1, 0)[:, None]).all() and (c["sure"].sum(2) + c["slack"][:, None] >= pairs).all()
    assert np.array_equal(R.counts_from_spfh(s, n_i), c["full"])       # F5 is invertible: the counts come back exactly
    live = c["valid"] & (pairs.min(1) > 0)
    assert live.mean() > 0.99
    assert np.abs(f[live].reshape(-1, 3, R.BINS).astype(F64).sum(2) - 100.0).max() < 1e-3
    assert np.isnan(f[~c["valid"]]).all() and np.isnan(s[~c["valid"]]).all()
    alone = c["valid"] & (n_i == 1)
    assert (f[alone] == 0).all() and (s[alone] == 0).all()


@pytest.mark.parametrize("case", ["box", "view"])
def test_share_of_queries_with_a_slack_pair(case, box_ref, view_ref):
    """a condition on the inputs: where it fails the input changes, not the cap"""
    p, nrm, radius, (f, s, c) = box_ref if case == "box" else view_ref
    share = float((c["slack"] > 0).mean())
    filled = int((c["full"].sum(0) > 0).sum())
    print("%s: %.1f neighbours, %d pairs, %d slack; share of queries with a slack pair %.3f; %d of 33 bins filled"
          % (case, c["n"].mean(), len(c["I"]), int(c["slack"].sum()), share, filled))
    assert share <= FC.SLACK_CAP
    assert 20 <= c["n"].mean() <= 80
    if case == "box":
        assert filled == 33
        o = c["I"] != c["J"]
        F = R.pair_features(p, nrm, c["I"][o], c["J"][o])
        a = np.abs((nrm[c["I"][o], :3].astype(F64) * (p[c["J"][o], :3].astype(F64) - p[c["I"][o], :3].astype(F64))).sum(1))
        b = np.abs((nrm[c["J"][o], :3].astype(F64) * (p[c["J"][o], :3].astype(F64) - p[c["I"][o], :3].astype(F64))).sum(1))
        assert 0.4 < (a < b).mean() < 0.6                                # the swap branch about half the time
        assert F["has_f64"].all()


@pytest.mark.parametrize("name", FC.WALK + FC.WALK_SURFACE)
def test_share_of_queries_with_a_slack_pair_on_the_walk_cases(name, mvr):
    """the same condition on the targets of the walk cases: far frames, a lattice, clusters with thousands of points in a cell,
    duplicates, an exact plane and the sizes around every launch edge"""
    p, nrm, radius = FC.walk(name, mvr)
    if nrm is None:
        nrm = FC.ref_normals(p, FC.walk_normal_radius(p))
    c = R.spfh_counts(p, nrm, radius)
    share = float((c["slack"] > 0).mean())
    print("%s: %d points, %d invalid, radius %.4g, %.1f neighbours, %d pairs, %d slack; share of queries with a slack pair %.3f"
          % (name, len(p), int((~c["valid"]).sum()), radius, c["n"].mean(), len(c["I"]), int(c["slack"].sum()), share))
    assert share <= FC.SLACK_CAP
    assert c["valid"].mean() > 0.9
    if len(p) >= 63:
        assert c["n"].mean() > 2.0                                       # the radius reaches neighbours: there is something to compare


def test_small_and_duplicate_clouds():
    for n in FC.TINY_SIZES:
        p, nrm, radius = FC.tiny(n)
        f, s, c = R.fpfh(p, nrm, radius)
        assert f.shape == (n, 33) and (c["n"] == 1).all() and (f == 0).all() and (s == 0).all()
    p, nrm, radius = FC.duplicates()
    f, s, c = R.fpfh(p, nrm, radius)
    d0 = (p[c["I"], :3] == p[c["J"], :3]).all(1) & (c["I"] != c["J"])
    assert d0.sum() >= 600                                               # coincident pairs: counted in n_i, no features, no weight
    assert (c["full"].sum(2) <= (c["n"] - 1)[:, None]).all() and (c["full"].sum(2)[p[:, 0] == p[0, 0]] < (c["n"] - 1)[p[:, 0] == p[0, 0], None]).all()
    assert np.isfinite(f).all()


# ------------------------------------------------------------------ the C-ABI

def test_library_exports_mvr_cloud_fpfh(mvr):
    assert "mvr_cloud_fpfh" in mvr.SIGNATURES and mvr.FPFH_BINS == 11
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    assert re.search(r" T mvr_cloud_fpfh$", r.stdout, re.M)
    assert C.sizeof(mvr.FpfhParams) == 16                              # double, int: the header's layout
    hdr = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    assert re.search(r"#define MVR_FPFH_BINS 11\b", hdr)
    assert hasattr(mvr.Context, "fpfh")


def test_fpfh_rejects_bad_arguments_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                                  # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    out, sp = (C.c_float * 33)(*[9.0] * 33), (C.c_float * 33)(*[9.0] * 33)
    cnt = (C.c_uint32 * 1)(9)
    f = L.mvr_cloud_fpfh
    assert f(None, 0, C.byref(mvr.FpfhParams(2.5, 0)), out, sp, cnt) == mvr.E_ARG
    assert f(ctx, 0, None, out, sp, cnt) == mvr.E_ARG
    for s in (-1, mvr.MAX_SLOTS, 1 << 20):
        assert f(ctx, s, C.byref(mvr.FpfhParams(2.5, 0)), out, sp, cnt) == mvr.E_ARG
    for r in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert f(ctx, 0, C.byref(mvr.FpfhParams(r, 0)), out, sp, cnt) == mvr.E_ARG
        assert f(ctx, 0, C.byref(mvr.FpfhParams(r, 1)), None, None, None) == mvr.E_ARG
    assert list(out) == [9.0] * 33 and list(sp) == [9.0] * 33 and cnt[0] == 9
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the kernels' resources

def _usage(built, tmp_path, name):
    """[(kernel, VGPRs, scratch bytes per lane, LDS bytes per block)] from the compiler's remarks for one source file"""
    src = os.path.join(ROOT, PKG, "csrc", name)
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / (name + ".o")),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    return [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
             int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
            for b in blocks]


def test_fpfh_kernels_use_no_scratch(built, tmp_path):
    assert "mvr_fpfh.hip" in built.HIP_SOURCES
    use = _usage(built, tmp_path, "mvr_fpfh.hip")
    print([(re.sub(r"^_ZN3mvr12_GLOBAL__N_1\d+", "", n), v, s, l) for n, v, s, l in use])
    assert len(use) == 6, use                                            # normals, SPFH x fma, weighting x fma, rows
    assert all(s == 0 for _, _, s, _ in use), [(n, s) for n, _, s, _ in use if s]
    spfh = [u for u in use if "fpfh_spfh_kernel" in u[0]]
    assert len(spfh) == 2 and all(l == 33 * 256 * 4 for _, _, _, l in spfh)      # hist[bin][thread]: four blocks per CU
    assert all(l == 0 for n, _, _, l in use if "fpfh_spfh_kernel" not in n)
    assert all(v <= 128 for _, v, _, _ in use)                           # four waves per SIMD at least
