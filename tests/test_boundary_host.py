"""CPU tests of the boundary estimation that need no device: the numpy reference (tests/boundary_ref.py) on the shared inputs
(tests/boundary_cases.py) -- the conditions under which the GPU test compares flags --, the reference against the answers of the
constructed cases and against a second implementation (the kernel's sector scheme restated in f32), the declarations and the
exported symbols, the argument refusals, and the resources of the kernels of csrc/mvr_boundary.hip.

Measured here on the reference (edge points / points with one in reach / undecided): view at 3 spacings 6.7 % / 43.9 % / 0 of
20 000, at 4 spacings 2.5 % / 11.6 % / 0; box 14.4 % / 69.0 % / 0 of 3 000; the view with invalid points 4.7 % / 21.8 % / 0 of
6 000; duplicates 31.0 % / 91.5 % / 0 of 1 500; the far-frame patches 5.4 % / 30.7 % at 1e5 mm and 5.3 % / 30.6 % at 1e6 mm,
0 of 6 000 undecided.  The sector scheme in f32 gives the reference's flag on every decided point and its largest gap within
0.15 of the slack wherever that gap is above a sector width."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import boundary_cases as BC
import boundary_ref as R
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ the conditions of the comparison

@pytest.mark.parametrize("name", BC.EXACT)
def test_undecided_share_and_both_outcomes(name, mvr):
    c, r = BC.reference(name, mvr)
    n = len(c["p"])
    und = int((~r["decided"]).sum())
    border = R.border_from_edges(r["boundary"], *r["sets"], r["valid"])
    print("%s: %d points, radius %.3f, %.1f neighbours, %d boundary points, %d with one in reach, %d undecided"
          % (name, n, c["radius"], r["neighbor_count"].mean(), r["boundary"].sum(), border.sum(), und))
    assert und <= BC.UNDECIDED_CAP * n
    live = r["valid"] & r["decided"]
    assert (r["boundary"] & live).sum() >= 20 and (~r["boundary"] & live & (r["neighbor_count"] >= 3)).sum() >= 20
    assert (r["boundary"] <= border).all() and not border[~r["valid"]].any()


def test_the_invalid_points_are_there(mvr):
    c, r = BC.reference("view_invalid", mvr)
    bad_p = ~np.isfinite(c["p"][:, :3]).all(1)
    bad_n = ~np.isfinite(c["nrm"][:, :3]).all(1) & ~bad_p
    assert bad_p.sum() >= 10 and bad_n.sum() >= 10
    assert (r["neighbor_count"][bad_p] == 0).all() and (r["neighbor_count"][bad_n] > 0).all()      # B1: the count does not look at the normal
    assert not r["boundary"][bad_p | bad_n].any() and (r["max_dif"][bad_p | bad_n] == 0).all()     # B2's deviation
    assert r["decided"][bad_p | bad_n].all()
    # an invalid point is nobody's neighbour
    assert not np.isin(r["sets"][0], np.nonzero(bad_p)[0]).any()


@pytest.mark.parametrize("name", BC.TINY)
def test_tiny_clouds_have_no_boundary(name, mvr):
    c, r = BC.reference(name, mvr)
    assert len(r["boundary"]) == int(name[5:]) and not r["boundary"].any() and (r["neighbor_count"] == (1 if len(c["p"]) else 0)).all()


# ------------------------------------------------------------------ the reference against known answers and a second implementation

@pytest.mark.parametrize("normal", sorted(BC.NORMALS))
@pytest.mark.parametrize("name", sorted(BC.CONSTRUCTED))
def test_reference_on_the_constructed_cases(name, normal):
    deg, copies, kw, want, count = BC.CONSTRUCTED[name]
    kw = dict(kw)
    p, nrm = BC.ring(normal, deg, copies, kw.pop("zero_normal", False))
    r = R.boundary(p, nrm, BC.RADIUS, **kw)
    assert r["neighbor_count"][0] == count and bool(r["boundary"][0]) == want and r["decided"][0]


def test_basis_is_orthogonal_and_first_largest():
    rng = np.random.default_rng(3)
    n = rng.standard_normal((500, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = np.concatenate([n, [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [-1, 1, 1]] / np.sqrt([[1], [1], [1], [2], [2], [2], [3]])])
    u, v, ok = R.basis(n.astype(F32))
    assert ok.all()
    n, u, v = n.astype(F32).astype(F64), u.astype(F64), v.astype(F64)
    assert np.abs((u * v).sum(1)).max() < 1e-6 and np.abs((u * n).sum(1)).max() < 1e-6 and np.abs((v * n).sum(1)).max() < 1e-6
    assert np.abs(np.linalg.norm(u, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(v, axis=1) - 1).max() < 1e-6
    # |n_x| == |n_y|: the first index wins, so v has no z component and v.x = -n.y * inv
    i = len(n) - 4
    assert v[i, 2] == 0 and v[i, 0] < 0 < v[i, 1]
    # the deviation: a zero normal and a non-finite one
    _, _, ok = R.basis(np.array([[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [0, 0, 2]], F32))
    assert ok.tolist() == [False, False, False, True]


def sector_scheme(c, r):
    """the kernel's scheme (csrc/mvr_boundary.hip) restated: f32 projections and angles, the smallest and the largest angle of 16
    sectors, the gaps between occupied sectors and the wrap-around: (flags, max_gap)"""
    p, n = c["p"], len(c["p"])
    flat, offs = r["sets"]
    cnt = np.diff(offs)
    u, v, ok = R.basis(c["nrm"])
    owner = np.repeat(np.arange(n), cnt)
    with np.errstate(all="ignore"):
        d = p[flat, :3] - p[owner, :3]
    take = (d != 0).any(1) & ok[owner]
    o, d = owner[take], d[take]
    y = (v[o, 0] * d[:, 0] + v[o, 1] * d[:, 1]) + v[o, 2] * d[:, 2]
    x = (u[o, 0] * d[:, 0] + u[o, 1] * d[:, 1]) + u[o, 2] * d[:, 2]
    a = np.arctan2(y, x).astype(F32)
    assert x.dtype == F32 and a.dtype == F32
    s = np.clip(np.floor((a + F32(np.pi)) * F32(R.SECTORS / (2 * np.pi))), 0, R.SECTORS - 1).astype(np.int64)
    lo, hi = np.full(n * R.SECTORS, np.inf, F32), np.full(n * R.SECTORS, -np.inf, F32)
    np.minimum.at(lo, o * R.SECTORS + s, a)
    np.maximum.at(hi, o * R.SECTORS + s, a)
    lo, hi = lo.reshape(n, R.SECTORS), hi.reshape(n, R.SECTORS)
    gap, seen = np.full(n, np.finfo(F32).tiny, F32), np.zeros(n, bool)
    first, last = np.zeros(n, F32), np.zeros(n, F32)
    for k in range(R.SECTORS):
        occ = lo[:, k] <= hi[:, k]
        gap = np.where(occ & seen, np.maximum(gap, lo[:, k] - last), gap)
        first = np.where(occ & ~seen, lo[:, k], first)
        last = np.where(occ, hi[:, k], last)
        seen |= occ
    gap = np.where(seen, np.maximum(gap, (F32(2) * F32(np.pi) - last) + first), gap)
    assert gap.dtype == F32
    flag = seen & (cnt >= 3) & (cnt >= c["min_neighbors"]) & (gap > F32(c["angle_threshold"]))
    return flag, np.where(seen, gap, F32(0))


@pytest.mark.parametrize("name", BC.EXACT)
def test_the_sector_scheme_decides_as_the_sort(name, mvr):
    c, r = BC.reference(name, mvr)
    flag, gap = sector_scheme(c, r)
    d = r["decided"]
    assert np.array_equal(flag[d], r["boundary"][d])
    wide = r["max_dif"] > R.SECTOR_WIDTH + r["slack"]
    assert wide.sum() > 1000 and (np.abs(gap.astype(F64) - r["max_dif"])[wide] <= r["slack"][wide]).all()
    assert (gap[~r["taken"]] == 0).all()


def test_border_and_detector_from_any_edge_array(mvr):
    import iss_cases as IC
    c, ref = IC.reference("box", mvr)
    n = len(c["p"])
    rng = np.random.default_rng(9)
    edge = rng.random(n) < 0.02
    flat, offs = ref["sets"][1]
    border = R.border_from_edges(edge, flat, offs, ref["valid"])
    for i in (0, 17, n - 1):
        assert border[i] == edge[flat[offs[i]:offs[i + 1]]].any()
    assert edge.sum() < border.sum() < n
    out = R.iss_with_border(ref, border)
    assert (out["saliency"][border] == 0).all() and (out["salient_count"][border] == 0).all() and (out["nms_count"][border] == 0).all()
    assert not out["keypoint"][border].any() and np.array_equal(out["saliency"][~border], ref["saliency"][~border])
    assert (ref["keypoint"] & ~border <= out["keypoint"]).all()          # a border point never suppresses: no keypoint elsewhere is lost
    none = R.iss_with_border(ref, np.zeros(n, bool))
    assert np.array_equal(none["index"], ref["index"]) and np.array_equal(none["nms_count"], ref["nms_count"])


# ------------------------------------------------------------------ the C-ABI

def test_header_declares_the_two_entries():
    h = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    assert re.search(r"\bint\s+mvr_cloud_boundary\(mvr_ctx \*ctx, int slot, const mvr_boundary_params \*", h)
    assert re.search(r"\bint\s+mvr_cloud_iss_keypoints_border\(mvr_ctx \*ctx, int dst_slot[^;]*const mvr_iss_border_params \*", h)
    assert "} mvr_boundary_params;" in h and "} mvr_iss_border_params;" in h
    m = re.search(r"#define MVR_BOUNDARY_MIN_ANGLE (\S+)", h)
    assert m and float(m.group(1)) == R.MIN_ANGLE and R.MIN_ANGLE <= math.pi / 4 and R.MIN_ANGLE >= 2 * R.SECTOR_WIDTH
    for rule in ["B%d." % k for k in range(1, 8)] + ["K9.", "K10.", "K11."]:
        assert " " + rule + " " in h, rule


def test_library_exports_the_two_entries(mvr):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    for sym in ("mvr_cloud_boundary", "mvr_cloud_iss_keypoints_border", "mvr_cloud_iss_keypoints"):
        assert sym in mvr.SIGNATURES and re.search(r" T %s$" % sym, r.stdout, re.M), sym
    assert C.sizeof(mvr.BoundaryParams) == 24 and C.sizeof(mvr.IssBorderParams) == 16 and C.sizeof(mvr.IssParams) == 40
    assert [f[0] for f in mvr.BoundaryParams._fields_] == ["radius", "angle_threshold", "min_neighbors", "fma_dist"]
    assert [f[0] for f in mvr.IssBorderParams._fields_] == ["border_radius", "angle_threshold"]
    assert mvr.BOUNDARY_MIN_ANGLE == R.MIN_ANGLE and hasattr(mvr.Context, "boundary")


def test_bad_arguments_are_refused_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                                  # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    flag, edge, border = (C.c_uint8 * 1)(9), (C.c_uint8 * 1)(9), (C.c_uint8 * 1)(9)
    gap = (C.c_float * 1)(9.0)
    cnt, idx, sc, nc = (C.c_uint32 * 1)(9), (C.c_uint32 * 1)(9), (C.c_uint32 * 1)(9), (C.c_uint32 * 1)(9)
    sal = (C.c_double * 1)(9.0)
    n_out = C.c_size_t(9)
    good = (3.0, math.pi / 2, 0, 0)

    def call(c, slot, p):
        return L.mvr_cloud_boundary(c, slot, C.byref(mvr.BoundaryParams(*p)) if p is not None else None, flag, gap, cnt)

    assert call(None, 0, good) == mvr.E_ARG and call(ctx, 0, None) == mvr.E_ARG
    for s in (-1, mvr.MAX_SLOTS, 1 << 20):
        assert call(ctx, s, good) == mvr.E_ARG
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(ctx, 0, (bad,) + good[1:]) == mvr.E_ARG
    below, two_pi = float(np.nextafter(R.MIN_ANGLE, 0.0)), 2.0 * math.pi
    for bad in (0.0, -1.0, below, two_pi, 7.0, math.nan, math.inf, -math.inf):
        assert call(ctx, 0, (3.0, bad, 0, 0)) == mvr.E_ARG
    assert call(ctx, 0, (3.0, math.pi / 2, -1, 0)) == mvr.E_ARG

    iss = (4.0, 2.5, 0.975, 0.975, 5, 0)

    def call_iss(c, dst, src, p, b):
        return L.mvr_cloud_iss_keypoints_border(c, dst, src, C.byref(mvr.IssParams(*p)) if p is not None else None,
                                                C.byref(mvr.IssBorderParams(*b)) if b is not None else None, C.byref(n_out), idx, sal, sc, nc, edge, border)

    assert call_iss(None, 1, 0, iss, (3.0, 1.5)) == mvr.E_ARG and call_iss(ctx, 1, 0, None, (3.0, 1.5)) == mvr.E_ARG
    assert call_iss(ctx, 1, -1, iss, None) == mvr.E_ARG and call_iss(ctx, -2, 0, iss, None) == mvr.E_ARG
    assert call_iss(ctx, 1, 0, (0.0,) + iss[1:], None) == mvr.E_ARG and call_iss(ctx, 1, 0, iss[:4] + (-1, 0), (3.0, 1.5)) == mvr.E_ARG
    for bad in (-1.0, math.nan, math.inf):
        assert call_iss(ctx, 1, 0, iss, (bad, 1.5)) == mvr.E_ARG
    for bad in (0.0, below, two_pi, math.nan):
        assert call_iss(ctx, 1, 0, iss, (3.0, bad)) == mvr.E_ARG
    assert flag[0] == 9 and gap[0] == 9.0 and cnt[0] == 9 and edge[0] == 9 and border[0] == 9
    assert n_out.value == 9 and idx[0] == 9 and sc[0] == 9 and nc[0] == 9 and sal[0] == 9.0
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the kernels' resources

def test_boundary_kernels_use_no_scratch(built, tmp_path):
    assert "mvr_boundary.hip" in built.HIP_SOURCES
    src = os.path.join(ROOT, PKG, "csrc", "mvr_boundary.hip")
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "mvr_boundary.o"),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    use = [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
            int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
           for b in blocks]
    print(use)
    assert len(use) == 4, use                                            # boundary x fma, the border instantiation of the ISS saliency x fma
    assert all(s == 0 for _, _, s, _ in use), use
    assert sorted(l for n, _, _, l in use if "boundary_kernel" in n) == [2 * R.SECTORS * 256 * 4] * 2      # [sector][thread], smallest and largest
    assert [l for n, _, _, l in use if "iss_saliency_kernel" in n] == [0, 0]
    assert all(v <= 64 for _, v, _, _ in use)
