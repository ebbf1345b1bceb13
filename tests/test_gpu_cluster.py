"""GPU tests of the Euclidean cluster extraction (mvr_cloud_euclidean_clusters, csrc/mvr_cluster.hip; rules E1-E8 in
include/mvr_hip.h) against tests/cluster_ref.py on the cases of tests/cluster_cases.py.  The clustering is integer
combinatorics over a link predicate whose arithmetic numpy reproduces operation by operation, so every comparison is EXACT:
the result struct, the offsets, the member lists and the labels equal the reference's; dst_slot's points and normals are the
bits of the gathered source."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import cluster_cases as CC
import cluster_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

F32 = np.float32
FIELDS = ("n_active", "n_components", "n_clusters", "n_clustered", "largest", "too_small", "too_large")


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def load(ctx, slot, case):
    ctx.upload(slot, case.pts)
    if case.normals is not None and len(case.pts):
        ctx.upload_normals(slot, case.normals)


def run(ctx, case, dst=-1, src=0, fma=False, **more):
    kw = dict(case.kw, **more)
    return ctx.euclidean_clusters(dst, src, case.tolerance, fma=fma, return_lists=True, return_labels=True, **kw)


def check(got, ref, what):
    res, lists, labels = got
    assert {k: res[k] for k in FIELDS} == ref["result"], (what, res, ref["result"])
    assert len(lists) == len(ref["lists"]) and all(np.array_equal(a, b) for a, b in zip(lists, ref["lists"])), what
    assert np.array_equal(labels, ref["labels"]), what


@pytest.mark.parametrize("name", CC.names())
def test_every_case_equals_the_reference(ctx, mvr, name):
    """result struct, lists (hence offsets) and labels, fma off and on, with no output slot: the source keeps its bits"""
    case = CC.cases(mvr)[name]
    load(ctx, 0, case)
    for fma in (False, True):
        got = run(ctx, case, fma=fma)
        check(got, CC.reference(case, fma), (name, fma))
        assert got[0]["n_out"] == 0
    assert ctx.size(0) == len(case.pts)
    if len(case.pts):
        assert np.array_equal(bits(ctx.download(0)), bits(case.pts))


def raw_call(mvr, ctx, case, offset_cap, dst=-1, keep=1):
    """the C-ABI itself with an offset array of offset_cap entries, pre-set to 9s behind it"""
    n = len(case.pts)
    p = mvr.ClusterParams(case.tolerance, case.kw.get("min_size", 1), case.kw.get("max_size", 2 ** 31 - 1), 0, 0.0, 0, keep, 0)
    res, n_out = mvr.ClusterResult(), C.c_size_t(77)
    off = np.full(offset_cap + 3, 9, np.uint32)
    cidx = np.full(n + 3, 9, np.uint32)
    rc = mvr._lib.mvr_cloud_euclidean_clusters(ctx._h, dst, 0, C.byref(p), None, 0, C.byref(res), C.byref(n_out),
                                               off.ctypes.data_as(C.POINTER(C.c_uint32)), offset_cap, cidx.ctypes.data_as(C.POINTER(C.c_uint32)), None)
    return rc, res, off, cidx


def test_offsets_are_truncated_at_offset_cap(ctx, mvr):
    case = CC.cases(mvr)["twelve_equal_blobs"]
    ref = CC.reference(case)
    load(ctx, 0, case)
    nc = ref["result"]["n_clusters"]
    assert nc == 12
    for cap in (0, 1, 2, nc, nc + 1, nc + 5):
        rc, res, off, cidx = raw_call(mvr, ctx, case, cap)
        m = min(nc, cap - 1) + 1 if cap else 0
        assert rc == 0 and res.n_clusters == nc and res.n_clustered == 240
        assert np.array_equal(off[:m], ref["offsets"][:m]) and np.all(off[m:] == 9), (cap, off)
        assert np.array_equal(cidx[:240], ref["index"]) and np.all(cidx[240:] == 9)
    empty = CC.cases(mvr)["min_above_max"]                       # no cluster: offset[0] = 0 and nothing else
    load(ctx, 0, empty)
    rc, res, off, cidx = raw_call(mvr, ctx, empty, 4)
    assert rc == 0 and res.n_clusters == 0 and off[0] == 0 and np.all(off[1:] == 9) and np.all(cidx == 9)


@pytest.mark.parametrize("name", ["twelve_equal_blobs", "sheets_with_normals", "non_finite", "subset_of_blobs_negative", "min_above_max"])
def test_dst_slot_gets_the_first_clusters(ctx, mvr, name):
    """in place and into another slot, keep 1, 2 and beyond n_clusters: points and normals are the bits of the gathered source"""
    case = CC.cases(mvr)[name]
    with_normals = case.normals is not None
    for keep in (1, 2, 10 ** 6):
        ref = R.clusters(case.pts, case.tolerance, normals=case.normals, keep=keep, **case.kw)
        for dst in (1, 0):
            load(ctx, 0, case)
            ctx.upload(1, np.ones((5, 4), F32))
            got = run(ctx, case, dst=dst, keep=keep)
            check(got, ref, (name, keep, dst))
            kept = ref["kept"]
            assert got[0]["n_out"] == len(kept) == ctx.size(dst)
            if len(kept):
                assert np.array_equal(bits(ctx.download(dst)), bits(case.pts[kept]))
                if with_normals:
                    assert np.array_equal(bits(ctx.download_normals(dst)), bits(case.normals[kept]))
            if dst == 1:
                assert ctx.size(0) == len(case.pts) and np.array_equal(bits(ctx.download(0)), bits(case.pts))
            elif len(kept) >= 4:                                    # the new point set is searched like any other
                again = ctx.euclidean_clusters(-1, 0, case.tolerance, return_lists=True, return_labels=True)
                check(again, R.clusters(case.pts[kept], case.tolerance), (name, keep, "clustered again"))


def test_two_runs_give_identical_bytes(ctx, mvr):
    for name in ("two_snakes", "walk_patch_at_0_several", "walk_duplicates_41_fraction", "non_finite"):
        case = CC.cases(mvr)[name]
        outs = []
        for _ in range(2):
            load(ctx, 0, case)                                    # a fresh upload: the grid is built again, too
            res, lists, labels = run(ctx, case)
            outs.append((sorted(res.items()), [m.tobytes() for m in lists], labels.tobytes()))
        assert outs[0] == outs[1], name


@pytest.mark.parametrize("name", ["snake", "two_snakes", "walk_patch_far_1e6_several", "walk_lattice_3d_at_step", "walk_clusters_and_a_far_point_several",
                                  "walk_collinear_several", "walk_duplicates_41_fraction", "non_finite", "sheets_with_normals"])
def test_result_does_not_depend_on_the_grid_resolution(ctx, mvr, name):
    """the resolutions tests/test_gpu_walk_fuzz.py sweeps (seq_cell_points 4, 1, 64, 4096; the cloud is uploaded again after
    each tune, a slot keeps its grid until its points change)"""
    case = CC.cases(mvr)[name]
    ref = CC.reference(case)
    try:
        for cp in (4, 1, 64, 4096):
            ctx.tune(seq_cell_points=cp)
            load(ctx, 0, case)
            check(run(ctx, case), ref, (name, cp))
    finally:
        ctx.tune(seq_cell_points=4)


def test_argument_errors_leave_outputs_and_slots_unwritten(ctx, mvr):
    """E8 on a live context: every refusal returns E_ARG, writes no output and touches no slot"""
    L = mvr._lib
    case = CC.cases(mvr)["sheets_with_normals"]
    plain = CC.cases(mvr)["twelve_equal_blobs"]
    load(ctx, 0, case)                                            # slot 0: normals; slot 1: none
    load(ctx, 1, plain)
    ctx.upload(2, np.ones((5, 4), F32))
    res, n_out = mvr.ClusterResult(9, 9, 9, 9, 9, 9, 9), C.c_size_t(9)
    n = len(case.pts)
    off, cidx, lab = np.full(n + 2, 9, np.uint32), np.full(n, 9, np.uint32), np.full(n, 9, np.uint32)
    u32 = C.POINTER(C.c_uint32)
    good = dict(tolerance=0.6, min_size=1, max_size=10 ** 6, use_normals=0, eps_angle=0.0, negative=0, keep=1, fma_dist=0)

    def call(dst, src, index=None, count=None, with_res=True, null=False, **kw):
        a = dict(good, **kw)
        p = None if null else C.byref(mvr.ClusterParams(a["tolerance"], a["min_size"], a["max_size"], a["use_normals"], a["eps_angle"],
                                                        a["negative"], a["keep"], a["fma_dist"]))
        idx = None if index is None else np.ascontiguousarray(index, np.uint32)
        return L.mvr_cloud_euclidean_clusters(ctx._h, dst, src, p, None if idx is None else idx.ctypes.data_as(u32),
                                              (0 if idx is None else len(idx)) if count is None else count, C.byref(res) if with_res else None,
                                              C.byref(n_out), off.ctypes.data_as(u32), len(off), cidx.ctypes.data_as(u32), lab.ctypes.data_as(u32))

    E = mvr.E_ARG
    assert call(2, 0, null=True) == E and call(2, 0, with_res=False) == E
    assert [call(2, s) for s in (-1, mvr.MAX_SLOTS)] == [E, E] and [call(d, 0) for d in (-2, mvr.MAX_SLOTS)] == [E, E]
    assert [call(2, 0, tolerance=t) for t in (0.0, -1.0, math.nan, math.inf)] == [E] * 4
    assert call(2, 0, keep=0) == E and call(-1, 0, keep=0) == 0                       # keep only matters with a dst slot
    assert call(2, 1, use_normals=1, eps_angle=0.5) == E                               # slot 1 has no normals
    assert [call(2, 0, use_normals=1, eps_angle=e) for e in (0.0, -0.5, float(np.nextafter(math.pi, 4.0)), math.nan)] == [E] * 4
    assert call(2, 0, use_normals=1, eps_angle=math.pi) == 0 and ctx.size(2) > 0
    ctx.upload(2, np.ones((5, 4), F32))
    res, n_out = mvr.ClusterResult(9, 9, 9, 9, 9, 9, 9), C.c_size_t(9)
    off[:], cidx[:], lab[:] = 9, 9, 9
    assert call(2, 0, index=None, count=3) == E
    assert call(2, 0, index=[0, 1, n]) == E and call(0, 0, index=[n + 5], negative=1) == E
    assert tuple(getattr(res, f) for f in FIELDS) == (9,) * 7 and n_out.value == 9
    assert np.all(off == 9) and np.all(cidx == 9) and np.all(lab == 9)
    assert ctx.size(2) == 5 and np.array_equal(bits(ctx.download(0)), bits(case.pts)) and np.array_equal(bits(ctx.download_normals(0)), bits(case.normals))
    with pytest.raises(mvr.MvrError):
        ctx.euclidean_clusters(-1, 0, 0.0)
    # an empty cloud is MVR_OK with zeros
    ctx.upload(3, np.zeros((0, 4), F32))
    r = ctx.euclidean_clusters(3, 3, 1.0, keep=2, return_lists=True, return_labels=True)
    assert all(v == 0 for v in r[0].values()) and r[1] == [] and len(r[2]) == 0


# ------------------------------------------------------------------ end to end: plane, then clusters

def scene(mvr):
    """a small synthetic view, a platter under it and two detached blobs beside it"""
    rng = np.random.default_rng(12)
    v = mvr.synth_view(mvr.synth_params(12, 2), 0, 4000)
    P = v[:, :3].astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    ext = float((hi - lo).max())
    g = np.linspace(-0.7, 0.7, 45)
    plat = np.stack(np.meshgrid(g * ext, g * ext, [0.0], indexing="ij"), -1).reshape(-1, 3) + [(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, lo[2] - 0.2 * ext]
    blob = [rng.standard_normal((m, 3)) * 0.01 * ext + [hi[0] + 0.5 * ext, lo[1] + k * 0.5 * ext, (lo[2] + hi[2]) / 2] for k, m in enumerate((150, 60))]
    xyz = np.concatenate([P, plat, blob[0], blob[1]])
    pts = np.ones((len(xyz), 4), F32)
    pts[:, :3] = xyz[rng.permutation(len(xyz))]
    return pts, ext


def test_plane_then_clusters_end_to_end(ctx, mvr):
    pts, ext = scene(mvr)
    threshold, tol = 0.002 * ext, 0.05 * ext
    ctx.upload(0, pts)
    res, inliers = ctx.segment_plane(-1, 0, threshold, max_iterations=200, seed=5, return_index=True)
    assert res["found"] and 1900 <= len(inliers) <= 2300                                  # the platter (45 x 45), give or take the object's foot
    direct = ctx.euclidean_clusters(-1, 0, tol, min_size=30, index=inliers, negative=True, return_lists=True, return_labels=True)
    ref = R.clusters(pts, tol, min_size=30, index=inliers, negative=True)
    check(direct, ref, "index = the plane's inliers, negative")
    assert direct[0]["n_clusters"] >= 3 and direct[0]["largest"] > 150
    # the same through the extracted cloud, indices mapped back
    rest = np.setdiff1d(np.arange(len(pts)), inliers)
    assert ctx.extract_indices(1, 0, inliers, negative=True) == len(rest)
    sub = ctx.euclidean_clusters(1, 1, tol, min_size=30, return_lists=True, return_labels=True)
    assert {k: sub[0][k] for k in FIELDS} == ref["result"]
    assert all(np.array_equal(rest[a], b) for a, b in zip(sub[1], ref["lists"])) and len(sub[1]) == len(ref["lists"])
    assert np.array_equal(sub[2], ref["labels"][rest])
    assert sub[0]["n_out"] == ref["result"]["largest"] and np.array_equal(bits(ctx.download(1)), bits(pts[ref["lists"][0]]))
