"""GPU tests of the boundary estimation (mvr_cloud_boundary; rules B1-B7 in include/mvr_hip.h) and of the ISS keypoints with a
border (mvr_cloud_iss_keypoints_border; K9-K11) against the numpy reference of tests/boundary_ref.py on the inputs of
tests/boundary_cases.py and tests/iss_cases.py.

Two correct implementations differ by the rounding of the projections and of the arctangent, so a flag is compared wherever the
reference is DECIDED (boundary_ref: the largest gap is further from the threshold than twice the slack of its angles;
tests/test_boundary_host.py shows that at most 0.5 % of an exact case is not).  The neighbour counts are exact everywhere.
max_gap is within that slack of the reference's largest gap wherever the rule promises it: where the reference's gap exceeds a
sector width by more than the slack (a gap within the slack OF the sector width may fall below it on the GPU, where max_gap
promises nothing).  The constructed cases carry their answers with them.  Nothing of the detector with a border is a
tolerance: the edge flags are the boundary call's, the border flags are K10 recomputed on the host from the GPU's own edge
flags, and saliency, counts and keypoints are checked as tests/test_gpu_iss.py checks them, against iss_ref with the GPU's own
border mask applied (K11)."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import boundary_cases as BC
import boundary_ref as R
import fpfh_cases as FC
import iss_cases as IC
import iss_ref as IR
import normals_ref as NR
from conftest import PKG

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
RUNS = [(n, False) for n in BC.NAMES] + [("box", True)]
IDS = ["%s%s" % (n, "-fma" if f else "") for n, f in RUNS]


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def put(ctx, slot, p, nrm):
    ctx.upload(slot, p)
    if len(p):
        ctx.upload_normals(slot, nrm)


def estimate(ctx, slot, c, fma=False):
    flag, gap, cnt = ctx.boundary(slot, c["radius"], c["angle_threshold"], c["min_neighbors"], fma=fma, return_gap=True, return_counts=True)
    assert flag.shape == gap.shape == cnt.shape == (len(c["p"]),) and flag.dtype == bool
    return dict(flag=flag, gap=gap, count=cnt)


_gpu = {}


def gpu_run(name, fma, mvr, ctx):
    if (name, fma) not in _gpu:
        c, ref = BC.reference(name, mvr, fma)
        put(ctx, 0, c["p"], c["nrm"])
        g = estimate(ctx, 0, c, fma)
        assert same_bits(ctx.download(0), c["p"])                            # B7: the slot is left as it was
        if len(c["p"]):
            assert same_bits(ctx.download_normals(0), np.ascontiguousarray(c["nrm"], F32))
        _gpu[(name, fma)] = (c, ref, g)
    return _gpu[(name, fma)]


# ------------------------------------------------------------------ against the reference

@pytest.mark.parametrize("name,fma", RUNS, ids=IDS)
def test_flags_equal_the_references_on_every_decided_point(name, fma, mvr, ctx):
    c, ref, g = gpu_run(name, fma, mvr, ctx)
    d = ref["decided"]
    print("%s fma=%d: %d points, %d boundary points on the GPU, %d in the reference, %d undecided, %d flags differ on the undecided"
          % (name, fma, len(d), g["flag"].sum(), ref["boundary"].sum(), (~d).sum(), (g["flag"] != ref["boundary"])[~d].sum()))
    assert np.array_equal(g["flag"][d], ref["boundary"][d])
    assert not g["flag"][~ref["valid"]].any()


@pytest.mark.parametrize("name,fma", RUNS, ids=IDS)
def test_neighbor_counts_are_exact(name, fma, mvr, ctx):
    c, ref, g = gpu_run(name, fma, mvr, ctx)
    assert np.array_equal(g["count"], ref["neighbor_count"])
    assert (g["count"][~ref["valid"]] == 0).all()


@pytest.mark.parametrize("name,fma", RUNS, ids=IDS)
def test_max_gap_against_the_reference(name, fma, mvr, ctx):
    c, ref, g = gpu_run(name, fma, mvr, ctx)
    wide = ref["max_dif"] > R.SECTOR_WIDTH + ref["slack"]
    err = np.abs(g["gap"].astype(F64) - ref["max_dif"])
    with np.errstate(invalid="ignore", divide="ignore"):
        print("%s fma=%d: %d of %d gaps above a sector width, largest difference %.2e, %.3f of its slack"
              % (name, fma, wide.sum(), len(wide), err[wide].max(initial=0.0), (err / ref["slack"])[wide].max(initial=0.0)))
    assert (err[wide] <= ref["slack"][wide]).all()
    assert (bits(g["gap"][~ref["taken"]]) == 0).all()                     # no angle (an invalid point, B2's deviation, only copies): +0.0
    assert np.isfinite(g["gap"]).all() and (g["gap"] <= np.float32(2 * np.pi) + np.float32(1e-6)).all()
    # B5 on the GPU's own gap
    live = ref["taken"] & (ref["neighbor_count"] >= 3) & (ref["neighbor_count"] >= c["min_neighbors"])
    assert np.array_equal(g["flag"], live & (g["gap"] > np.float32(c["angle_threshold"])))


@pytest.mark.parametrize("name", ["box", "patch_far_1e6"])
def test_results_do_not_depend_on_the_grid_resolution(name, mvr, ctx):
    """minima and maxima do not depend on the walk order: the same bits at every cell edge"""
    c, ref, base = gpu_run(name, False, mvr, ctx)
    try:
        for cp in (1, 64, 4096):
            ctx.tune(seq_cell_points=cp)
            put(ctx, 8, c["p"], c["nrm"])
            g = estimate(ctx, 8, c)
            assert all(same_bits(g[k], base[k]) for k in ("flag", "gap", "count")), (name, cp)
    finally:
        ctx.tune(seq_cell_points=4)


def test_two_runs_give_the_same_bits(mvr, ctx):
    for name, fma in (("view_3", False), ("box", True), ("duplicates", False)):
        c, ref, g = gpu_run(name, fma, mvr, ctx)
        put(ctx, 4, c["p"], c["nrm"])
        h = estimate(ctx, 4, c, fma)
        assert all(same_bits(h[k], g[k]) for k in ("flag", "gap", "count"))


def test_exact_copies_get_the_same_answer(mvr, ctx):
    c, ref, g = gpu_run("duplicates", False, mvr, ctx)
    p, nrm = c["p"], c["nrm"]
    a, b = np.arange(3, len(p), 5)[:len(p[4::5])], np.arange(4, len(p), 5)
    twins = (p[a, :3] == p[b, :3]).all(1)
    assert twins.sum() >= 280
    assert np.array_equal(g["count"][a[twins]], g["count"][b[twins]])      # (their normals differ: the gaps need not agree)
    # the same normal on both: the same bits
    m = nrm.copy()
    m[b] = m[a]
    put(ctx, 5, p, m)
    h = estimate(ctx, 5, c)
    assert same_bits(h["gap"][a[twins]], h["gap"][b[twins]]) and np.array_equal(h["flag"][a[twins]], h["flag"][b[twins]])


# ------------------------------------------------------------------ the constructed cases

@pytest.mark.parametrize("normal", sorted(BC.NORMALS))
def test_constructed_cases(normal, mvr, ctx):
    for name in sorted(BC.CONSTRUCTED):
        deg, copies, kw, want, count = BC.CONSTRUCTED[name]
        kw = dict(kw)
        p, nrm = BC.ring(normal, deg, copies, kw.pop("zero_normal", False))
        put(ctx, 6, p, nrm)
        flag, gap, cnt = ctx.boundary(6, BC.RADIUS, return_gap=True, return_counts=True, **kw)
        assert cnt[0] == count and bool(flag[0]) == want, (name, normal, cnt[0], flag[0], gap[0])
        if name == "three_at_120":
            assert abs(float(gap[0]) - 2 * np.pi / 3) < 1e-3      # (the coordinates are rounded at 900 mm: 3e-5 of the ring radius each)
        if name == "one_neighbour_and_copies":
            assert abs(float(gap[0]) - 2 * np.pi) < 2e-6 and (cnt[:3] == 4).all() and flag[:3].all()      # the copies are the same point
        if name in ("only_copies", "zero_normal"):
            assert bits(gap[:1])[0] == 0
        # the flipped normal gives the same flags
        put(ctx, 7, p, -nrm)
        assert np.array_equal(ctx.boundary(7, BC.RADIUS, **kw), flag), (name, normal)


def test_the_smallest_threshold_and_just_below_it(mvr, ctx):
    p, nrm = BC.ring("z", [10, 130, 250])
    put(ctx, 6, p, nrm)
    assert ctx.boundary(6, BC.RADIUS, angle_threshold=mvr.BOUNDARY_MIN_ANGLE)[0]
    assert ctx.boundary(6, BC.RADIUS, angle_threshold=float(np.nextafter(2 * np.pi, 0)))[0] == False      # noqa: E712 (no gap exceeds it)
    for bad in (float(np.nextafter(mvr.BOUNDARY_MIN_ANGLE, 0)), 0.0, 2 * math.pi, math.nan):
        with pytest.raises(mvr.MvrError):
            ctx.boundary(6, BC.RADIUS, angle_threshold=bad)


# ------------------------------------------------------------------ refusals

def test_refusals_write_nothing(mvr, ctx):
    p, nrm, radius = FC.box(500)
    ctx.upload(5, p)                                                       # a new upload drops the normals
    flag, gap, cnt = np.full(500, 9, np.uint8), np.full(500, 9.0, F32), np.full(500, 9, np.uint32)

    def call(slot, *prm):
        return mvr._lib.mvr_cloud_boundary(ctx._h, slot, C.byref(mvr.BoundaryParams(*prm)), flag.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           gap.ctypes.data_as(C.POINTER(C.c_float)), cnt.ctypes.data_as(C.POINTER(C.c_uint32)))

    assert call(5, radius, math.pi / 2, 0, 0) == mvr.E_ARG                # a slot without normals
    ctx.upload_normals(5, nrm)
    for r in (0.0, -1.0, math.nan, math.inf):
        assert call(5, r, math.pi / 2, 0, 0) == mvr.E_ARG
    for t in (0.0, float(np.nextafter(R.MIN_ANGLE, 0)), 2 * math.pi, math.nan, math.inf):
        assert call(5, radius, t, 0, 0) == mvr.E_ARG
    assert call(5, radius, math.pi / 2, -1, 0) == mvr.E_ARG
    assert call(mvr.MAX_SLOTS, radius, math.pi / 2, 0, 0) == mvr.E_ARG
    assert (flag == 9).all() and (gap == 9.0).all() and (cnt == 9).all()
    prm = mvr.BoundaryParams(radius, math.pi / 2, 0, 0)
    assert mvr._lib.mvr_cloud_boundary(ctx._h, 5, C.byref(prm), None, None, None) == mvr.OK      # all outputs NULL: the work, no copy
    assert call(5, radius, math.pi / 2, 0, 0) == mvr.OK and (flag <= 1).all() and flag.any()
    assert same_bits(p, ctx.download(5)) and same_bits(nrm, ctx.download_normals(5))
    ctx.upload(5, p[:0])
    assert ctx.boundary(5, radius).shape == (0,)                          # an empty cloud is MVR_OK, with or without normals


# ------------------------------------------------------------------ the detector with a border

def iss_border_call(mvr, ctx, dst, src, c, border, fma=False):
    """mvr_cloud_iss_keypoints_border itself; border: None (a NULL pointer) or (border_radius, angle_threshold)"""
    n = ctx.size(src)
    p = mvr.IssParams(c["salient_radius"], c["non_max_radius"], c["gamma_21"], c["gamma_32"], c["min_neighbors"], int(fma))
    idx, sal = np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), F64)
    sc, nc = np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.uint32)
    edge, brd = np.full(max(n, 1), 9, np.uint8), np.full(max(n, 1), 9, np.uint8)
    n_out = C.c_size_t()
    b = mvr.IssBorderParams(*border) if border is not None else None
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    rc = mvr._lib.mvr_cloud_iss_keypoints_border(ctx._h, dst, src, C.byref(p), C.byref(b) if b is not None else None, C.byref(n_out),
                                                 idx.ctypes.data_as(u32), sal.ctypes.data_as(C.POINTER(C.c_double)), sc.ctypes.data_as(u32),
                                                 nc.ctypes.data_as(u32), edge.ctypes.data_as(u8), brd.ctypes.data_as(u8))
    assert rc == mvr.OK, rc
    return dict(index=idx[:n_out.value].copy(), saliency=sal[:n], salient_count=sc[:n], nms_count=nc[:n], edge=edge[:n].astype(bool), border=brd[:n].astype(bool))


KEYS = ("index", "saliency", "salient_count", "nms_count")
# the view of iss_cases with its surface normals at 3 spacings; the box with its random normals at its own radius
ISS_BORDER = {"view": 3.0 * BC.VIEW_SPACING, "box": FC.BOX_RADIUS}


def iss_input(name, mvr):
    c, ref = IC.reference(name, mvr)
    nrm = BC.view(mvr)[1] if name == "view" else FC.box()[1]
    if name == "view":
        assert same_bits(BC.view(mvr)[0], c["p"])
    return c, ref, nrm


@pytest.mark.parametrize("name", sorted(ISS_BORDER))
def test_iss_without_a_border_equals_the_old_entry(name, mvr, ctx):
    c, ref, nrm = iss_input(name, mvr)
    put(ctx, 2, c["p"], nrm)
    n_out, idx, sal, sc, nc = ctx.iss_keypoints(3, 2, return_index=True, return_saliency=True, return_counts=True, **IC.params(c))      # mvr_cloud_iss_keypoints
    old = dict(index=idx, saliency=sal.copy(), salient_count=sc.copy(), nms_count=nc.copy())
    pts, nr = ctx.download(3), ctx.download_normals(3)
    assert len(idx) > 100
    for border in (None, (0.0, math.pi / 2), (0.0, math.nan)):             # NULL; radius 0 (the threshold is then not looked at)
        g = iss_border_call(mvr, ctx, 4, 2, c, border)
        assert all(same_bits(g[k], old[k]) for k in KEYS), border
        assert not g["edge"].any() and not g["border"].any()
        assert same_bits(ctx.download(4), pts) and same_bits(ctx.download_normals(4), nr)
    out = ctx.iss_keypoints(-1, 2, return_index=True, return_edges=True, border_radius=0.0, **IC.params(c))
    assert len(out) == 4 and same_bits(out[1], idx) and not out[2].any() and not out[3].any()


@pytest.mark.parametrize("name", sorted(ISS_BORDER))
def test_iss_with_a_border(name, mvr, ctx):
    c, ref, nrm = iss_input(name, mvr)
    p, n, rb, thr = c["p"], len(c["p"]), ISS_BORDER[name], math.pi / 2
    put(ctx, 2, p, nrm)
    plain = iss_border_call(mvr, ctx, -1, 2, c, None)
    n_out, idx, sal, sc, nc, edge, border = ctx.iss_keypoints(3, 2, return_index=True, return_saliency=True, return_counts=True, return_edges=True,
                                                              border_radius=rb, angle_threshold=thr, **IC.params(c))
    assert n_out == len(idx) and edge.dtype == border.dtype == bool and edge.shape == border.shape == (n,)
    # K9: the edge flags are the boundary call's, with the detector's min_neighbors
    assert np.array_equal(edge, ctx.boundary(2, rb, thr, min_neighbors=c["min_neighbors"]))
    # K10 from the GPU's own edge flags
    flat, offs = NR.radius_sets(p, rb)
    assert np.array_equal(border, R.border_from_edges(edge, flat, offs, ref["valid"]))
    assert edge.any() and (edge <= border).all() and not border.all()
    # K11: zeros on the border, the detector's own bits elsewhere
    assert (bits(sal[border]) == 0).all() and (sc[border] == 0).all() and (nc[border] == 0).all() and not np.isin(idx, np.nonzero(border)[0]).any()
    assert same_bits(sal[~border], plain["saliency"][~border]) and np.array_equal(sc[~border], plain["salient_count"][~border])
    # saliency, counts and keypoints against iss_ref with the GPU's own border mask, as tests/test_gpu_iss.py checks them
    want = R.iss_with_border(ref, border)
    d = R.decided_with_border(ref, border)
    assert np.array_equal(sc, want["salient_count"])
    s = want["salient"]
    rel = np.abs(sal[s] - want["saliency"][s]) / want["saliency"][s]
    assert rel.max(initial=0.0) <= IR.GAP / 4 and (bits(sal[d & ~s]) == 0).all()
    cnt, key = IR.nms(sal, ref["sets"][1][0], ref["sets"][1][1], c["min_neighbors"])
    assert np.array_equal(idx, np.nonzero(key)[0].astype(np.uint32)) and np.array_equal(nc, cnt)
    assert np.array_equal(nc[d], want["nms_count"][d])
    if c["exact"]:
        assert np.array_equal(sal != 0, want["salient"]) and np.array_equal(idx, want["index"])
    out = p[idx.astype(np.int64)].copy()
    out[:, 3] = 1.0
    assert same_bits(ctx.download(3), out) and same_bits(ctx.download_normals(3), np.ascontiguousarray(nrm[idx.astype(np.int64)], F32))
    assert same_bits(ctx.download(2), p)
    lost = np.setdiff1d(plain["index"], idx)
    print("%s: border radius %.2f: %d edge points, %d border points of %d; %d keypoints without a border, %d with, %d lost, %d new"
          % (name, rb, edge.sum(), border.sum(), n, len(plain["index"]), len(idx), len(lost), len(np.setdiff1d(idx, plain["index"]))))
    assert len(lost) >= 1 and border[lost].all()                           # what is lost is lost to the border alone
    # two runs, and no output slot
    h = iss_border_call(mvr, ctx, -1, 2, c, (rb, thr))
    assert same_bits(h["index"], idx) and same_bits(h["saliency"], sal) and np.array_equal(h["edge"], edge) and np.array_equal(h["border"], border)


def test_iss_border_refusals(mvr, ctx):
    c, ref, nrm = iss_input("box", mvr)
    ctx.upload(2, c["p"])                                                  # no normals
    with pytest.raises(mvr.MvrError):
        ctx.iss_keypoints(-1, 2, border_radius=3.0, **IC.params(c))
    assert ctx.iss_keypoints(-1, 2, **IC.params(c)) > 100                  # without a border no normals are needed
    ctx.upload_normals(2, nrm)
    for kw in (dict(border_radius=-1.0), dict(border_radius=math.inf), dict(border_radius=3.0, angle_threshold=0.1),
               dict(border_radius=3.0, angle_threshold=2 * math.pi)):
        with pytest.raises(mvr.MvrError):
            ctx.iss_keypoints(-1, 2, **kw, **IC.params(c))
    ctx.upload(2, c["p"][:0])
    assert ctx.iss_keypoints(3, 2, border_radius=3.0, **IC.params(c)) == 0 and ctx.size(3) == 0      # an empty cloud: MVR_OK
