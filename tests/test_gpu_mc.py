"""GPU tests of the surface reconstruction (mvr_cloud_marching_cubes_hoppe, rules M1-M15 in include/mvr_hip.h) against the numpy
restatement tests/mc_ref.py: lattice values, soup vertices, triangle count and order BIT FOR BIT -- every operation of M2-M8 is
one rounded f32 operation and the search is mvr_nn's, so there is no tolerance anywhere in this file (mc_ref.same_bits: equal
bits, every NaN the same NaN).  Each case is the smallest at which its mistake shows."""
import ctypes as C

import numpy as np
import pytest

import mc_cases as Cs
import mc_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
VIEW_RES = (17, 9, 33)      # 4 096 cells: sixteen blocks, no multiple of 64 or 256 along any axis


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def put(ctx, slot, pts, nrm):
    ctx.upload(slot, np.ascontiguousarray(pts, F32))
    ctx.upload_normals(slot, np.ascontiguousarray(nrm, F32))


def check(ctx, slot, pts, nrm, res, iso=0.0, pct=0.0, dist_ignore=-1.0, fma=False, weld=False):
    """one call against the reference: the grid, the soup (or the weld) and the count"""
    ref = R.reconstruct(pts, nrm, res, iso, pct, dist_ignore, fma)
    v, t, g = ctx.marching_cubes_hoppe(slot, res, iso, pct, dist_ignore, weld=weld, return_grid=True, fma=fma)
    assert R.same_bits(g, ref["grid"])
    if weld:
        assert R.same_bits(v, ref["vertices"]) and np.array_equal(t.ravel(), ref["indices"])
    else:
        assert len(t) * 3 == len(ref["soup"]) and R.same_bits(v, ref["soup"])
        assert np.array_equal(t.ravel(), np.arange(len(v), dtype=np.uint32))
    return ref, v, t, g


@pytest.fixture(scope="module")
def view(mvr, ctx):
    """the 3 000-point synthetic view with its GPU normals: an open surface, so far sheets and unbounded queries"""
    pts = mvr.synth_view(mvr.synth_params(12, 1), 0, 3000)
    ctx.upload(10, pts)
    ctx.estimate_normals(10, k=12)
    nrm = ctx.download_normals(10)
    return pts[:, :3].copy(), nrm[:, :3].copy()


@pytest.fixture(scope="module")
def view_ref(view):
    return {fma: R.reconstruct(view[0], view[1], VIEW_RES, fma=fma) for fma in (False, True)}


@pytest.fixture(scope="module")
def ball():
    return Cs.sphere()


# ---- a: one cell

def test_one_cell_cases(ctx):
    cases = Cs.one_cell({0, 255, 1, 128, 3, 90, 165, 60, 105})
    for cube, (p, n) in sorted(cases.items()):
        put(ctx, 0, p, n)
        ref, v, t, g = check(ctx, 0, p, n, (2, 2, 2))
        tri = R.tables()[1][cube]
        assert len(t) == int((tri >= 0).sum()) // 3, cube
    assert len(R.reconstruct(*cases[0], (2, 2, 2))["soup"]) == 0 == len(R.reconstruct(*cases[255], (2, 2, 2))["soup"])


# ---- b: index order and corner order

@pytest.mark.parametrize("res", [(2, 3, 5), (5, 3, 2)])
def test_plane_patch_unequal_resolutions(ctx, res):
    p, n = Cs.plane_patch()
    put(ctx, 0, p, n)
    ref, v, t, g = check(ctx, 0, p, n, res)
    assert len(t) > 0 and g.shape == res


# ---- c, j: the view, unbounded, on two grids of the slot, both distances, every route

@pytest.mark.parametrize("fma", [False, True])
def test_view_unbounded_on_two_slot_grids_and_every_route(ctx, view, view_ref, fma):
    pts, nrm = view
    ref = view_ref[fma]
    assert len(ref["soup"]) > 300 and np.isfinite(ref["grid"]).all()
    got = []
    try:
        for cell_points in (4, 32):
            ctx.tune(seq_cell_points=cell_points)
            put(ctx, 1, pts, nrm)                      # a new point set: its grid is built at this resolution
            for route in (0, 1, 2, 3):
                ctx.tune(mc_route=route)
                v, t, g = ctx.marching_cubes_hoppe(1, VIEW_RES, return_grid=True, fma=fma)
                assert ctx.stat("mc_route_used") == (route or 2)
                assert R.same_bits(g, ref["grid"]) and R.same_bits(v, ref["soup"]) and len(t) * 3 == len(ref["soup"]), (cell_points, route)
                got.append(v)
    finally:
        ctx.tune(seq_cell_points=4, mc_route=0)
    v2, _ = ctx.marching_cubes_hoppe(1, VIEW_RES, fma=fma)      # a second run: the same bits (M9)
    assert R.same_bits(v2, got[-1])


def test_view_values_are_those_of_mvr_nn(mvr, ctx, view, view_ref):
    """(j, d2) of rule M5 is what mvr_nn answers for the lattice as a cloud of its own"""
    pts, nrm = view
    ref = view_ref[False]
    lat = R.lattice(ref["lower"], ref["size"], VIEW_RES).reshape(-1, 3)
    ctx.upload(2, np.concatenate([lat, np.ones((len(lat), 1), F32)], 1))
    ctx.upload(1, pts)
    idx, d2 = ctx.nn(2, 1)
    ridx, rd2 = R.nearest(lat, pts)
    assert np.array_equal(idx, ridx) and R.same_bits(d2, rd2) and R.same_bits(d2, ref["d2"].ravel())


# ---- d: dist_ignore

def test_view_dist_ignore_and_its_strict_bound(ctx, view, view_ref):
    pts, nrm = view
    d2 = np.sort(view_ref[False]["d2"].ravel())
    put(ctx, 1, pts, nrm)
    mid = float(d2[len(d2) // 3])
    assert d2[0] < mid < d2[-1]
    for cap in (mid * 1.0000001, float(d2[len(d2) // 2])):      # between two d2, and exactly on one: `d2 < cap` is strict
        for route in (0, 1, 2, 3):
            ctx.tune(mc_route=route)
            try:
                ref, v, t, g = check(ctx, 1, pts, nrm, VIEW_RES, dist_ignore=cap)
                assert ctx.stat("mc_route_used") == (route or 1)
            finally:
                ctx.tune(mc_route=0)
            nan = np.isnan(ref["grid"])
            assert nan.any() and not nan.all() and len(t) > 0
            assert np.array_equal(nan, ~(view_ref[False]["d2"] < F32(cap)))
    on = float(d2[len(d2) // 2])
    assert np.isnan(ref["grid"][view_ref[False]["d2"] == F32(on)]).all()
    assert len(t) * 3 < len(view_ref[False]["soup"])             # cells with a NaN corner were skipped


# ---- e, g: the sphere, welded on the device

@pytest.mark.parametrize("iso", [0.0, 0.3, -0.3])
def test_sphere_weld_is_closed_and_equals_the_reference(ctx, ball, iso):
    p, n = ball
    put(ctx, 3, p, n)
    ref, v, t, g = check(ctx, 3, p, n, (24, 24, 24), iso=iso, pct=0.2, weld=True)
    assert R.closed_and_oriented(t) and R.euler(len(v), t) == 2
    check(ctx, 3, p, n, (24, 24, 24), iso=iso, pct=0.2)
    vol = R.signed_volume(v, t)
    assert 0.9 < vol / (4.0 / 3.0 * np.pi * (50.0 + iso) ** 3) < 1.01      # outward normals: a positive volume (coarse: the host test has the bound)


def test_iso_level_on_a_lattice_value(ctx, ball):
    """mu = 0: the vertex lies on the corner itself, and `value < iso` leaves that corner outside"""
    p, n = ball
    put(ctx, 3, p, n)
    g0 = R.values(p, n, (24, 24, 24), 0.2)[0]
    # a lattice vertex near the surface whose +x neighbour lies deeper: it is corner 0 of its cell and the `a` end of edge 0
    deeper = g0[1:] < g0[:-1]
    x, y, z = np.unravel_index(np.where(deeper, np.abs(g0[:-1]), np.inf)[:, :-1, :-1].argmin(), (23, 23, 23))
    iso = float(g0[x, y, z])
    ref, v, t, g = check(ctx, 3, p, n, (24, 24, 24), iso=iso, pct=0.2)
    corner = R.lattice(ref["lower"], ref["size"], (24, 24, 24))[x, y, z]
    assert (v == corner).all(1).any()


# ---- f: normals and points that are no numbers

def test_bad_normals_and_non_finite_points(ctx, ball):
    p, n = (a.copy() for a in ball)
    n[::7] = np.nan
    n[1::7] *= F32(0.4)
    n[2::7] = [0.5, 0.0, 0.0]              # a norm of exactly 0.5 is not > 0.5
    n[3::7, 1] = np.nan                    # n.x a number, the norm not
    p[5::50, 0] = np.nan
    p[6::50, 1] = np.inf
    p[7::50, 2] = -np.inf
    put(ctx, 4, p, n)
    for route in (0, 1, 2, 3):                # (the culled search has no rule for such a cloud: 0 and 2 take the tiled one)
        ctx.tune(mc_route=route)
        try:
            ref, v, t, g = check(ctx, 4, p, n, (12, 12, 12), pct=0.1)
            assert ctx.stat("mc_route_used") == (1 if route == 1 else 3)
        finally:
            ctx.tune(mc_route=0)
    assert np.isnan(g).any() and not np.isnan(g).all()
    # no finite point at all: every value NaN, no triangle, MVR_OK
    q = np.full((5, 3), np.nan, F32)
    q[1] = np.inf
    put(ctx, 4, q, np.tile(F32([0, 0, 1]), (5, 1)))
    v, t, g = ctx.marching_cubes_hoppe(4, (4, 4, 4), return_grid=True)
    assert len(v) == 0 and len(t) == 0 and np.isnan(g).all()
    ctx.clear(4)                            # an empty slot: the same (M1)
    v, t, g = ctx.marching_cubes_hoppe(4, (4, 4, 4), return_grid=True, weld=True)
    assert len(v) == 0 and len(t) == 0 and np.isnan(g).all()


# ---- h: M15

def test_flat_cloud(ctx):
    p, n = Cs.flat()
    put(ctx, 5, p, n)
    ref, v, t, g = check(ctx, 5, p, n, (9, 7, 3))
    assert ref["size"][2] == 0 and len(t) > 0 and (v[:, 2] == F32(7.5)).all()
    check(ctx, 5, p, n, (9, 7, 3), weld=True)


# ---- i: M11, M12, M14

def test_sizing_arguments_and_an_untouched_slot(mvr, ctx, ball):
    p, n = ball
    put(ctx, 6, p, n)
    L, h = mvr._lib, ctx._h
    before = ctx.download(6).tobytes(), ctx.download_normals(6).tobytes()
    ref = R.reconstruct(p, n, (16, 16, 16), pct=0.2)
    T = len(ref["soup"]) // 3
    prm = mvr.McParams((C.c_int * 3)(16, 16, 16), 0.0, 0.2, -1.0, 0, 0)
    nt, nv = C.c_uint64(7), C.c_uint64(7)
    assert ctx.marching_cubes_hoppe(6, (16, 16, 16), percentage_extend_grid=0.2, count_only=True) == T
    verts = np.full((3 * T, 3), 9.0, F32)
    grid = np.full(16 ** 3, 9.0, F32)
    vp, gp = verts.ctypes.data_as(C.POINTER(C.c_float)), grid.ctypes.data_as(C.POINTER(C.c_float))
    assert L.mvr_cloud_marching_cubes_hoppe(h, 6, C.byref(prm), gp, vp, T - 1, None, C.byref(nt), C.byref(nv)) == mvr.E_ARG
    assert nt.value == T and (verts == 9.0).all() and (grid == 9.0).all()          # the count and nothing else
    assert L.mvr_cloud_marching_cubes_hoppe(h, 6, C.byref(prm), gp, vp, T, None, C.byref(nt), C.byref(nv)) == mvr.OK
    assert (nt.value, nv.value) == (T, 3 * T) and R.same_bits(verts, ref["soup"]) and R.same_bits(grid.reshape(16, 16, 16), ref["grid"])

    def refused(slot=6, res=(16, 16, 16), iso=0.0, pct=0.2, cap=-1.0, weld=0, params=True, handle=h):
        q = mvr.McParams((C.c_int * 3)(*res), iso, pct, cap, weld, 0)
        a, b = C.c_uint64(7), C.c_uint64(7)
        out = np.full(9, 9.0, F32)
        rc = L.mvr_cloud_marching_cubes_hoppe(handle, slot, C.byref(q) if params else None, None, out.ctypes.data_as(C.POINTER(C.c_float)), 1, None,
                                              C.byref(a), C.byref(b))
        return rc == mvr.E_ARG and a.value == 7 and b.value == 7 and (out == 9.0).all()

    assert refused(handle=None) and refused(params=False) and refused(slot=-1) and refused(slot=mvr.MAX_SLOTS)
    assert refused(res=(1, 16, 16)) and refused(res=(16, 16, 0)) and refused(res=(512, 512, 513)) and refused(res=(2 ** 30, 2 ** 30, 2 ** 30))
    assert refused(iso=np.nan) and refused(iso=np.inf) and refused(pct=np.nan) and refused(pct=np.inf) and refused(pct=-0.1) and refused(cap=np.nan)
    assert refused(weld=1)                                                           # vertices without indices
    ctx.upload(7, p)                                                                 # M1: no normals
    assert refused(slot=7)
    assert (ctx.download(6).tobytes(), ctx.download_normals(6).tobytes()) == before  # M14
