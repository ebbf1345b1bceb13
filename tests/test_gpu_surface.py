"""GPU tests of the features at query points over a search surface (mvr_cloud_estimate_normals_at, mvr_cloud_fpfh_at,
mvr_cloud_pfh_at; rules Q1-Q8 in include/mvr_hip.h).

Two kinds of check.  EQUIVALENCE (Q5): a query exactly at a surface point -- through `indices` on the surface's own slot, or as a
copy of the point in another slot -- gets the bits the existing whole-cloud call gives that point; that pins the new entries to
everything the existing tests pin.  OFF THE SURFACE: queries that are no surface point are compared with tests/surface_ref.py --
FPFH within one f32 ulp of the reference's weighting run on the GPU's own full SPFH table (which pins the on-demand SPFH to the
full one), PFH by the count bounds of tests/test_gpu_pfh.py, normals by the bars of tests/test_gpu_normals.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import fpfh_ref as R
import normals_ref as NR
import pfh_cases as PC
import pfh_ref as PR
import surface_cases as SC
import surface_ref as SR
from conftest import PKG
from mls_ref import within_one_ulp

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SURF, QRY, TMP = 0, 1, 2          # slots: the surface with its normals, the query points, the surface's points for the normals calls


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


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


_surfaces = {}


def surface(name, mvr, ctx):
    if name not in _surfaces:
        def view_normals(p, radius):
            ctx.upload(TMP, p)
            ctx.estimate_normals(TMP, radius=radius)
            return ctx.download_normals(TMP)
        _surfaces[name] = SC.surface(name, mvr, view_normals)
    return _surfaces[name]


def put(ctx, slot, p, nrm=None):
    ctx.upload(slot, p)
    if nrm is not None and len(p):
        ctx.upload_normals(slot, nrm)


def normal_radius(name, radius):
    return SC.NORMAL_RADIUS.get(name, radius)


def all_at(ctx, q_slot, s_slot, indices, radius, nradius, fma):
    """every output of the three *_at calls, radius and k modes: a dict of arrays with one row per query"""
    f, fc = ctx.fpfh_at(q_slot, s_slot, radius, indices=indices, fma=fma, return_counts=True)
    h, hc, hn = ctx.pfh_at(q_slot, s_slot, indices=indices, radius=radius, fma=fma, return_counts=True, return_neighbors=True)
    k, kc, kn = ctx.pfh_at(q_slot, s_slot, indices=indices, k=SC.K, fma=fma, return_counts=True, return_neighbors=True)
    nr, cr = ctx.estimate_normals_at(q_slot, s_slot, indices=indices, radius=nradius, fma=fma)
    nk, ck = ctx.estimate_normals_at(q_slot, s_slot, indices=indices, k=SC.K, fma=fma)
    return dict(fpfh=f, fpfh_n=fc, pfh=h, pfh_c=hc, pfh_n=hn, pfhk=k, pfhk_c=kc, pfhk_n=kn, nrm_r=nr, curv_r=cr, nrm_k=nk, curv_k=ck)


def all_full(ctx, p, nrm, radius, nradius, fma):
    """the same outputs from the existing whole-cloud calls on the surface (slot SURF; the normals calls on a copy in TMP)"""
    f, fc = ctx.fpfh(SURF, radius, fma=fma, return_counts=True)
    h, hc, hn = ctx.pfh(SURF, radius=radius, fma=fma, return_counts=True, return_neighbors=True)
    k, kc, kn = ctx.pfh(SURF, k=SC.K, fma=fma, return_counts=True, return_neighbors=True)
    cr = ck = np.zeros(0, F32)
    nr = nk = np.zeros((0, 3), F32)
    if len(p):
        put(ctx, TMP, p)
        cr = ctx.estimate_normals(TMP, radius=nradius, curvature=True, fma=fma)
        nr = ctx.download_normals(TMP)[:, :3].copy()
        ck = ctx.estimate_normals(TMP, k=SC.K, curvature=True, fma=fma)
        nk = ctx.download_normals(TMP)[:, :3].copy()
    return dict(fpfh=f, fpfh_n=fc, pfh=h, pfh_c=hc, pfh_n=hn, pfhk=k, pfhk_c=kc, pfhk_n=kn, nrm_r=nr, curv_r=cr, nrm_k=nk, curv_k=ck)


NEED_NORMAL = ("fpfh", "fpfh_n", "pfh", "pfh_c", "pfh_n", "pfhk", "pfhk_c", "pfhk_n")


def rows_equal(got, full, idx, only=None):
    for key, a in got.items():
        b = full[key][idx]
        if only is not None and key in NEED_NORMAL:
            a, b = a[only], b[only]
        assert same_bits(a, b), key


# ------------------------------------------------------------------ Q5: a query at a surface point

@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("name", SC.SURFACES)
def test_query_at_a_surface_point_gets_the_bits_of_the_existing_call(name, fma, mvr, ctx):
    p, nrm, radius = surface(name, mvr, ctx)
    nradius = normal_radius(name, radius)
    n = len(p)
    put(ctx, SURF, p, nrm)
    full = all_full(ctx, p, nrm, radius, nradius, fma)
    valid = R.valid_mask(p, nrm)
    # (a) a shuffled subset with repeats, through indices on the surface's own slot
    idx = SC.subset_with_repeats(n)
    got = all_at(ctx, SURF, SURF, idx, radius, nradius, fma)
    rows_equal(got, full, idx)
    if n:
        first = {int(i): r for r, i in reversed(list(enumerate(idx)))}
        rep = np.array([first[int(i)] for i in idx[-SC.REPEATS:]])
        for a in got.values():
            assert same_bits(a[-SC.REPEATS:], a[rep])
    # (f) every point, indices None, on the same slot
    rows_equal(all_at(ctx, SURF, SURF, None, radius, nradius, fma), full, np.arange(n))
    # (b) copies of the points in another slot, in another order: positions only, so the rows of the points that are valid
    # under F1 (the others: the tests off the surface below); the normals calls ask no normal of anybody
    put(ctx, QRY, p[idx])
    rows_equal(all_at(ctx, QRY, SURF, None, radius, nradius, fma), full, idx, only=valid[idx])
    # ... and through indices into that slot, reversed
    back = np.arange(len(idx), dtype=np.uint32)[::-1].copy()
    rows_equal(all_at(ctx, QRY, SURF, back, radius, nradius, fma), full, idx[back], only=valid[idx[back]])
    # (e) query slots of 1 and 3 points: no grid of their own
    for m in (1, 3):
        if n >= m:
            put(ctx, QRY, p[idx[:m]])
            rows_equal(all_at(ctx, QRY, SURF, None, radius, nradius, fma), full, idx[:m], only=valid[idx[:m]])


def test_the_query_sort_changes_no_bit(mvr, ctx):
    p, nrm, radius = surface("box", mvr, ctx)
    put(ctx, SURF, p, nrm)
    put(ctx, QRY, SC.off_surface(p))
    base = all_at(ctx, QRY, SURF, None, radius, radius, False)
    assert ctx.stat("at_sort") == 1
    try:
        ctx.tune(at_sort=0)
        got = all_at(ctx, QRY, SURF, None, radius, radius, False)
    finally:
        ctx.tune(at_sort=1)
    for key in base:
        assert same_bits(base[key], got[key]), key


# ------------------------------------------------------------------ queries off the surface, against the reference

def queries_off(name, p, nrm):
    """(c) and (d) in one query set: the moved points, then far / NaN / at a point whose normal is NaN (returned: that point)"""
    bad = np.nonzero(np.isfinite(p[:, :3]).all(1) & ~np.isfinite(nrm[:, :3]).all(1))[0]
    at = int(bad[0]) if len(bad) else min(7, max(len(p) - 1, 0))
    return np.concatenate([SC.off_surface(p), SC.degenerate(p, at)]), at


def with_a_nan_normal(name, p, nrm):
    """the surface with the normal of point 7 (the last point of a smaller cloud) made NaN where the case has no such point"""
    if len(p) and not (np.isfinite(p[:, :3]).all(1) & ~np.isfinite(nrm[:, :3]).all(1)).any():
        nrm = nrm.copy()
        nrm[min(7, len(p) - 1), 1] = np.nan
    return nrm


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("name", SC.OFF_SURFACE)
def test_fpfh_off_the_surface(name, fma, mvr, ctx):
    p, nrm, radius = surface(name, mvr, ctx)
    nrm = with_a_nan_normal(name, p, nrm)
    q, at = queries_off(name, p, nrm)
    put(ctx, SURF, p, nrm)
    put(ctx, QRY, q)
    got, cnt = ctx.fpfh_at(QRY, SURF, radius, fma=fma, return_counts=True)
    marked = ctx.stat("fpfh_at_marked")
    _, spfh, _ = ctx.fpfh(SURF, radius, fma=fma, return_spfh=True, return_counts=True)
    I, J, d2 = SR.hoods_radius(q, p, nrm, radius, fma)
    n_i = SR.neighbor_count(len(q), I)
    assert np.array_equal(cnt.astype(np.int64), n_i)
    large = name in SC.LARGE      # (the tiny surfaces: points 2 mm apart at radius 0.8, every point alone)
    assert marked == len(np.unique(J)) and marked <= len(p) and (marked > 0 or not large)
    want = SR.fpfh_from_spfh(len(q), spfh, I, J, d2)
    none = n_i == 0
    assert none[-3] and none[-2] and none[-1] != large and np.isnan(got[none]).all() and np.isnan(want[none]).all()
    one = within_one_ulp(got[~none], want[~none])
    differ = bits(got[~none]) != bits(want[~none])
    print("%s fma=%d: %d queries, %.1f neighbours, %d of %d SPFH rows computed; %d components, beyond one ulp %d, differing %d"
          % (name, fma, len(q), n_i.mean(), int(marked), len(p), differ.size, int((~one).sum()), int(differ.sum())))
    assert one.all()
    # the query at the point with the NaN normal: a position in another slot (the point itself is nobody's neighbour) ...
    if len(p):
        assert (cnt[-1] > 0) == large and at not in J[I == len(q) - 1] and not np.isfinite(nrm[at, :3]).all()
        # ... and invalid on the surface's own slot (Q2)
        g2, c2 = ctx.fpfh_at(SURF, SURF, radius, indices=[at], fma=fma, return_counts=True)
        assert np.isnan(g2).all() and c2[0] == 0


def pfh_bounds(got, ref):
    got = got.astype(np.int64)
    sure, maybe, slack = ref["sure"], ref["maybe"], ref["slack"]
    assert (got >= sure).all() and (got <= sure + maybe).all()
    tot, st = got.sum(1), sure.sum(1)
    assert (tot >= st).all() and (tot <= st + slack).all()
    none = slack == 0
    assert np.array_equal(got[none], ref["full"][none])
    return int(np.abs(got - ref["full"]).sum()), int(slack.sum())


@pytest.mark.parametrize("mode", ["radius", "radius_fma", "k"])
@pytest.mark.parametrize("name", SC.OFF_SURFACE)
def test_pfh_off_the_surface(name, mode, mvr, ctx):
    p, nrm, radius = surface(name, mvr, ctx)
    nrm = with_a_nan_normal(name, p, nrm)
    q, at = queries_off(name, p, nrm)
    fma = mode == "radius_fma"
    put(ctx, SURF, p, nrm)
    put(ctx, QRY, q)
    kw = dict(k=SC.K) if mode == "k" else dict(radius=radius)
    f, c, nb = ctx.pfh_at(QRY, SURF, fma=fma, return_counts=True, return_neighbors=True, **kw)
    tiled = ctx.stat("pfh_tiled_queries")
    I, J, d2 = SR.hoods_knn(q, p, nrm, SC.K) if mode == "k" else SR.hoods_radius(q, p, nrm, radius, fma)
    rows = SC.reference_rows(name, len(q))
    ref = SR.pfh_counts(len(q), p, nrm, I, J, d2, rows)
    assert np.array_equal(nb.astype(np.int64), SR.neighbor_count(len(q), I)) and np.array_equal(nb[rows].astype(np.int64), ref["n"])
    off, slack = pfh_bounds(c[rows], ref)
    assert same_bits(f, PR.rows_from_counts(c, nb, np.ones(len(q), bool)))
    assert nb[-2] == 0 and np.isnan(f[-2]).all() and (c[-2] == 0).all()                      # the NaN query
    if name in SC.LARGE:
        assert nb[-1] > 0                                                                    # the one at a point: its other neighbours
    if mode == "k":
        assert nb[-3] == min(SC.K, int(R.valid_mask(p, nrm).sum()))                          # the far query has its k neighbours too
    else:
        assert nb[-3] == 0 and np.isnan(f[-3]).all() and (c[-3] == 0).all()
    print("%s %s: %d queries (%d compared), %.1f neighbours (max %d), %d on the tiled path; %d pairs, %d slack; count differences from the "
          "reference's f64 bins, summed over bins: %d" % (name, mode, len(q), len(rows), nb.mean(), nb.max(), int(tiled), ref["pairs"], slack, off))
    if name == "blob" and mode != "k":
        assert tiled == np.isfinite(q[:, :3]).all(1).sum() - 1        # every valid query but the far one
    # the query at the point with the NaN normal, on the surface's own slot: invalid (Q2)
    if len(p):
        f2, c2, n2 = ctx.pfh_at(SURF, SURF, indices=[at], fma=fma, return_counts=True, return_neighbors=True, **kw)
        assert np.isnan(f2).all() and (c2 == 0).all() and n2[0] == 0


@pytest.mark.parametrize("name", ["box", "blob"])
def test_pfh_counts_do_not_depend_on_grid_or_path(name, mvr, ctx):
    p, nrm, radius = surface(name, mvr, ctx)
    q = SC.off_surface(p)
    put(ctx, QRY, q)

    def run():
        put(ctx, SURF, p, nrm)      # a new upload: a new grid at the current resolution
        return ctx.pfh_at(QRY, SURF, radius=radius, return_counts=True, return_neighbors=True)
    base = run()
    try:
        for cp in PC.CELL_POINTS:
            ctx.tune(seq_cell_points=cp)
            assert all(same_bits(x, y) for x, y in zip(base, run())), cp
    finally:
        ctx.tune(seq_cell_points=4)
    try:
        for stage in (64, PC.STAGE):
            ctx.tune(pfh_stage=stage)
            assert all(same_bits(x, y) for x, y in zip(base, run())), stage
    finally:
        ctx.tune(pfh_stage=PC.STAGE)


def compare_normals(nrm, curv, ref, rc, w, q, vp=(0.0, 0.0, 0.0)):
    """the bars of tests/test_gpu_normals.py (_compare_to_reference) for the same quantities"""
    gap = (w[:, 1] - w[:, 0]) / np.where(w[:, 2] != 0, w[:, 2], 1.0)
    ok = ~np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(nrm[:, 0]), ~ok) and np.array_equal(np.isnan(curv), ~ok)
    good = ok & (gap >= 1e-4)
    if good.any():
        ang = NR.angle_between(nrm[good], ref[good], unsigned=True)
        assert ang.max() <= 1e-5, ang.max()
    if ok.any():
        assert np.abs(curv[ok].astype(F64) - rc[ok]).max() <= 1e-6
    v = np.asarray(vp, F64)[None, :] - q[:, :3].astype(F64)
    cs = np.sum(v * ref[:, :3], 1)
    sure = good & (np.abs(cs) > 1e-4 * np.linalg.norm(v, axis=1))
    assert (np.sum(nrm[sure, :3] * ref[sure, :3], 1) > 0).all()
    return int(good.sum()), int(ok.sum())


@pytest.mark.parametrize("name", SC.OFF_SURFACE)
def test_normals_off_the_surface(name, mvr, ctx):
    p, nrm, radius = surface(name, mvr, ctx)
    nradius = normal_radius(name, radius)
    q, _ = queries_off(name, p, nrm)
    put(ctx, SURF, p)                                  # no normals: the normals calls need none
    put(ctx, QRY, q)
    vp = (10.0, -500.0, 200.0)
    for fma in (False, True):
        got, curv = ctx.estimate_normals_at(QRY, SURF, radius=nradius, viewpoint=vp, fma=fma)
        I, J, _ = SR.hoods_radius(q, p, None, nradius, fma)
        ref, rc, w = SR.normals_from_sets(q, p, I, J, vp)
        good, ok = compare_normals(got, curv, ref, rc, w, q, vp)
        large = name in SC.LARGE
        assert np.isnan(got[-3:-1]).all() and (not large or (ok >= 0.9 * len(q) and good >= 0.9 * ok))
        got, curv = ctx.estimate_normals_at(QRY, SURF, k=SC.K, viewpoint=vp, fma=fma)
        ref, rc, w = SR.normals_from_lists(q, p, SC.K, vp, fma)
        good, ok = compare_normals(got, curv, ref, rc, w, q, vp)
        finite = int(np.isfinite(p[:, :3]).all(1).sum())
        assert np.isnan(got[-2]).all() and ok == (len(q) - 1 if finite >= 3 else 0)      # (the far query has its k neighbours too)
        assert not large or good >= 0.9 * ok


def test_normals_into_the_query_slot(mvr, ctx):
    """Q6: store_in_slot puts the normals of the query slot's points, taken from the surface, into the query slot"""
    p, _, radius = surface("box", mvr, ctx)
    q = SC.off_surface(p)
    put(ctx, SURF, p)
    put(ctx, QRY, q)
    want, wc = ctx.estimate_normals_at(QRY, SURF, radius=radius)
    assert len(ctx.download_normals(QRY)) == 0 and len(ctx.download_normals(SURF)) == 0      # store = 0 modifies neither slot
    got, gc = ctx.estimate_normals_at(QRY, SURF, radius=radius, store=True)
    assert same_bits(got, want) and same_bits(gc, wc)
    assert same_bits(ctx.download_normals(QRY)[:, :3].copy(), want) and (ctx.download_normals(QRY)[:, 3] == 0).all()
    assert len(ctx.download_normals(SURF)) == 0
    # the slot against itself, into the slot: the existing call
    got, gc = ctx.estimate_normals_at(SURF, SURF, radius=radius, store=True)
    put(ctx, TMP, p)
    wc = ctx.estimate_normals(TMP, radius=radius, curvature=True)
    assert same_bits(ctx.download_normals(SURF), ctx.download_normals(TMP)) and same_bits(gc, wc)
    assert same_bits(got, ctx.download_normals(TMP)[:, :3].copy())


# ------------------------------------------------------------------ empty sides and refusals

def test_empty_surface_and_empty_query_set(mvr, ctx):
    p, nrm, radius = surface("box", mvr, ctx)
    put(ctx, SURF, np.zeros((0, 4), F32))
    put(ctx, QRY, p[:5])
    f, fc = ctx.fpfh_at(QRY, SURF, radius, return_counts=True)                       # Q7: MVR_OK, the rows of an empty neighbourhood
    assert f.shape == (5, 33) and np.isnan(f).all() and (fc == 0).all()
    for kw in (dict(radius=radius), dict(k=SC.K)):
        h, hc, hn = ctx.pfh_at(QRY, SURF, return_counts=True, return_neighbors=True, **kw)
        assert np.isnan(h).all() and (hc == 0).all() and (hn == 0).all()
        nr, cr = ctx.estimate_normals_at(QRY, SURF, **kw)
        assert np.isnan(nr).all() and np.isnan(cr).all()
    put(ctx, SURF, p, nrm)
    none = np.zeros(0, np.uint32)
    assert ctx.fpfh_at(QRY, SURF, radius, indices=none).shape == (0, 33)             # Q1: rows == 0
    assert ctx.pfh_at(QRY, SURF, indices=none, radius=radius).shape == (0, 125)
    assert ctx.estimate_normals_at(QRY, SURF, indices=none, k=8)[0].shape == (0, 3)


def test_refusals_write_nothing(mvr, ctx):
    p, nrm, radius = surface("box", mvr, ctx)
    put(ctx, SURF, p, nrm)
    put(ctx, QRY, p[:50])
    L, h = mvr._lib, ctx._h
    out, cnt = (C.c_float * 500)(*[9.0] * 500), (C.c_uint32 * 500)(*[9] * 500)
    idx = (C.c_uint32 * 3)(1, 50, 2)                                                  # Q1: an index >= n_q
    fp, pp, npar = mvr.FpfhParams(radius, 0), mvr.PfhParams(radius, 0, 0), mvr.NormalParams(0, radius, (C.c_float * 3)(), 0)
    assert L.mvr_cloud_fpfh_at(h, QRY, idx, 3, SURF, C.byref(fp), out, cnt) == mvr.E_ARG
    assert L.mvr_cloud_pfh_at(h, QRY, idx, 3, SURF, C.byref(pp), out, cnt, cnt) == mvr.E_ARG
    assert L.mvr_cloud_estimate_normals_at(h, QRY, idx, 3, SURF, C.byref(npar), 0, out, out) == mvr.E_ARG
    ok = (C.c_uint32 * 3)(1, 49, 2)                                                   # Q6: store_in_slot with indices
    assert L.mvr_cloud_estimate_normals_at(h, QRY, ok, 3, SURF, C.byref(npar), 1, out, out) == mvr.E_ARG
    assert len(ctx.download_normals(QRY)) == 0
    put(ctx, TMP, p)                                                                  # Q7: a surface without normals
    assert L.mvr_cloud_fpfh_at(h, QRY, ok, 3, TMP, C.byref(fp), out, cnt) == mvr.E_ARG
    assert L.mvr_cloud_pfh_at(h, QRY, ok, 3, TMP, C.byref(pp), out, cnt, cnt) == mvr.E_ARG
    assert L.mvr_cloud_fpfh_at(h, TMP, ok, 3, TMP, C.byref(fp), out, cnt) == mvr.E_ARG
    assert L.mvr_cloud_fpfh_at(h, SURF, ok, 3, QRY, C.byref(fp), out, cnt) == mvr.E_ARG      # (the query slot's normals do not count)
    assert list(out) == [9.0] * 500 and list(cnt) == [9] * 500
    # ... and the query slot needs none
    assert L.mvr_cloud_fpfh_at(h, QRY, ok, 3, SURF, C.byref(fp), out, cnt) == 0
    assert list(cnt[:4]) != [9] * 4 and cnt[3] == 9
