"""GPU tests of the FPFH descriptors (mvr_cloud_fpfh; rules F1-F8 in include/mvr_hip.h) against the numpy reference of
tests/fpfh_ref.py and against anchors that pass through no reference.

The first pass is compared as COUNTS: the integers recovered from the returned SPFH must lie, per query, feature and bin, between
the reference's sure counts and the sure counts plus the query's slack pairs (fpfh_ref: the pairs f32 arithmetic cannot be held
to their f64 bin); a query without a slack pair matches bin for bin, and no query is excluded.  The second pass is compared as
VALUES: the reference's weighting run on the GPU's own SPFH table, every component within one f32 ulp.

Measured on an MI355X (profiles/fpfh_pytest_gpu.log): neighbour counts exact on all four inputs; count differences from the
reference's f64 bins, summed over bins, 4 on the view (5 192 slack pairs), 4 on the view with 76 invalid points, 0 on the box and
on the duplicates; weighting 0 of 659 868 / 99 000 / 657 492 / 49 500 components differ at all, fma off and on; the fma chain
changes no neighbour set on the box and the duplicates; pose invariance, median L1 0.0002 of 300 on the GPU and 0.0002 in the
reference (31.6 between unrelated points).

The targets of the walk cases (fpfh_cases.WALK, WALK_SURFACE) and the four grid resolutions were added later and were NOT
measured on a GPU when they were written: no device could be had.  They were run once against a stand-in context whose
descriptor is the numpy reference."""
import importlib

import numpy as np
import pytest

import fpfh_cases as FC
import fpfh_ref as R
from conftest import PKG
from mls_ref import within_one_ulp

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


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


def run(ctx, p, nrm, radius, fma=False, slot=0):
    ctx.upload(slot, p)
    ctx.upload_normals(slot, nrm)
    f, s, c = ctx.fpfh(slot, radius, fma=fma, return_spfh=True, return_counts=True)
    assert f.shape == s.shape == (len(p), 33) and c.shape == (len(p),)
    return f, s, c


_inputs, _refs, _gpu = {}, {}, {}


def inputs(name, mvr, ctx):
    """(points, normals, radius) of a case; the view's normals are the library's own (radius 2.5 mm)"""
    if name not in _inputs:
        if name in ("view", "invalid"):
            if "view" not in _inputs:
                p = FC.view(mvr)
                ctx.upload(2, p)
                ctx.estimate_normals(2, radius=FC.VIEW_NORMAL_RADIUS)
                _inputs["view"] = (p, ctx.download_normals(2), FC.VIEW_RADIUS)
            if name == "invalid":
                p, nrm, radius = _inputs["view"]
                q, m, bad = FC.with_invalid(p, nrm)
                _inputs["invalid"] = (q, m, radius)
        elif name == "box":
            _inputs[name] = FC.box()
        elif name == "duplicates":
            _inputs[name] = FC.duplicates()
        elif name in FC.WALK + FC.WALK_SURFACE:
            p, nrm, radius = FC.walk(name, mvr)
            if nrm is None:                                               # the library's radius-mode normals of the patch
                ctx.upload(2, p)
                ctx.estimate_normals(2, radius=FC.walk_normal_radius(p))
                nrm = ctx.download_normals(2)
            _inputs[name] = (p, nrm, radius)
    return _inputs[name]


def reference(name, mvr, ctx, fma=False):
    key = (name, fma)
    if key not in _refs:
        p, nrm, radius = inputs(name, mvr, ctx)
        _refs[key] = R.spfh_counts(p, nrm, radius, fma=fma)
    return _refs[key]


def gpu(name, mvr, ctx, fma=False):
    key = (name, fma)
    if key not in _gpu:
        _gpu[key] = run(ctx, *inputs(name, mvr, ctx), fma=fma)
    return _gpu[key]


CASES = ["view", "box", "invalid", "duplicates"] + list(FC.WALK + FC.WALK_SURFACE)


# ------------------------------------------------------------------ the first pass: counts

@pytest.mark.parametrize("name", CASES)
def test_counts(name, mvr, ctx):
    f, s, cnt = gpu(name, mvr, ctx)
    c = reference(name, mvr, ctx)
    n_i = c["n"]
    assert np.array_equal(cnt.astype(np.int64), n_i)
    got = R.counts_from_spfh(s, n_i)
    assert same_bits(R.spfh_from_counts(got, n_i, c["valid"]), s)        # the table IS (float)c * (100.0f / (float)(n_i - 1))
    sure, slack = c["sure"], c["slack"][:, None, None]
    assert (got >= sure).all() and (got <= sure + slack).all()
    tot, st = got.sum(2), sure.sum(2)
    assert (tot >= st).all() and (tot <= st + c["slack"][:, None]).all()
    none = c["slack"] == 0
    assert np.array_equal(got[none], c["full"][none])
    off = int(np.abs(got - c["full"]).sum())
    print("%s: %d queries, %.1f neighbours, %d invalid; %d queries with a slack pair (share %.3f), %d slack pairs; count "
          "differences from the reference's f64 bins, summed over bins: %d (a pair off its bin gives 2 per feature)"
          % (name, len(n_i), n_i.mean(), int((~c["valid"]).sum()), int((~none).sum()), (~none).mean(), int(c["slack"].sum()), off))


# ------------------------------------------------------------------ the second pass: values

@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_weighting_on_the_gpus_own_spfh(name, fma, mvr, ctx):
    p, nrm, radius = inputs(name, mvr, ctx)
    f, s, cnt = gpu(name, mvr, ctx, fma)
    c = reference(name, mvr, ctx, fma)
    want = R.fpfh_from_spfh(p, s, c["I"], c["J"], c["valid"], fma)
    v = c["valid"]
    assert np.isnan(f[~v]).all() and np.isnan(want[~v]).all()
    one = within_one_ulp(f[v], want[v])
    differ = bits(f[v]) != bits(want[v])
    print("%s fma=%d: %d components, beyond one ulp %d, differing at all %d (share %.2e)"
          % (name, fma, differ.size, int((~one).sum()), int(differ.sum()), differ.mean() if differ.size else 0.0))
    assert one.all()


# ------------------------------------------------------------------ anchors that pass through no reference

@pytest.mark.parametrize("name", CASES)
def test_anchors(name, mvr, ctx):
    p, nrm, radius = inputs(name, mvr, ctx)
    f, s, cnt = gpu(name, mvr, ctx)
    valid = np.isfinite(p[:, :3]).all(1) & np.isfinite(nrm[:, :3]).all(1)
    assert np.isnan(f[~valid]).all() and np.isnan(s[~valid]).all() and (cnt[~valid] == 0).all()
    assert np.isfinite(f[valid]).all() and np.isfinite(s[valid]).all() and (cnt[valid] >= 1).all()
    assert (f[valid] >= 0).all() and (s[valid] >= 0).all()
    alone = valid & (cnt == 1)
    assert (f[alone] == 0).all() and (s[alone] == 0).all()
    sums = f[valid].reshape(-1, 3, 11).astype(F64).sum(2)
    assert ((np.abs(sums - 100.0) < 1e-3) | (sums == 0)).all()
    # a block is empty only when no neighbour contributes: every neighbour's SPFH block is empty too, or lies at d2 == 0
    ssum = s[valid].reshape(-1, 3, 11).astype(F64).sum(2)
    assert (ssum <= 100.0 + 1e-3).all()
    live = (sums != 0).all(1)
    print("%s: %d valid, %d alone, %d with three full blocks" % (name, int(valid.sum()), int(alone.sum()), int(live.sum())))
    if name in ("view", "box"):
        assert live.mean() > 0.99


def test_bit_identical_from_run_to_run_and_fma(mvr, ctx):
    for name in ("box", "invalid"):
        p, nrm, radius = inputs(name, mvr, ctx)
        a = gpu(name, mvr, ctx)
        b = run(ctx, p, nrm, radius, slot=3)                              # a fresh slot: a new grid over the same points
        assert all(same_bits(x, y) for x, y in zip(a, b))
        # the optional outputs change nothing
        ctx.upload(3, p); ctx.upload_normals(3, nrm)
        assert same_bits(ctx.fpfh(3, radius), a[0])
    # fma: the first pass does not see d2 beyond the membership test, so where the reference finds the same neighbour sets
    # counts and SPFH are the same bits; the weights 1 / d2 may differ in the last place
    for name in ("box", "duplicates"):
        p, nrm, radius = inputs(name, mvr, ctx)
        a, b = gpu(name, mvr, ctx), gpu(name, mvr, ctx, True)
        ca, cb = reference(name, mvr, ctx), reference(name, mvr, ctx, True)
        n = len(p)
        changed = np.unique(np.setxor1d(ca["I"] * n + ca["J"], cb["I"] * n + cb["J"]) // n)      # queries whose set differs
        print("%s: the fma chain changes the neighbour set of %d queries" % (name, len(changed)))
        assert np.array_equal(b[2], np.bincount(cb["I"], minlength=n))
        keep = np.ones(n, bool)
        keep[changed] = False
        assert same_bits(a[1][keep], b[1][keep]) and np.array_equal(a[2][keep], b[2][keep])
        if len(changed) == 0:
            v = ca["valid"]
            assert np.abs(a[0][v].astype(F64) - b[0][v].astype(F64)).max() < 1e-3


# ------------------------------------------------------------------ the grid's resolution must not show

@pytest.mark.parametrize("name", ["box", "patch_far_1e6"])
def test_results_do_not_depend_on_the_grid_resolution(name, mvr, ctx):
    """seq_cell_points 4 (the default), 1, 64 and 4096 change the cell edge of every grid built afterwards (the cloud is uploaded
    again after each tune).  Neighbour counts and the SPFH table are byte-identical: the counts are integers of per-pair f32
    features, the order of the walk cannot show.  The f64 sums of the weighting run in walk order, so identical bits are not
    promised for the signature: at every resolution it is within one f32 ulp of the reference's weighting of that SPFH"""
    p, nrm, radius = inputs(name, mvr, ctx)
    c = reference(name, mvr, ctx)
    v = c["valid"]
    try:
        base = None
        for cp in (4, 1, 64, 4096):
            ctx.tune(seq_cell_points=cp)
            f, s, cnt = run(ctx, p, nrm, radius, slot=7)
            if base is None:
                base = (f, s, cnt)
                assert np.array_equal(cnt.astype(np.int64), c["n"])
            assert np.array_equal(cnt, base[2]) and same_bits(s, base[1]), (name, cp)
            want = R.fpfh_from_spfh(p, s, c["I"], c["J"], v)
            assert np.isnan(f[~v]).all() and within_one_ulp(f[v], want[v]).all(), (name, cp)
            print("%s seq_cell_points=%d: %d of %d signature components differ from the default resolution's"
                  % (name, cp, int((bits(f[v]) != bits(base[0][v])).sum()), f[v].size))
    finally:
        ctx.tune(seq_cell_points=4)


# ------------------------------------------------------------------ pose invariance

def test_pose_invariance(mvr, ctx):
    p, nrm, radius = inputs("view", mvr, ctx)
    q, m = FC.moved(p, nrm)
    f0 = gpu("view", mvr, ctx)[0]
    f1 = run(ctx, q, m, radius, slot=3)[0]
    r0 = R.fpfh(p, nrm, radius)[0]
    r1 = R.fpfh(q, m, radius)[0]
    v = np.isfinite(f0).all(1) & np.isfinite(f1).all(1)
    assert np.array_equal(v, np.isfinite(r0).all(1) & np.isfinite(r1).all(1))
    got = float(np.median(np.abs(f0[v].astype(F64) - f1[v].astype(F64)).sum(1)))
    ref = float(np.median(np.abs(r0[v].astype(F64) - r1[v].astype(F64)).sum(1)))
    other = float(np.median(np.abs(f0[v].astype(F64) - f0[v][::-1].astype(F64)).sum(1)))
    print("median L1 distance between the signatures of a point before and after the move: GPU %.4f, reference %.4f (of 300; "
          "between unrelated points %.1f)" % (got, ref, other))
    assert got <= 2.0 * ref


# ------------------------------------------------------------------ small clouds, refusals, degenerate sets

def test_small_clouds(mvr, ctx):
    for n in FC.TINY_SIZES:
        p, nrm, radius = FC.tiny(n)
        ctx.upload(4, p)
        if n:
            ctx.upload_normals(4, nrm)
        f, s, c = ctx.fpfh(4, radius, return_spfh=True, return_counts=True)
        assert f.shape == s.shape == (n, 33) and (c == 1).all() and (f == 0).all() and (s == 0).all()
    p, nrm, radius = FC.tiny(5)                                           # the same five within reach of each other
    f, s, c = run(ctx, p, nrm, 2.5, slot=4)
    rf, rs, rc = R.fpfh(p, nrm, 2.5)
    assert np.array_equal(c, rc["n"]) and list(c) == [2, 3, 3, 3, 2]
    if (rc["slack"] == 0).all():
        assert same_bits(s, rs)
    assert within_one_ulp(f, R.fpfh_from_spfh(p, s, rc["I"], rc["J"], rc["valid"])).all()
    # a point with a NaN normal is nobody's neighbour
    nrm[2, 1] = np.nan
    f, s, c = run(ctx, p, nrm, 2.5, slot=4)
    assert list(c) == [2, 2, 0, 2, 2] and np.isnan(f[2]).all() and np.isnan(s[2]).all() and np.isfinite(np.delete(f, 2, 0)).all()


def test_refusals_on_the_device(mvr, ctx):
    p, nrm, radius = FC.tiny(5)
    ctx.upload(5, p)                                                       # a new upload drops the normals
    keep = np.full((5, 33), 9.0, F32)
    import ctypes as C
    prm = mvr.FpfhParams(2.5, 0)
    rc = mvr._lib.mvr_cloud_fpfh(ctx._h, 5, C.byref(prm), keep.ctypes.data_as(C.POINTER(C.c_float)), None, None)
    assert rc == mvr.E_ARG and (keep == 9.0).all()
    with pytest.raises(mvr.MvrError):
        ctx.fpfh(5, 2.5)
    ctx.upload_normals(5, nrm)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(mvr.MvrError):
            ctx.fpfh(5, r)
    with pytest.raises(mvr.MvrError):
        ctx.fpfh(mvr.MAX_SLOTS, 2.5)
    assert mvr._lib.mvr_cloud_fpfh(ctx._h, 5, C.byref(prm), None, None, None) == mvr.OK       # all outputs NULL: the work, no copy
    ctx.upload(5, p[:0])
    assert ctx.fpfh(5, 2.5).shape == (0, 33)                              # an empty cloud is MVR_OK
    p, nrm, radius = FC.box(500)
    ctx.upload(5, p); ctx.upload_normals(5, nrm)
    ctx.fpfh(5, radius)
    assert same_bits(p, ctx.download(5)) and same_bits(nrm, ctx.download_normals(5))      # the slot is not modified


@pytest.mark.parametrize("name", FC.DEGENERATE)
def test_degenerate_sets(name, mvr, ctx):
    p, nrm, radius = FC.degenerate(name, mvr)
    f, s, c = run(ctx, p, nrm, radius, slot=6)
    assert np.isfinite(f).all() and np.isfinite(s).all() and (f >= 0).all() and (c >= 1).all()
    sums = f.reshape(-1, 3, 11).astype(F64).sum(2)
    assert ((np.abs(sums - 100.0) < 1e-3) | (sums == 0)).all()
    print("%s: %d points, radius %.4g, %.1f neighbours, %d points with three full blocks"
          % (name, len(p), radius, c.mean(), int((sums != 0).all(1).sum())))
    if name == "all_identical":
        assert (c == len(p)).all() and (f == 0).all() and (s == 0).all()  # every pair at d2 == 0: no features, no weight
