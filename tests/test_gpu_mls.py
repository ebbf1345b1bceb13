"""GPU tests of the moving-least-squares smoothing (mvr_cloud_mls; rules M1-M9 in include/mvr_hip.h) against the numpy
reference of tests/mls_ref.py and against a ground truth that passes through no reference: the generator's noise-free twin
of every point (the same seed with noise_sigma = 0) and its analytic normal.

Value comparisons leave out the points the reference itself cannot pin (mls_ref.excluded: eigen-gap below 1e-6, condition of
the system in units of the radius above 1e10, the two f64 routes more than 1e-9 radii apart); their share is asserted to be 0 on
the synthetic views.  Kept set, order and counts are compared everywhere.  The bars themselves are in tests/mls_compare.py,
shared with tests/test_gpu_mls_cases.py (adversarial clouds, other units of length).

The curvature alone has a further blind spot (coplanar neighbours, always with exactly 3: l0 is rounding noise); it is left out
where the reference's two routes disagree on it (mls_ref.curvature_unpinned); there the reference's curvature and the GPU's must
both lie in [0, 1e-6), and on the 200k view such a point has at most 4 neighbours.

Measured on an MI355X (profiles/mls_pytest_gpu_new_tests.log): in all 8 value cases 0 of 600 000 coordinates, 0 normal
components and 0 pinned curvatures differ from the reference; 1 curvature is unpinned at radius 1 mm.  Ground truth, radius 2.5,
order 2: view 0 at 200k 0.0999 mm in, 0.0196 mm out (reference on 3 000 queries 0.0198), normal error 0.0336 rad (reference
0.0373); twelve views merged, 789 neighbours, 0.1000 mm in, 0.0079 mm out (reference 0.0078), normal error 0.00399 rad
(reference 0.00391), smallest gap 0.395, largest condition 77."""
import importlib

import numpy as np
import pytest

import mls_cases as K
import mls_ref as R
import walk_cases as W
from conftest import PKG
from mls_compare import DIFFER_CAP, FLAT, bits, compare_values, same_bits  # noqa: F401  (the bars, shared with test_gpu_mls_cases.py)

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


synth, with_non_finite = K.synth, K.with_non_finite


@pytest.fixture(scope="module")
def view200k(mvr):
    return synth(mvr, 0, 200000)


@pytest.fixture(scope="module")
def view20k(mvr):
    return synth(mvr, 0, 20000)


_fits = {}


def ref_fit(tag, p, radius, fma=False, rows=None):
    """mls_ref.fit, cached.  The reference is a function of the neighbour sets alone, so where the fma chain changes no
    membership (checked pair by pair) the plain result IS the fma result"""
    if fma and not R.membership_differs(p, radius, rows):
        fma = False
    key = (tag, radius, fma)
    if key not in _fits:
        _fits[key] = R.fit(p, radius, fma=fma, rows=rows)
    return _fits[key]


def mls(ctx, p, radius, dst=1, src=0, normals=None, **kw):
    ctx.upload(src, p)
    if normals is not None:
        ctx.upload_normals(src, normals)
    n, idx, curv = ctx.mls(dst, src, radius, return_index=True, return_curvature=True, **kw)
    out = ctx.download(dst)
    assert len(out) == n == len(idx) == len(curv)
    return out, idx, curv


# ------------------------------------------------------------------ values

@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("radius", [2.5, 1.0])
def test_values_on_a_200k_view(ctx, view200k, radius, order, fma):
    """every coordinate, normal component and curvature within one f32 ulp of the f64 reference rounded to f32, at most 1e-5
    of the coordinates differing at all, nothing excluded"""
    p = view200k[0]
    F = ref_fit("view200k", p, radius, fma)
    ref = R.result(p, F, order)
    out, idx, curv = mls(ctx, p, radius, order=order, compute_normals=True, fma=fma)
    assert np.array_equal(idx, ref["index"])
    bad = R.excluded(F, order)[F["keep"]]
    print("radius %g order %d fma %d: %d of %d kept, mean count %.1f, smallest gap %.3g, largest condition %.3g, routes apart %.3g mm"
          % (radius, order, fma, len(idx), len(p), F["count"].mean(), np.nanmin(F["gap"][F["keep"]]), np.nanmax(F["cond"][F["keep"]]),
             np.nanmax(np.where(F["keep"], F["diff_poly"], 0.0))))
    assert bad.sum() == 0                                 # the cap on the excluded share of a synthetic view is 0
    assert (out[:, 3] == 1).all()
    nrm = ctx.download_normals(1)
    assert (nrm[:, 3] == 0).all()
    flat = R.curvature_unpinned(F)[F["keep"]]
    # on a noisy scan only the sparsest neighbourhoods are coplanar: three points always, four nearly so now and then
    assert (F["count"][F["keep"]][flat] <= 4).all()
    compare_values("radius %g order %d fma %d" % (radius, order, fma), out[:, :3], nrm[:, :3], curv, ref, bad, flat)
    if order == 2:
        assert F["fit"][F["keep"] & (F["count"] >= 6)].all()      # no fit was abandoned on this input


# ------------------------------------------------------------------ exactness of the kept set

def check_kept(ctx, p, radius, what, fma=False):
    ref = R.kept_index(p, radius, fma)
    out, idx, curv = mls(ctx, p, radius, order=2, compute_normals=True, fma=fma)
    assert np.array_equal(idx, ref), what
    nrm = ctx.download_normals(1)
    assert len(nrm) == len(idx) or len(idx) == 0, what
    assert np.isfinite(out).all() and np.isfinite(curv).all() and np.isfinite(nrm[:len(idx)]).all(), what
    return idx


@pytest.mark.parametrize("name", W.NAMES)
def test_kept_set_on_the_walk_cases(ctx, mvr, name):
    """degenerate, far-frame and tie-ridden input: the kept set is the reference's at every radius of the case table, every
    output value is finite (an abandoned fit or a rank-deficient covariance leaves the plane result or the point itself)"""
    q, t = W.get(name, mvr)
    for p in (t, q):
        for tag, r in W.radii(name, t).items():
            for fma in (False, True):
                idx = check_kept(ctx, p, r, (name, len(p), tag, fma), fma)
                if tag == "whole_cloud" and p is t:
                    assert len(idx) == (len(p) if len(p) >= 3 else 0)


def test_results_do_not_depend_on_the_grid_resolution(ctx, view20k):
    """seq_cell_points 4 (the default), 1, 64 and 4096 change the cell edge of every grid built afterwards (mls() uploads the
    cloud again after each tune): the kept index is identical, and the values are held to the reference at each resolution --
    the f64 sums of the fit run in walk order, so identical bits are not promised beyond that"""
    p, radius = view20k[0], 2.5
    F = ref_fit("view20k", p, radius)
    ref = R.result(p, F, 2)
    bad, flat = R.excluded(F, 2)[F["keep"]], R.curvature_unpinned(F)[F["keep"]]
    assert bad.sum() == 0
    try:
        base = None
        for cp in (4, 1, 64, 4096):
            ctx.tune(seq_cell_points=cp)
            out, idx, curv = mls(ctx, p, radius, order=2, compute_normals=True)
            nrm = ctx.download_normals(1)
            if base is None:
                base = (out, idx, curv, nrm)
            assert np.array_equal(idx, ref["index"]) and np.array_equal(idx, base[1]), cp
            compare_values("20k view, radius 2.5, order 2, seq_cell_points %d" % cp, out[:, :3], nrm[:, :3], curv, ref, bad, flat)
            print("seq_cell_points=%d: %d of %d coordinates differ in a bit from the default resolution's"
                  % (cp, int((bits(out[:, :3]) != bits(base[0][:, :3])).sum()), out[:, :3].size))
    finally:
        ctx.tune(seq_cell_points=4)


def test_non_finite_points_are_dropped_and_nobodys_neighbour(ctx, view20k):
    p, bad = with_non_finite(view20k[0])
    fin = R.finite_mask(p)
    assert (~fin).sum() == 60
    for radius, fma in K.NON_FINITE_RUNS:
        F = R.fit(p, radius, fma=fma)
        ref = R.result(p, F, 2)
        assert R.excluded(F, 2).sum() == 0                # the cap on the excluded share of a synthetic view is 0
        out, idx, curv = mls(ctx, p, radius, order=2, compute_normals=True, fma=fma)
        assert np.array_equal(idx, ref["index"]) and not np.isin(bad, idx).any()
        assert (F["count"][~fin] == 0).all() and np.isfinite(out).all()
        compare_values("20k with 60 non-finite points, radius %g" % radius, out[:, :3], ctx.download_normals(1)[:, :3], curv, ref,
                       R.excluded(F, 2)[F["keep"]], R.curvature_unpinned(F)[F["keep"]])
    # nothing finite at all; a finite point among non-finite ones has itself as its only neighbour
    none = np.full((50, 4), np.nan, F32)
    none[::2, 0] = np.inf
    out, idx, curv = mls(ctx, none, 1.0)
    assert len(idx) == 0 and ctx.size(1) == 0
    few = W.cloud(np.random.default_rng(2).standard_normal((10, 3)) + [0, 0, 900])
    few[[0, 2, 3, 5, 6, 8, 9], 0] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf]
    out, idx, curv = mls(ctx, few, 100.0)
    assert list(idx) == [1, 4, 7] and np.array_equal(idx, R.kept_index(few, 100.0))


def test_too_few_neighbours_and_tiny_clouds(ctx):
    """M3: fewer than 3 neighbours drops the point; clouds of 0, 1 and 2 points give an empty output"""
    rng = np.random.default_rng(9)
    p = W.cloud(rng.uniform(-5, 5, (10, 3)) + [0, 0, 900])
    ctx.upload(1, p)
    for n in (0, 1, 2):
        out, idx, curv = mls(ctx, p[:n], 100.0)
        assert len(idx) == 0 and ctx.size(1) == 0
    out, idx, curv = mls(ctx, p[:3], 100.0, compute_normals=True)      # no grid: one cell
    assert list(idx) == [0, 1, 2] and np.isfinite(out).all()
    # a line of points one apart and two stragglers: radius 1 gives the ends 2 neighbours, the inner points 3
    line = W.cloud([[x, 3.0, 900.0] for x in (0, 1, 2, 3, 4, 14, 40)])
    out, idx, curv = mls(ctx, line, 1.0)
    assert list(idx) == [1, 2, 3] and np.array_equal(idx, R.kept_index(line, 1.0))
    assert same_bits(out, line[1:4])                                    # collinear: each point is its own projection
    out, idx, curv = mls(ctx, line, 1.0, order=0)
    assert list(idx) == [1, 2, 3]


# ------------------------------------------------------------------ ground truth

def rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


def normal_error(got, true):
    c = (got.astype(F64) * true.astype(F64)).sum(1)
    return float(np.mean(np.arccos(np.clip(c, -1.0, 1.0))))


def test_ground_truth_on_a_200k_view(ctx, view200k):
    """rms of (out - noise-free twin) . true normal over ALL points against the reference's on 3 000 sampled queries + 10 %
    (the sampling spread of 3 000 queries is under 2 %), and the mean angle of the output normals to the analytic ones.
    Measured: input 0.0999 mm, GPU 0.0196 mm over all points, reference 0.0198 mm on its 3 000 queries; normal error 0.0336 rad
    against the reference's 0.0373."""
    p, true_n, clean = view200k
    rows = K.sample_rows(len(p), K.VIEW_SEED)
    F = R.fit(p, 2.5, rows=rows)
    assert R.excluded(F, 2).sum() == 0
    ref = R.result(p, F, 2, rows=rows)
    k = rows[F["keep"]]
    ref_rms = rms(((ref["xyz64"] - clean[k, :3].astype(F64)) * true_n[k, :3].astype(F64)).sum(1))
    ref_ang = normal_error(ref["normal"], true_n[k, :3])
    out, idx, curv = mls(ctx, p, 2.5, order=2, compute_normals=True)
    nrm = ctx.download_normals(1)
    tn = true_n[idx, :3].astype(F64)
    in_rms = rms(((p[idx, :3].astype(F64) - clean[idx, :3].astype(F64)) * tn).sum(1))
    got_rms = rms(((out[:, :3].astype(F64) - clean[idx, :3].astype(F64)) * tn).sum(1))
    got_ang = normal_error(nrm[:, :3], true_n[idx, :3])
    print("200k view, radius 2.5, order 2: input rms %.4f mm, output rms %.4f mm (reference on 3000 queries %.4f); normal error "
          "%.5f rad (reference %.5f)" % (in_rms, got_rms, ref_rms, got_ang, ref_ang))
    assert len(idx) == len(p)
    assert got_rms <= 1.10 * ref_rms
    assert got_ang <= 1.10 * ref_ang
    assert 0.09 < in_rms < 0.11 and ref_rms < 0.25 * in_rms


@pytest.fixture(scope="module")
def merged(mvr):
    return K.merged_object(mvr)


def test_ground_truth_on_the_merged_object(ctx, merged):
    """the twelve views merged under their true poses, 2.4 M points: the same two bars, the reference on 3 000 sampled
    queries; normals oriented along the uploaded analytic normals (a merged object has no single viewpoint).  Measured: 789
    neighbours, input 0.1000 mm, GPU 0.0079 mm, reference 0.0078 mm; normal error 0.00399 rad against 0.00391."""
    p, true_n, clean = merged
    assert len(p) == 2400000
    rows = K.sample_rows(len(p), K.MERGED_SEED)
    F = R.fit(p, 2.5, rows=rows)
    assert R.excluded(F, 2).sum() == 0                    # the cap on the excluded share of the synthetic views is 0
    ref = R.result(p, F, 2, rows=rows, src_normals=true_n)
    k = rows[F["keep"]]
    ref_rms = rms(((ref["xyz64"] - clean[k]) * true_n[k, :3].astype(F64)).sum(1))
    ref_ang = normal_error(ref["normal"], true_n[k, :3])
    out, idx, curv = mls(ctx, p, 2.5, normals=true_n, order=2, compute_normals=True, orient="normals")
    nrm = ctx.download_normals(1)
    tn = true_n[idx, :3].astype(F64)
    in_rms = rms(((p[idx, :3].astype(F64) - clean[idx]) * tn).sum(1))
    got_rms = rms(((out[:, :3].astype(F64) - clean[idx]) * tn).sum(1))
    got_ang = normal_error(nrm[:, :3], true_n[idx, :3])
    print("merged object, radius 2.5, order 2, mean count %.0f: input rms %.4f mm, output rms %.4f mm (reference on 3000 queries "
          "%.4f); normal error %.5f rad (reference %.5f); smallest gap %.3g, largest condition %.3g, excluded %d"
          % (F["count"].mean(), in_rms, got_rms, ref_rms, got_ang, ref_ang, F["gap"].min(), F["cond"].max(), int(R.excluded(F, 2).sum())))
    assert len(idx) == len(p)
    assert got_rms <= 1.10 * ref_rms
    assert got_ang <= 1.10 * ref_ang
    # the sampled queries themselves, value by value
    sel = np.searchsorted(idx, rows[F["keep"]])
    compare_values("merged object, sampled queries", out[sel, :3], nrm[sel, :3], curv[sel], ref, R.excluded(F, 2)[F["keep"]],
                   R.curvature_unpinned(F)[F["keep"]])


# ------------------------------------------------------------------ behaviour

def test_in_place_equals_out_of_place_and_the_source_stays(ctx, view20k):
    p, nr, _ = view20k
    for kw in (dict(order=2, compute_normals=True), dict(order=1), dict(order=2, compute_normals=True, orient="normals")):
        a = mls(ctx, p, 1.0, dst=1, src=0, normals=nr, **kw)
        na = ctx.download_normals(1)
        assert same_bits(ctx.download(0), p) and same_bits(ctx.download_normals(0), nr)
        b = mls(ctx, p, 1.0, dst=0, src=0, normals=nr, **kw)
        nb = ctx.download_normals(0)
        assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(na, nb)
        assert 0 < len(a[1]) <= len(p) and not same_bits(a[0], p[a[1]])
    # without a grid (3 points) as well
    a = mls(ctx, p[:3], 500.0, dst=1, src=0, compute_normals=True)
    b = mls(ctx, p[:3], 500.0, dst=0, src=0, compute_normals=True)
    assert len(a[1]) == 3 and same_bits(a[0], b[0]) and same_bits(ctx.download_normals(1), ctx.download_normals(0))


def test_normals_follow_their_points_when_not_computed(ctx, view20k):
    p = view20k[0]
    rng = np.random.default_rng(3)
    nr = rng.standard_normal((len(p), 4)).astype(F32)
    nr[:, 3] = 0
    for dst in (1, 0):
        out, idx, curv = mls(ctx, p, 0.6, dst=dst, normals=nr)
        assert 0 < len(idx) < len(p) and same_bits(ctx.download_normals(dst), nr[idx])
    ctx.upload(0, p)                                      # no source normals, none computed: none in the output
    ctx.upload(1, p); ctx.upload_normals(1, nr)
    ctx.mls(1, 0, 0.6)
    assert len(ctx.download_normals(1)) == 0


def test_orient_along_the_uploaded_normals(ctx, view20k):
    p, nr, _ = view20k
    out, idx, curv = mls(ctx, p, 2.5, compute_normals=True)
    towards = ctx.download_normals(1)
    out2, idx2, _ = mls(ctx, p, 2.5, normals=-nr, compute_normals=True, orient="normals")
    away = ctx.download_normals(1)
    assert np.array_equal(idx, idx2) and same_bits(out, out2)
    # each output normal is the same vector up to its side; the f32 test that chose the side holds on what came out
    assert np.array_equal(np.abs(away), np.abs(towards))
    assert same_bits(R.flip(away[:, :3], -nr[idx, :3]), away[:, :3])
    assert same_bits(R.flip(towards[:, :3], F32(0) - p[idx, :3]), towards[:, :3])
    # the analytic normals face the sensor at the origin, their negatives face away: nearly every output normal changes side
    assert ((away[:, :3] * towards[:, :3]).sum(1) < 0).mean() > 0.9
    assert ((away[:, :3].astype(F64) * nr[idx, :3]).sum(1) < 0).mean() > 0.99
    # a viewpoint behind the object turns most of them as well
    mls(ctx, p, 2.5, compute_normals=True, viewpoint=(0.0, 0.0, 3000.0))
    assert ((ctx.download_normals(1)[:, :3] * towards[:, :3]).sum(1) < 0).mean() > 0.8


def test_two_runs_give_identical_bytes(ctx, view200k):
    p = view200k[0]
    a = mls(ctx, p, 2.5, compute_normals=True)
    na = ctx.download_normals(1)
    b = mls(ctx, p, 2.5, compute_normals=True)
    nb = ctx.download_normals(1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    assert na.tobytes() == nb.tobytes()


def test_point_to_plane_icp_runs_on_a_smoothed_slot(ctx, mvr, view20k):
    sp = mvr.synth_params(12, 3)
    piv, ax = mvr.synth_prior(sp)
    ctx.upload(0, view20k[0])
    ctx.nn(0, 0)                                          # orderings / grids of the source exist; none may be reused
    n, idx = ctx.mls(0, 0, 2.5, compute_normals=True, return_index=True)
    smoothed, nrm = ctx.download(0), ctx.download_normals(0)
    ctx.upload(5, smoothed); ctx.upload_normals(5, nrm)
    ctx.upload(6, mvr.synth_view(sp, 1, 20000))
    ctx.transform(6, 6, mvr.axis_rotation(piv, ax, mvr.turntable_angle(1, 12)))
    prm = mvr.icp_params(point_to_plane=True)
    T0, st0, rc0 = ctx.icp_align(6, 0, 7, prm)
    T5, st5, rc5 = ctx.icp_align(6, 5, 7, prm)
    assert rc0 == rc5 == 0 and st0["n_corr"] == st5["n_corr"] > 1000 and np.array_equal(bits(T0), bits(T5))


def test_python_options(ctx, mvr, view20k):
    p = view20k[0]
    ctx.upload(0, p)
    n = ctx.mls(1, 0, 2.5)
    assert isinstance(n, int) and n == ctx.size(1)
    n, idx = ctx.mls(1, 0, 2.5, return_index=True)
    assert len(idx) == n and idx.dtype == np.uint32
    n, curv = ctx.mls(1, 0, 2.5, return_curvature=True)
    assert len(curv) == n and curv.dtype == np.float32
    a = ctx.download(1)
    ctx.mls(1, 0, 2.5, sqr_gauss_param=6.25)              # the default, spelled out
    assert same_bits(a, ctx.download(1))
    ctx.mls(1, 0, 2.5, sqr_gauss_param=1.0)
    assert not same_bits(a, ctx.download(1))
    F = R.fit(p, 2.5, sqr_gauss_param=1.0)
    ref = R.result(p, F, 2)
    assert R.within_one_ulp(ctx.download(1)[:, :3], ref["xyz"]).all()
    ctx.mls(1, 0, 2.5, order=0)
    o0 = ctx.download(1)
    ctx.mls(1, 0, 2.5, order=1)
    assert same_bits(o0, ctx.download(1)) and not same_bits(o0, a)
    with pytest.raises(ValueError):
        ctx.mls(1, 0, 2.5, orient="sideways")


def test_refusals_leave_the_slots_unchanged(ctx, mvr, view20k):
    p = view20k[0]
    ctx.upload(0, p)
    ctx.upload(1, p[:100])
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(order=3), dict(order=-1),
           dict(sqr_gauss_param=-1.0), dict(sqr_gauss_param=np.nan), dict(sqr_gauss_param=np.inf), dict(viewpoint=(0.0, np.nan, 0.0)),
           dict(viewpoint=(np.inf, 0.0, 0.0)), dict(orient="normals"), dict(orient="normals", compute_normals=True)]
    for kw in bad:
        args = dict(radius=2.5)
        args.update(kw)
        with pytest.raises(mvr.MvrError):
            ctx.mls(1, 0, **args)
    with pytest.raises(mvr.MvrError):
        ctx.mls(mvr.MAX_SLOTS, 0, 2.5)
    with pytest.raises(mvr.MvrError):
        ctx.mls(1, -1, 2.5)
    assert same_bits(ctx.download(0), p) and same_bits(ctx.download(1), p[:100])
    assert len(ctx.download_normals(0)) == 0 and len(ctx.download_normals(1)) == 0
    # an empty cloud is fine and empties the destination
    ctx.upload(0, p[:0])
    assert ctx.mls(1, 0, 2.5) == 0 and ctx.size(1) == 0
