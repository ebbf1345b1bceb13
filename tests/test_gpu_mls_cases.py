"""mvr_cloud_mls (csrc/mvr_mls.hip, csrc/mvr_plane.h) on the case table of tests/mls_cases.py: the adversarial geometry of
tests/walk_cases.py -- far frames, thousands of points per cell, duplicates, neighbour counts of 5, 6 and 7, abandoned fits --
and clouds in another unit of length.  tests/test_mls_host.py proves every precondition stated here on the reference alone;
DESIGN.md 14 has the table and what the run showed.

  values          kept index, then mls_compare.compare_values against tests/mls_ref.py with the bars of tests/test_gpu_mls.py (one
                  f32 ulp, DIFFER_CAP, the coplanar-curvature rule), the excluded share held to the row's cap first
  properties      on every kept point, excluded or not: w, finiteness, unit normals, the f32 orientation, the curvature's range,
                  and at order 1 a projection that stays inside the ball
  abandoned fits  where the reference abandons the polynomial because a diagonal entry of the normal equations is exactly 0
                  (mls_ref: zero_diag) order 2 returns the bits of order 1.  Any other abandoned fit hangs on the sign of a
                  pivot that is rounding noise (tests/test_mls_host.py shows the reference changing its mind under a
                  permutation of the neighbours); there the test counts and prints, and asserts what holds in any order of
                  summation: the output is finite
  exact shapes    planes, a line, identical points: the answer follows from the arithmetic, no reference
  unit of length  cloud and radius times a power of two: the same kept index, the coordinates times that power and the same
                  normals and curvature, bit for bit, wherever the grid is the unscaled cloud's

Measured on an MI355X (profiles/mls_cases_gpu.log): 98 tests in 41 s, the slowest 2.8 s.  In every row the kept index is the
reference's; in all value comparisons no coordinate and no pinned curvature differs from the reference in a bit and no pinned
normal component is beyond one ulp; 10 972 normal components that are 0 but for rounding are beyond one ulp of their noise, the
largest of them 1.9e-13.  Order 2 returns the bits of order 1 at all 1 012 abandoned fits with a zero diagonal, and at 18 of 18,
222 of 224, 1 of 1 and (narrow weight) 3 497 of 4 004 of the others.  At every scale, 2^-30 included, 0 words differ from the
unscaled run's."""
import importlib

import numpy as np
import pytest

import mls_cases as K
import mls_ref as R
import walk_cases as W
from conftest import PKG
from mls_compare import bits, compare_values, same_bits

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SRC, DST = 0, 1


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def run(ctx, p, radius, **kw):
    """one call on a fresh upload, normals computed: (points, normals, kept index, curvature)"""
    ctx.upload(SRC, p)
    n, idx, curv = ctx.mls(DST, SRC, radius, compute_normals=True, return_index=True, return_curvature=True, **kw)
    out = ctx.download(DST)
    nrm = ctx.download_normals(DST) if n else np.zeros((0, 4), F32)
    assert len(out) == n == len(idx) == len(curv) == len(nrm)
    return out, nrm, idx, curv


_fits = {}


def reference(tag, p, radius, rows, **kw):
    if tag not in _fits:
        _fits[tag] = R.fit(p, radius, rows=rows, **kw)
    return _fits[tag]


def check_properties(what, p, radius, order, out, nrm, idx, curv):
    """the reference-free properties of every kept point"""
    assert (out[:, 3] == 1).all() and (nrm[:, 3] == 0).all(), what
    assert np.isfinite(out).all() and np.isfinite(nrm).all() and np.isfinite(curv).all(), what
    assert np.array_equal(idx, np.unique(idx)) and (len(idx) == 0 or idx[-1] < len(p)), what
    ln = np.sqrt((nrm[:, :3].astype(F64) ** 2).sum(1))
    assert (np.abs(ln - 1.0) <= 2.0 ** -22).all(), what
    src = p[idx, :3]
    assert same_bits(R.flip(nrm[:, :3], F32(0) - src), nrm[:, :3]), what          # M6: the f32 orientation test holds on what came out
    assert (curv >= 0).all() and (curv <= 1.0 / 3.0 + 1e-6).all(), what
    if order <= 1:
        # the plane passes through the mean of points inside the ball, so the foot of the query lies inside it too
        d = np.sqrt(((out[:, :3].astype(F64) - src.astype(F64)) ** 2).sum(1))
        assert (d <= radius * (1.0 + 1e-6)).all(), (what, float(d.max()) if len(d) else 0.0)


def check_values(what, F, rows, p, order, cap, out, nrm, idx, curv):
    """3a on the queries `rows` (None: all): the excluded share against its cap, then the bars of tests/test_gpu_mls.py"""
    keep = F["keep"]
    bad = R.excluded(F, order)
    share = bad.sum() / max(1, int(keep.sum()))
    print("%s: excluded share %.4f, cap %s" % (what, share, cap))
    if cap is None:
        assert share > 0.7, what
        return
    assert share <= cap, what
    ref = R.result(p, F, order, rows=rows)
    at = np.arange(len(p)) if rows is None else np.asarray(rows)
    sel = np.searchsorted(idx, at[keep])
    assert np.array_equal(idx[sel], at[keep]), what
    if keep.any():
        compare_values(what, out[sel, :3], nrm[sel, :3], curv[sel], ref, bad[keep], R.curvature_unpinned(F)[keep],
                       R.normal_unpinned(F, order)[keep])


def check_abandoned(what, F, rows, p, idx, first, second):
    """first / second: (points, normals, curvature) of order 1 and order 2 on the same input.  Where the reference abandoned the
    fit and order 1 does not exclude the point: bit for bit the same where a diagonal entry is exactly 0; elsewhere counted"""
    at = np.arange(len(p)) if rows is None else np.asarray(rows)
    aband = F["keep"] & (F["count"] >= 6) & ~F["fit"] & ~R.excluded(F, 1)
    sel = np.searchsorted(idx, at[aband])
    same = np.ones(len(sel), bool)
    for a, b in zip(first, second):
        if len(sel):
            same &= (bits(a[sel]) == bits(b[sel])).reshape(len(sel), -1).all(1)
    sure = F["zero_diag"][aband]
    print("%s: %d abandoned fits that order 1 does not exclude, %d of them with an exactly zero diagonal; order 2 returns the bits of "
          "order 1 at %d, and at %d of those with the zero diagonal" % (what, len(sel), int(sure.sum()), int(same.sum()), int(same[sure].sum())))
    assert same[sure].all(), what
    return len(sel), int(same.sum())


# ------------------------------------------------------------------ the table

@pytest.mark.parametrize("name,tag", K.case_rows())
def test_case_row(ctx, mvr, name, tag):
    """orders 1 and 2, fma off and on: the kept index in full, the values at the row's queries, the properties everywhere"""
    inp = K.case_input(mvr, name, tag)
    if inp is None:
        assert tag == "whole_cloud" and len(W.get(name, mvr)[1]) > K.WHOLE_CLOUD_MAX
        return
    p, radius, rows = inp
    F = reference((name, tag), p, radius, rows)
    assert not R.membership_differs(p, radius, rows)      # one reference serves both distance chains (the kept set has its own)
    for fma in (False, True):
        kept = R.kept_index(p, radius, fma)
        got = {}
        for order in (1, 2):
            what = "%s %s order %d fma %d" % (name, tag, order, fma)
            out, nrm, idx, curv = run(ctx, p, radius, order=order, fma=fma)
            assert np.array_equal(idx, kept), what
            check_properties(what, p, radius, order, out, nrm, idx, curv)
            check_values(what, F, rows, p, order, K.caps(name, tag)[order - 1], out, nrm, idx, curv)
            got[order] = (out, nrm, curv)
        check_abandoned("%s %s fma %d" % (name, tag, fma), F, rows, p, kept, got[1], got[2])


# ------------------------------------------------------------------ exact shapes

@pytest.mark.parametrize("name", ["planar_sheet", "regular_grid_midpoints"])
def test_a_plane_is_returned_as_it_is(ctx, mvr, name):
    """z = 900 exactly: the covariance has a zero z row, Jacobi never rotates it, the normal is (0, 0, 1) turned towards the
    origin, t = 0; f = 0 at every neighbour, so the right-hand sums are 0 and c = 0 whether or not the fit stands"""
    p = W.get(name, mvr)[1]
    assert (p[:, 2] == 900).all()
    for tag, radius in W.radii(name, p).items():
        if tag in ("zero_r2", "whole_cloud"):
            continue
        for order in (1, 2):
            for fma in (False, True):
                out, nrm, idx, curv = run(ctx, p, radius, order=order, fma=fma)
                what = (name, tag, order, fma)
                assert np.array_equal(idx, R.kept_index(p, radius, fma)), what
                assert same_bits(out, p[idx]), what
                assert (nrm[:, 0] == 0).all() and (nrm[:, 1] == 0).all() and (nrm[:, 2] == -1).all() and (curv == 0).all(), what
        assert tag == "fraction_of_a_cell" or len(idx) == len(p)


def test_a_line_is_returned_as_it_is(ctx, mvr):
    """y = 0, z = 900: the plane's normal is orthogonal to the line and t = 0; at order 2 the tangent pair is (z, x), a = 0 at
    every neighbour, the pivot of a is exactly 0 and the fit is abandoned -- and f = 0 besides"""
    p = W.get("collinear", mvr)[1]
    assert (p[:, 1] == 0).all() and (p[:, 2] == 900).all()
    for tag, radius in W.radii("collinear", p).items():
        if tag == "zero_r2":
            continue
        for order in (1, 2):
            for fma in (False, True):
                out, nrm, idx, curv = run(ctx, p, radius, order=order, fma=fma)
                what = ("collinear", tag, order, fma)
                assert np.array_equal(idx, R.kept_index(p, radius, fma)) and len(idx) >= len(p) - 2, what
                assert same_bits(out, p[idx]), what
                assert (nrm[:, 0] == 0).all() and (curv == 0).all(), what
                check_properties(what, p, radius, order, out, nrm, idx, curv)


def test_identical_points_are_returned_as_they_are(ctx, mvr):
    p = W.get("all_identical", mvr)[1]
    for tag, radius in W.radii("all_identical", p).items():
        if tag == "zero_r2":
            continue
        for order in (1, 2):
            for fma in (False, True):
                out, nrm, idx, curv = run(ctx, p, radius, order=order, fma=fma)
                what = ("all_identical", tag, order, fma)
                assert len(idx) == len(p) and same_bits(out, p) and (curv == 0).all(), what
                check_properties(what, p, radius, order, out, nrm, idx, curv)


# ------------------------------------------------------------------ the unit of length

@pytest.mark.parametrize("name", K.UNIT_CLOUDS)
def test_unit_of_length(ctx, mvr, name):
    """Order 2 with normals, fma off and on, the cloud and the radius times 2^-30, 2^-10, 2^10 and 2^30 (the f32 multiply is
    exact).  The preconditions are computed and asserted here (mls_cases.unit_preconditions): the f32 distances are ordinary
    numbers at every scale, and at 2^-10, 2^10 and 2^30 the grid is the unscaled cloud's.  There the kept index is identical,
    the coordinates are the unscaled ones times the scale and normals and curvature the unscaled ones, BIT FOR BIT.
    At 2^-30 all four clouds are under the 1e-6 of model_grid_size on their shortest side (mls_cases.GRID_MOVES): the grid is
    another one, the f64 sums run in another order, and what is promised is what is promised between two grid resolutions
    (test_results_do_not_depend_on_the_grid_resolution): the same kept index, and the values held to the reference's, which
    are the unscaled reference's times the scale bit for bit (tests/test_mls_host.py)."""
    p, radius, rows = K.case_input(mvr, name, "several_cells")
    F = reference((name, "several_cells"), p, radius, rows)
    cap = K.caps(name, "several_cells")[1]
    pre_of = {s: K.unit_preconditions(p, radius, s) for s in K.UNIT_SCALES}
    for fma in (False, True):
        base = run(ctx, p, radius, order=2, fma=fma)
        for s in K.UNIT_SCALES:
            what = "%s x 2^%d fma %d" % (name, round(np.log2(s)), fma)
            pre = pre_of[s]
            assert pre["d2_ok"], what
            assert pre["box_ok"] == (s not in K.GRID_MOVES), what
            ps = K.scaled(p, s)
            out, nrm, idx, curv = run(ctx, ps, radius * s, order=2, fma=fma)
            assert np.array_equal(idx, base[2]), what
            want = base[0].copy()
            want[:, :3] = base[0][:, :3] * F32(s)
            diff = int((bits(out) != bits(want)).sum()), int((bits(nrm) != bits(base[1])).sum()), int((bits(curv) != bits(base[3])).sum())
            print("%s: grid as unscaled %s; words that differ from the unscaled run's: %d of the points, %d of the normals, %d of the "
                  "curvatures" % ((what, pre["box_ok"]) + diff))
            if pre["box_ok"]:
                assert diff == (0, 0, 0), what
            else:
                check_properties(what, ps, radius * s, 2, out, nrm, idx, curv)
                if cap is not None:
                    Fs = reference((name, "several_cells", s), ps, radius * s, rows)
                    check_values(what, Fs, rows, ps, 2, cap, out, nrm, idx, curv)


@pytest.mark.parametrize("order", [1, 2])
def test_a_patch_in_metres(ctx, mvr, order):
    """patch_at_0 times 2^-10 at several_cells times 2^-10, against the reference with its unit-free rules (in raw coordinates the
    order-2 condition number is 3e12 and every point was excluded): cap 1 %"""
    p, radius, _ = K.case_input(mvr, "patch_at_0", "several_cells")
    s = 2.0 ** -10
    ps = K.scaled(p, s)
    F = reference(("patch_at_0", "metres"), ps, radius * s, None)
    for fma in (False, True):
        what = "patch_at_0 in metres, order %d fma %d" % (order, fma)
        out, nrm, idx, curv = run(ctx, ps, radius * s, order=order, fma=fma)
        assert np.array_equal(idx, R.kept_index(ps, radius * s, fma)), what
        check_properties(what, ps, radius * s, order, out, nrm, idx, curv)
        check_values(what, F, None, ps, order, 0.01, out, nrm, idx, curv)


# ------------------------------------------------------------------ dense cells, weight widths

@pytest.mark.parametrize("name", ["clusters_and_a_far_point", "patch_far_1e6"])
def test_grid_resolution_on_dense_cells(ctx, mvr, name):
    """seq_cell_points 1, 4 and 4096 at several_cells: the kept index is identical and the values are held to the reference at each
    resolution (clusters_and_a_far_point: 2 500 neighbours per point, and at 4096 whole clusters in a cell)"""
    p, radius, rows = K.case_input(mvr, name, "several_cells")
    F = reference((name, "several_cells"), p, radius, rows)
    kept = R.kept_index(p, radius)
    try:
        for cp in (1, 4, 4096):
            ctx.tune(seq_cell_points=cp)
            for order in (1, 2):
                what = "%s several_cells seq_cell_points %d order %d" % (name, cp, order)
                out, nrm, idx, curv = run(ctx, p, radius, order=order)
                assert np.array_equal(idx, kept), what
                check_properties(what, p, radius, order, out, nrm, idx, curv)
                check_values(what, F, rows, p, order, K.caps(name, "several_cells")[order - 1], out, nrm, idx, curv)
    finally:
        ctx.tune(seq_cell_points=4)


@pytest.mark.parametrize("width", sorted(K.WIDTHS))
def test_weight_width(ctx, mvr, width):
    """patch_at_0 at several_cells with sqr_gauss_param = r^2 / 4096 (most weights 0 or denormal: the small-pivot branch of
    mls_solve) and 4096 r^2: the properties everywhere, the values where the reference pins the point.  The narrow width's
    order-2 share is 1 (tests/test_mls_host.py), so order 2 is held to the properties and, where the reference abandoned the
    fit, to what check_abandoned can assert"""
    p, radius, _ = K.case_input(mvr, "patch_at_0", "several_cells")
    g = radius * radius * K.WIDTHS[width]
    F = reference(("patch_at_0", width), p, radius, None, sqr_gauss_param=g)
    kept = R.kept_index(p, radius)
    got = {}
    for order in (1, 2):
        what = "patch_at_0 several_cells, %s weight, order %d" % (width, order)
        out, nrm, idx, curv = run(ctx, p, radius, order=order, sqr_gauss_param=g)
        assert np.array_equal(idx, kept), what
        check_properties(what, p, radius, order, out, nrm, idx, curv)
        check_values(what, F, None, p, order, K.WIDTH_CAPS[width][order - 1], out, nrm, idx, curv)
        got[order] = (out, nrm, curv)
    check_abandoned("patch_at_0 several_cells, %s weight" % width, F, None, p, kept, got[1], got[2])
