"""CPU tests of the moving-least-squares smoothing that need no device: the two f64 routes of the numpy reference
(tests/mls_ref.py) agree, also after rounding to f32, the reference's error against the generator's noise-free points is what its
docstring records, the inputs of the GPU tests exclude no point from value comparisons, the exclusion rules know no unit of
length, the case table of tests/mls_cases.py holds on the reference alone, the library exports mvr_cloud_mls and rejects bad arguments before touching the
GPU, and the kernels of csrc/mvr_mls.hip use no scratch memory while those of csrc/mvr_knn.hip keep their registers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mls_cases as K
import mls_ref as R
import walk_cases as W
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64


synth = K.synth


@pytest.fixture(scope="module")
def view200k(mvr):
    return synth(mvr, 0, 200000)


def rms(x):
    return float(np.sqrt(np.mean(np.square(x))))


def along_normal(xyz64, clean, true_n):
    return ((xyz64 - clean[:, :3].astype(F64)) * true_n[:, :3].astype(F64)).sum(1)


# ------------------------------------------------------------------ the reference against the ground truth

def test_reference_reproduces_the_ground_truth_figures(view200k):
    """View 0 of config 3 at 200 000 points, 3 000 sampled queries, errors rms along the true normal, measured here:

        radius 2.5 mm (111.4 neighbours, at least 46): input 0.1002 mm, order 1 0.0240 mm, order 2 0.0198 mm;
                      smallest gap 0.195, largest condition 323, the two routes 1.1e-13 apart
        radius 1.0 mm (18.6 neighbours, at least 6):   order 1 0.0276 mm, order 2 0.0501 mm (too few neighbours overfit);
                      smallest gap 0.053, largest condition 1.5e5, the two routes 1.1e-13 apart
    """
    p, true_n, clean = view200k
    rows = K.sample_rows(len(p), K.VIEW_SEED)
    e_in = rms(along_normal(p[rows, :3].astype(F64), clean[rows], true_n[rows]))
    got = {}
    for radius in (2.5, 1.0):
        F = R.fit(p, radius, rows=rows)
        assert F["keep"].all() and F["count"].min() >= 6 and F["fit"].all()
        for order in (1, 2):
            res = R.result(p, F, order, rows=rows)
            got[radius, order] = rms(along_normal(res["xyz64"], clean[rows], true_n[rows]))
            assert R.excluded(F, order).sum() == 0
        diff = max(np.nanmax(F["diff_plane"]), np.nanmax(F["diff_poly"]))
        print("radius %g: %.1f neighbours (at least %d), input %.4f, order 1 %.4f, order 2 %.4f mm; smallest gap %.3g, largest "
              "condition %.3g, routes apart %.2e mm" % (radius, F["count"].mean(), F["count"].min(), e_in, got[radius, 1], got[radius, 2],
                                                     F["gap"].min(), F["cond"].max(), diff))
        assert diff <= 1e-11                              # two f64 routes: rounding at |z| = 917 is 1.1e-13
        assert F["gap"].min() > 0.04 and F["cond"].max() < 1e6
    assert abs(e_in - 0.1002) < 0.0005
    assert abs(got[2.5, 1] - 0.0240) < 0.0005 and abs(got[2.5, 2] - 0.0198) < 0.0005
    assert got[1.0, 2] > got[1.0, 1] > got[2.5, 1]        # at 18 neighbours the quadratic overfits


def test_the_two_routes_agree_after_rounding(view200k):
    """every 40th point of the 200k view at radius 2.5 mm: the two routes' f64 coordinates, 1e-13 mm apart, round to the same f32
    in every coordinate, for the plane projection and for the polynomial alike"""
    p = view200k[0]
    rows = np.arange(0, len(p), 40)
    F = R.fit(p, 2.5, rows=rows)
    assert F["keep"].all() and F["fit"].all()
    assert np.nanmax(F["diff_poly"]) <= 1e-11 and np.nanmax(F["diff_plane"]) <= 1e-11
    for a, b in (("plane", "plane_b"), ("poly", "poly_b")):
        assert np.array_equal(F[a].astype(F32).view(np.uint32), F[b].astype(F32).view(np.uint32)), a
    assert not np.array_equal(F["plane"].astype(F32).view(np.uint32), F["poly"].astype(F32).view(np.uint32))


@pytest.mark.parametrize("radius", [2.5, 1.0])
def test_the_gpu_tests_inputs_exclude_nothing(view200k, radius):
    """the excluded share of the inputs tests/test_gpu_mls.py compares values on, against its cap of 0.  Measured: radius 2.5:
    0 of 200 000, smallest gap 0.162, largest condition 463, routes 1.1e-13 mm apart; radius 1.0: 0 of 199 999 (one point has
    fewer than 3 neighbours), smallest gap 0.0058, largest condition 1.1e9, routes 7.3e-11 mm apart, 1 curvature the reference
    cannot pin; the fma chain changes no neighbour set at either radius"""
    p = view200k[0]
    F = R.fit(p, radius)
    for order in (1, 2):
        bad = R.excluded(F, order)
        print("radius %g order %d: %d of %d kept points excluded (share %.2e); smallest gap %.3g, largest condition %.3g, routes "
              "apart %.2e" % (radius, order, int(bad.sum()), int(F["keep"].sum()), bad.sum() / max(1, F["keep"].sum()),
                              np.nanmin(F["gap"][F["keep"]]), np.nanmax(F["cond"][F["keep"]]), np.nanmax(np.where(F["keep"], F["diff_poly"], 0.0))))
        assert bad.sum() == 0
    flat = R.curvature_unpinned(F)
    print("radius %g: %d points whose curvature the reference cannot pin, neighbour counts %s" % (radius, int(flat.sum()), sorted(set(F["count"][flat]))))
    assert (F["curv"][flat] < 1e-6).all()                 # (nearly) coplanar neighbours only: three points always are
    assert (F["count"][flat] <= 4).all()                  # ... and on a noisy scan only the sparsest neighbourhoods
    print("radius %g: the fma chain changes a neighbour set: %s" % (radius, R.membership_differs(p, radius)))


def test_the_view_with_non_finite_points_excludes_nothing(mvr):
    """the 20k view with 60 non-finite points, at the radii and distance chains tests/test_gpu_mls.py runs it with.  Measured:
    nothing excluded; curvatures the reference cannot pin: 5 300 of 10 454 kept points at 1 mm (half the kept points have exactly 3
    neighbours), 18 of 19 936 at 2.5 mm"""
    p, bad = K.with_non_finite(synth(mvr, 0, 20000)[0])
    for radius, fma in K.NON_FINITE_RUNS:
        F = R.fit(p, radius, fma=fma)
        ex, flat = R.excluded(F, 2), R.curvature_unpinned(F)
        print("radius %g fma %d: %d of %d kept points excluded, %d curvatures not pinned; smallest gap %.3g, largest condition %.3g"
              % (radius, fma, int(ex.sum()), int(F["keep"].sum()), int(flat.sum()), np.nanmin(F["gap"][F["keep"]]), np.nanmax(F["cond"][F["keep"]])))
        assert ex.sum() == 0 and not F["keep"][bad].any() and (F["curv"][flat] < 1e-6).all()


def test_the_merged_objects_sampled_queries_exclude_nothing(mvr):
    """the 3 000 sampled queries of the twelve views merged under their true poses (2.4 M points), radius 2.5 mm.  Measured: 789
    neighbours, nothing excluded, every curvature pinned, smallest gap 0.395, largest condition 77"""
    p, _, _ = K.merged_object(mvr)
    rows = K.sample_rows(len(p), K.MERGED_SEED)
    F = R.fit(p, 2.5, rows=rows)
    print("merged object: %.0f neighbours, %d of %d excluded, %d curvatures not pinned; smallest gap %.3g, largest condition %.3g"
          % (F["count"].mean(), int(R.excluded(F, 2).sum()), int(F["keep"].sum()), int(R.curvature_unpinned(F).sum()), F["gap"].min(), F["cond"].max()))
    assert F["keep"].all() and R.excluded(F, 2).sum() == 0 and R.curvature_unpinned(F).sum() == 0


def test_the_20k_view_at_a_weight_width_of_1_excludes_nothing(mvr):
    """the input of test_python_options (tests/test_gpu_mls.py): radius 2.5 mm, sqr_gauss_param = 1"""
    p = synth(mvr, 0, 20000)[0]
    F = R.fit(p, 2.5, sqr_gauss_param=1.0)
    print("20k view, sqr_gauss_param 1: %d of %d excluded; largest condition %.3g raw, %.3g in radii; routes apart %.2e radii"
          % (int(R.excluded(F, 2).sum()), int(F["keep"].sum()), np.nanmax(F["cond"][F["keep"]]), np.nanmax(F["cond_r"][F["keep"]]),
             np.nanmax(np.where(F["keep"], F["rel_poly"], 0.0))))
    assert R.excluded(F, 1).sum() == 0 and R.excluded(F, 2).sum() == 0


# ------------------------------------------------------------------ the exclusion rules know no unit of length

@pytest.mark.parametrize("name", ["patch_at_0", "huge_coordinates"])
def test_the_reference_knows_no_unit_of_length(mvr, name):
    """the target cloud of the walk case at several_cells, cloud and radius times 2^-30, 2^-10, 2^10 and 2^30 (exact in f32):
    excluded() returns the mask of the unscaled cloud at both orders, and route A's plane and poly are the unscaled ones times
    the scale, its normal, poly_normal and curv the unscaled ones, BIT FOR BIT in f64.  Measured: shares 0 / 0 at every scale on
    both clouds.  Under the rules in raw coordinates (cond > 1e10 on the raw system, routes 1e-9 apart as a length) order 2
    excluded all of patch_at_0 at 2^-10 (metres; cond 3e12), 2^10 and 2^30, and all of huge_coordinates unscaled (cond 1.5e21,
    routes 3e-6 apart) but none of it at 2^-17."""
    t, r, _ = K.case_input(mvr, name, "several_cells")
    rows = K.sample_rows(len(t), 11, 500)
    F0 = R.fit(t, r, rows=rows)
    m0 = [R.excluded(F0, o) for o in (1, 2)]
    print("%s: unscaled, radius %.6g: excluded %d / %d of %d; largest condition %.3g raw, %.3g in radii" %
          (name, r, int(m0[0].sum()), int(m0[1].sum()), int(F0["keep"].sum()), np.nanmax(F0["cond"]), np.nanmax(F0["cond_r"])))
    assert F0["keep"].all() and (F0["count"] >= 6).all()
    for s in K.UNIT_SCALES:
        F = R.fit(K.scaled(t, s), r * s, rows=rows)
        m = [R.excluded(F, o) for o in (1, 2)]
        print("%s x 2^%d: excluded %d / %d; largest condition %.3g raw, %.3g in radii; max |poly / s - poly| = %.3g"
              % (name, round(np.log2(s)), int(m[0].sum()), int(m[1].sum()), np.nanmax(F["cond"]), np.nanmax(F["cond_r"]),
                 np.abs(F["poly"] / s - F0["poly"]).max()))
        assert np.array_equal(F["count"], F0["count"]) and np.array_equal(F["fit"], F0["fit"])
        assert np.array_equal(m[0], m0[0]) and np.array_equal(m[1], m0[1])
        for k in ("plane", "poly"):
            assert np.array_equal((F0[k] * s).view(np.uint64), F[k].view(np.uint64)), (k, s)
        for k in ("normal", "poly_normal", "curv", "gap"):
            assert np.array_equal(F0[k].view(np.uint64), F[k].view(np.uint64)), (k, s)


# ------------------------------------------------------------------ the case table of tests/test_gpu_mls_cases.py

_records = {}


def row_record(mvr, name, tag):
    """what the reference alone says about a row of the table (None: the row does not exist)"""
    if (name, tag) in _records:
        return _records[name, tag]
    inp = K.case_input(mvr, name, tag)
    rec = None
    if inp is not None:
        t, r, rows = inp
        F = R.fit(t, r, rows=rows)
        keep, cnt = F["keep"], F["count"]
        ex = [R.excluded(F, o) for o in (1, 2)]
        aband = keep & (cnt >= 6) & ~F["fit"]
        rec = dict(n=len(t), radius=r, compared=len(cnt), kept=int(keep.sum()),
                   share=tuple(float(e.sum()) / max(1, int(keep.sum())) for e in ex),
                   counts=tuple(int((cnt[keep] == c).sum()) for c in (5, 6, 7)), max_count=int(cnt.max()) if len(cnt) else 0,
                   abandoned=int(aband.sum()), abandoned_not_excluded=int((aband & ~ex[0]).sum()),
                   abandoned_for_good=int((aband & ~ex[0] & F["zero_diag"]).sum()), zero_diag_kept=int((F["zero_diag"] & F["fit"]).sum()),
                   fma_differs=R.membership_differs(t, r, rows), unpinned=int(R.curvature_unpinned(F).sum()))
        if rows is not None:
            full = R.counts(t, r)
            rec["sample_has_the_sparse"] = bool(np.isin(np.nonzero((full >= 5) & (full <= 7))[0], rows).all()) and len(rows) <= K.SAMPLE
    _records[name, tag] = rec
    return rec


@pytest.mark.parametrize("name,tag", K.case_rows())
def test_case_table_row(mvr, name, tag):
    """the reference alone stays within the row's caps on the excluded share (tests/mls_cases.py: conditions set by rule from
    the measured share), and a sampled row's sample holds every point with 5, 6 or 7 neighbours"""
    rec = row_record(mvr, name, tag)
    if rec is None:
        assert tag == "whole_cloud" and len(W.get(name, mvr)[1]) > K.WHOLE_CLOUD_MAX
        return
    print("%s %s: radius %.6g, %d points, %d compared, %d kept; excluded share %.4f / %.4f against caps %s; kept points with 5 / 6 / 7 "
          "neighbours %d / %d / %d (largest count %d); abandoned fits %d, not excluded at order 1 %d, of them with an exactly zero "
          "diagonal %d; curvatures not pinned %d; the fma chain changes a neighbour set: %s"
          % ((name, tag, rec["radius"], rec["n"], rec["compared"], rec["kept"]) + rec["share"] + (K.caps(name, tag),) + rec["counts"] +
             (rec["max_count"], rec["abandoned"], rec["abandoned_not_excluded"], rec["abandoned_for_good"], rec["unpinned"], rec["fma_differs"])))
    for share, cap in zip(rec["share"], K.caps(name, tag)):
        if cap is None:
            assert share > 0.7                            # a row compares no values only where the rule says so
        else:
            assert share <= cap
            assert cap == 0.01 or share > cap - 0.05      # ... and a wider cap is the share rounded up to the next 0.05
    assert ((name, tag) in K.SAMPLED) == ("sample_has_the_sparse" in rec) and rec.get("sample_has_the_sparse", True)
    assert rec["zero_diag_kept"] == 0                     # an exactly zero diagonal entry always abandons the fit
    assert not rec["fma_differs"]                         # one reference per row serves both distance chains


def test_case_table_as_a_whole(mvr):
    """every (walk case, radius tag) is a row; exactly the rows named in mls_cases.CAPS compare no values or fewer; across the
    table there are kept points with exactly 5, exactly 6 and exactly 7 neighbours, rows with abandoned fits that order 1 does
    not exclude and rows with none, and rows where an abandoned fit does not hang on a rounding (an exactly zero diagonal)"""
    rows = K.case_rows()
    assert len(rows) == len(set(rows)) and set(K.CAPS) <= set(rows) and K.SAMPLED <= set(rows)
    for name in W.NAMES:
        tags = set(W.radii(name, W.get(name, mvr)[1])) - {"zero_r2"}
        assert tags == {t for n, t in rows if n == name}
    recs = {k: row_record(mvr, *k) for k in rows}
    live = {k: v for k, v in recs.items() if v is not None}
    assert all((k[1] == "whole_cloud" and len(W.get(k[0], mvr)[1]) > K.WHOLE_CLOUD_MAX) for k in recs if recs[k] is None)
    tot = np.sum([v["counts"] for v in live.values()], axis=0)
    print("%d rows; kept points with exactly 5 / 6 / 7 neighbours: %d / %d / %d" % ((len(live),) + tuple(tot)))
    assert (tot > 0).all()
    some = sorted(k for k, v in live.items() if v["abandoned_not_excluded"] > 0)
    good = sorted(k for k, v in live.items() if v["abandoned_for_good"] > 0)
    print("rows with abandoned fits that order 1 does not exclude: %s; with an exactly zero diagonal among them: %s" % (some, good))
    assert ("every_target_duplicated", "several_cells") in some and ("lattice_3d", "lattice_distance") in good
    assert any(v["abandoned"] == 0 and v["kept"] > 0 and v["max_count"] >= 6 for v in live.values())
    none = sorted(k for k in live if None in K.caps(*k))
    print("rows that compare no values at an order: %s" % none)
    assert set(none) == {k for k in K.CAPS if None in K.CAPS[k]}


def test_an_abandoned_fit_hangs_on_a_rounding_unless_a_diagonal_is_zero(mvr):
    """Route A on the same neighbours in another order of summation: the normal equations of fewer than 6 distinct points (or
    of 6 weights of which all but a few have underflowed) are singular, the failing pivot is rounding noise about 0, and
    whether the fit is abandoned changes with the order -- on every_target_duplicated at 2 of the sample's 18 abandoned fits, at
    the narrow weight of patch_at_0 at 138 of the 665 among 1 000 sampled queries.  So 'the reference abandoned the fit' says nothing about
    another implementation's sums, and the GPU test holds order 2 to order 1 bit for bit only where a diagonal entry is exactly
    0 (zero_diag: the lattice's 1 012 face points): there no order changes it."""
    def flags(t, r, rows, g, seed):
        fit, zero = [], []
        for _, q, X, member in R._chunks(t, r, False, rows):
            if seed:
                o = np.random.default_rng(seed).permutation(X.shape[1])
                X, member = X[:, o], member[:, o]
            A = R._route_a(q, X, member, g, r)
            fit.append(A["fit"] | (A["count"] < 6)); zero.append(A["zero_diag"])
        return np.concatenate(fit), np.concatenate(zero)
    changed = {}
    for what, row, factor, nrows in (("duplicated", ("every_target_duplicated", "several_cells"), 1.0, None),
                                     ("narrow", ("patch_at_0", "several_cells"), K.WIDTHS["narrow"], 1000),
                                     ("lattice", ("lattice_3d", "lattice_distance"), 1.0, None)):
        t, r, rows = K.case_input(mvr, *row)
        if nrows:
            rows = K.sample_rows(len(t), 13, nrows)
        f0, z0 = flags(t, r, rows, r * r * factor, 0)
        ch = np.zeros(len(f0), bool)
        for seed in (1, 2, 3):
            f, z = flags(t, r, rows, r * r * factor, seed)
            assert np.array_equal(z, z0) and not f[z0].any()
            ch |= f != f0
        changed[what] = int(ch.sum())
        print("%s: %d abandoned fits, %d with an exactly zero diagonal; the decision changes under a permutation at %d"
              % (what, int((~f0).sum()), int(z0.sum()), changed[what]))
        assert not ch[z0].any()
    assert changed["lattice"] == 0 and changed["narrow"] > 0


@pytest.mark.parametrize("width", sorted(K.WIDTHS))
def test_the_weight_widths_stay_within_their_caps(mvr, width):
    """patch_at_0 at several_cells with sqr_gauss_param = r^2 / 4096 and 4096 r^2.  Measured: narrow 0 / 1.0 (4 004 of 6 000
    fits abandoned, the condition number in radii up to 1.9e80: all weights but the nearest few are 0 or denormal), wide 0 / 0
    (largest condition 916)"""
    t, r, _ = K.case_input(mvr, "patch_at_0", "several_cells")
    F = R.fit(t, r, sqr_gauss_param=r * r * K.WIDTHS[width])
    share = [R.excluded(F, o).sum() / F["keep"].sum() for o in (1, 2)]
    aband = F["keep"] & (F["count"] >= 6) & ~F["fit"]
    print("%s: excluded share %.4f / %.4f, abandoned fits %d, largest condition in radii %.3g"
          % (width, share[0], share[1], int(aband.sum()), np.nanmax(F["cond_r"])))
    for sh, cap in zip(share, K.WIDTH_CAPS[width]):
        assert sh > 0.7 if cap is None else sh <= cap


def test_the_patch_in_metres_excludes_nothing(mvr):
    """patch_at_0 times 2^-10 at several_cells times 2^-10, the case the rules in raw coordinates excluded completely at order 2
    (cond 3e12): measured 0 / 0 of 6 000, largest condition in radii 892"""
    t, r, _ = K.case_input(mvr, "patch_at_0", "several_cells")
    s = 2.0 ** -10
    F = R.fit(K.scaled(t, s), r * s)
    print("patch_at_0 in metres: excluded %d / %d of %d; largest condition %.3g raw, %.3g in radii"
          % (int(R.excluded(F, 1).sum()), int(R.excluded(F, 2).sum()), int(F["keep"].sum()), np.nanmax(F["cond"]), np.nanmax(F["cond_r"])))
    assert F["keep"].all() and R.excluded(F, 1).sum() == 0 and R.excluded(F, 2).sum() <= 0.01 * len(t)
    assert np.nanmax(F["cond"]) > 1e10                    # what the raw rule saw


@pytest.mark.parametrize("name", K.UNIT_CLOUDS)
def test_the_unit_of_length_preconditions(mvr, name):
    """what test_unit_of_length (tests/test_gpu_mls_cases.py) states before it compares a bit.  At 2^-10, 2^10 and 2^30 both hold
    on all four clouds.  At 2^-30 the f32 distances are still ordinary numbers, but the scaled box is 4.6e-9 to 1.5e-8 wide on
    its shortest side: under the 1e-6 that model_grid_size lifts an extent to, so the grid is another one (K.GRID_MOVES)"""
    t, r, _ = K.case_input(mvr, name, "several_cells")
    for s in K.UNIT_SCALES:
        pre = K.unit_preconditions(t, r, s)
        print("%s x 2^%d: %s" % (name, round(np.log2(s)), pre))
        assert pre["d2_ok"] and pre["box_ok"] == (s not in K.GRID_MOVES)


# ------------------------------------------------------------------ the reference, by hand

def cloud(xyz):
    p = np.ones((len(xyz), 4), F32)
    p[:, :3] = np.asarray(xyz, F32)
    return p


def test_reference_recovers_an_exact_quadric():
    """points ON z = 900 + 0.02 x^2 - 0.01 x y + 0.015 y^2 + 0.03 x (a polynomial of total degree 2 over a plane stays one over
    any other plane only approximately -- but a quadric sampled finely is fitted to far below the step): the projected point
    lies on the surface, the normal is the surface normal"""
    g = np.stack(np.meshgrid(np.linspace(-3, 3, 61), np.linspace(-3, 3, 61), indexing="ij"), -1).reshape(-1, 2)
    z = 900 + 0.02 * g[:, 0] ** 2 - 0.01 * g[:, 0] * g[:, 1] + 0.015 * g[:, 1] ** 2 + 0.03 * g[:, 0]
    p = cloud(np.c_[g, z])
    mid = np.nonzero((np.abs(g) < 1.0).all(1))[0]
    F = R.fit(p, 1.5, rows=mid)
    res = R.result(p, F, 2, rows=mid)
    x, y = res["xyz64"][:, 0], res["xyz64"][:, 1]
    on = 900 + 0.02 * x ** 2 - 0.01 * x * y + 0.015 * y ** 2 + 0.03 * x
    assert np.abs(res["xyz64"][:, 2] - on).max() < 2e-4  # (f32 storage of z at 900: 6e-5)
    nt = np.c_[-(0.04 * x - 0.01 * y + 0.03), -(-0.01 * x + 0.03 * y), np.ones_like(x)]
    nt /= np.linalg.norm(nt, axis=1, keepdims=True)
    assert np.abs(np.abs((res["normal"].astype(F64) * nt).sum(1)) - 1).max() < 1e-6
    assert (((0 - p[mid, :3]) * res["normal"]).sum(1) >= 0).all()        # towards the viewpoint at the origin


def test_reference_counts_and_drops():
    line = cloud([[x, 3.0, 900.0] for x in (0, 1, 2, 3, 4, 14, 40)])
    assert list(R.counts(line, 1.0)) == [2, 3, 3, 3, 2, 1, 1] and list(R.kept_index(line, 1.0)) == [1, 2, 3]
    line[2, 1] = np.nan
    assert list(R.counts(line, 1.0)) == [2, 2, 0, 2, 2, 1, 1] and len(R.kept_index(line, 1.0)) == 0
    F = R.fit(line, 2.0)
    assert list(F["count"]) == [2, 3, 0, 3, 2, 1, 1] and list(R.result(line, F, 2)["index"]) == [1, 3]
    for n in (0, 1, 2):
        assert len(R.kept_index(line[:n], 100.0)) == 0
    none = np.full((5, 4), np.nan, F32)
    assert len(R.kept_index(none, 1.0)) == 0 and not R.fit(none, 1.0)["keep"].any()


def test_within_one_ulp():
    a = F32([1.0, -1.0, 0.0, 917.0])
    assert R.within_one_ulp(a, a).all()
    assert R.within_one_ulp(np.nextafter(a, F32(np.inf)), a).all() and R.within_one_ulp(np.nextafter(a, F32(-np.inf)), a).all()
    two = np.nextafter(np.nextafter(a, F32(np.inf)), F32(np.inf))
    assert not R.within_one_ulp(two, a).any()


# ------------------------------------------------------------------ the C-ABI

def test_library_exports_mvr_cloud_mls(mvr):
    assert "mvr_cloud_mls" in mvr.SIGNATURES
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    assert re.search(r" T mvr_cloud_mls$", r.stdout, re.M)
    assert C.sizeof(mvr.MlsParams) == 48                  # double, int, double, int, int, float[3], int: the header's layout


def test_mls_rejects_bad_arguments_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                    # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    n = C.c_size_t(7)
    idx = (C.c_uint32 * 4)(9, 9, 9, 9)
    curv = (C.c_float * 4)(9, 9, 9, 9)

    def prm(radius=2.5, order=2, g=0.0, normals=0, orient=0, vp=(0.0, 0.0, 0.0), fma=0):
        return mvr.MlsParams(radius, order, g, normals, orient, (C.c_float * 3)(*vp), fma)

    f = L.mvr_cloud_mls
    assert f(None, 0, 1, C.byref(prm()), C.byref(n), idx, curv) == mvr.E_ARG
    assert f(ctx, 0, 1, None, C.byref(n), idx, curv) == mvr.E_ARG
    for d, s in ((-1, 0), (0, -1), (mvr.MAX_SLOTS, 0), (0, mvr.MAX_SLOTS)):
        assert f(ctx, d, s, C.byref(prm()), C.byref(n), idx, curv) == mvr.E_ARG
    for r in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert f(ctx, 0, 1, C.byref(prm(radius=r)), C.byref(n), idx, curv) == mvr.E_ARG
    for g in (-1.0, math.nan, math.inf, -math.inf):
        assert f(ctx, 0, 1, C.byref(prm(g=g)), C.byref(n), idx, curv) == mvr.E_ARG
    for o in (-1, 3, 1 << 20):
        assert f(ctx, 0, 1, C.byref(prm(order=o)), C.byref(n), idx, curv) == mvr.E_ARG
    for o in (-1, 2):
        assert f(ctx, 0, 1, C.byref(prm(orient=o)), C.byref(n), idx, curv) == mvr.E_ARG
    for vp in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf)):
        assert f(ctx, 0, 1, C.byref(prm(vp=vp)), C.byref(n), idx, curv) == mvr.E_ARG
    assert n.value == 7 and list(idx) == [9] * 4 and list(curv) == [9.0] * 4
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the kernels' resources

def _usage(built, tmp_path, name):
    """[(kernel, VGPRs, scratch bytes per lane)] from the compiler's remarks for one source file (device code only)"""
    src = os.path.join(ROOT, PKG, "csrc", name)
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / (name + ".o")),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    return [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
             int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))) for b in blocks]


def test_mls_kernels_use_no_scratch(built, tmp_path):
    use = _usage(built, tmp_path, "mvr_mls.hip")
    own = [(n, v, s) for n, v, s in use if "mls_" in n]
    print(own)
    assert len(own) == 5, own                             # the fit x fma x order 2, the curvature gather
    assert all(s == 0 for _, _, s in use), [(n, s) for n, _, s in use if s]


def test_knn_kernels_keep_their_registers(built, tmp_path):
    """Moments, the Jacobi rotation and the eigenvector pick moved into csrc/mvr_plane.h: the kernels of mvr_knn.hip are
    allocated what they were before the move (the counts of the parent commit, gfx950)"""
    before = {"knn_kernelILi8E": 100, "knn_kernelILi16E": 150, "knn_kernelILi32E": 116, "knn_kernelILi64E": 181,
              "normals_knn_kernelILi8E": 100, "normals_knn_kernelILi16E": 151, "normals_knn_kernelILi32E": 117,
              "normals_knn_kernelILi64E": 182, "normals_radius_kernelIL": 54}
    use = _usage(built, tmp_path, "mvr_knn.hip")
    assert len(use) == 18 and all(s == 0 for _, _, s in use)
    for name, v, _ in use:
        key = [k for k in before if re.search(r"\d+" + re.escape(k), name)]
        assert len(key) == 1, name
        assert v == before[key[0]], (name, v, before[key[0]])
