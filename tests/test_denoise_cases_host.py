"""What tests/denoise_cases.py states about its cases, proved on the references alone (no GPU): the brute-force reference of
tests/denoise_ref.py equals oracle.denoise on every finite case (two independent searches: all pairs against a grid), the closed
forms hold, no pair lies within 1e-12 (relative) of a radius unless the case declares the tie, every surface or volume case has
a call that keeps a proper subset in two or more components, and nothing is left out of the GPU test."""
import importlib

import numpy as np
import pytest

import denoise_cases as D
import denoise_ref as R
import walk_cases as W
from conftest import PKG

MIN_MARGIN = 1e-12
LEFT_OUT_SHARE = 0.0            # of the cases, by tests/test_gpu_denoise_cases.py


@pytest.fixture(scope="module")
def mvr():
    return importlib.import_module(PKG)          # the scan generator is host code


def expected(case, tag, thr, ref):
    """the kept indices of a call: the closed form where there is one, else the reference"""
    if tag in case.closed and thr in case.closed[tag][1]:
        return np.asarray(case.closed[tag][1][thr], np.uint32)
    return R.select(ref[tag][0], thr)


@pytest.mark.parametrize("name", D.NAMES)
def test_case_preconditions_hold_for_the_references(mvr, orc, name):
    case = D.all_cases(mvr)[name]
    n = len(case.pts)
    assert n <= 6001 or not case.brute
    if not case.brute:                              # the 20 000-point chains: the closed form against the oracle (a grid search)
        assert case.finite and set(case.radii) == set(case.closed)
        for tag, r, thr in case.calls():
            keep, lab, ncomp = orc.denoise(case.pts, thr, r)
            assert ncomp == case.closed[tag][0] and np.array_equal(keep, case.closed[tag][1][thr])
        return
    ref = D.reference(case, margins=True)
    partial = False
    for tag, r in case.radii.items():
        label, ncomp, margin = ref[tag]
        print("%s %s: r %.17g, %d components, margin %.2e" % (name, tag, r, ncomp, margin))
        assert tag in case.ties or margin > MIN_MARGIN
        if tag in case.closed:
            assert ncomp == case.closed[tag][0]
            for thr, keep in case.closed[tag][1].items():
                assert np.array_equal(R.select(label, thr), keep)
        if case.finite:
            olab = None
            for thr in case.thresholds + tuple(t for g, t in case.extra if g == tag):
                keep, olab, oncomp = orc.denoise(case.pts, thr, r)
                assert oncomp == ncomp and np.array_equal(keep, expected(case, tag, thr, ref))
            assert np.array_equal(olab, label)
        for thr in case.thresholds:
            keep = R.select(label, thr)
            partial |= 0 < len(keep) < n and len(np.unique(label[keep])) >= 2
    assert all(np.array_equal(np.sort(R.select(ref[tag][0], thr)), np.arange(n)) for tag, thr in case.extra)      # thresholds 0 and -3 keep all
    if case.kind in ("surface", "volume") and name not in D.NO_PARTIAL:
        assert partial
    if not case.finite:                             # the rule: a non-finite point is a component of its own
        bad = np.flatnonzero(~np.isfinite(case.pts[:, :3]).all(1))
        for tag in case.radii:
            label = ref[tag][0]
            assert np.array_equal(label[bad], bad) and not np.isin(label[np.isfinite(case.pts[:, :3]).all(1)], bad).any()
            assert np.isin(bad, R.select(label, 1)).all() and not np.isin(bad, R.select(label, 2)).any()


def test_no_partial_cases_cannot_have_one(mvr):
    """the reasons of denoise_cases.NO_PARTIAL: components only grow with the radius, so the lattice -- singletons just below one
    step, one component at it -- has no radius in between; and fewer than five points cannot be split into two kept components
    and something dropped (the smallest such sizes are 2, 2 and 1)"""
    cases = D.all_cases(mvr)
    assert set(D.NO_PARTIAL) <= set(W.NAMES)
    for name in D.NO_PARTIAL:
        n = len(cases[name].pts)
        if name == "lattice_3d":
            ref = D.reference(cases["lattice_3d_edge"], margins=True)
            assert np.array_equal(cases["lattice_3d_edge"].pts, cases[name].pts) and ref["at"][1] == 1 and ref["below"][1] == n
        else:
            assert n < 5


def test_knife_edges_are_edges(mvr):
    cases = D.all_cases(mvr)
    # the far lattice: every coordinate is an integer held exactly, so the distances are those of the lattice at the origin
    far, g = cases["lattice_far_1e6"].pts[:, :3].astype(np.float64), D.unit_lattice()
    assert np.array_equal(far - far[0], g - g[0]) and np.abs(far).max() < 2 ** 24 and np.abs(far).min() > 5.0e5
    assert np.array_equal(D.reference(cases["lattice_far_1e6"], margins=True)["at"][0], D.reference(cases["lattice_3d_edge"], margins=True)["at"][0])
    # the face-centred half: the nearest distance is sqrt(0.125) to the last bit, and r is that double
    h = cases["lattice_fcc_half"].pts[:, :3].astype(np.float64)
    d = h[1:] - h[0]
    d2 = np.sort(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    assert d2[0] == 0.125 and cases["lattice_fcc_half"].radii["at"] == np.sqrt(0.125)
    # ... while on the full lattice that radius is no edge: the unit steps link everything below it already
    full = R.components(cases["lattice_3d"].pts, [D.below(np.sqrt(0.125))])
    assert next(iter(full.values()))[1] == 1
    for name in ("lattice_3d_edge", "lattice_fcc_half", "grid_midpoints_edge", "lattice_far_1e6", "sheet_64x64_permuted", "bbox_corners_100",
                 "bbox_corners_4096"):
        ref = D.reference(cases[name], margins=True)
        assert ref["at"][2] == 0 and 0 < ref["below"][2] < 1e-15 and ref["at"][1] < ref["below"][1] == len(cases[name].pts)


def test_chains_against_the_brute_force(mvr):
    """the closed form of the chains: every order with and without the cut at 2 000 points, and the permuted cut chain at the full
    20 000 (2e8 pairs, the one brute-force run above the table's 6 001 points)"""
    for order in D.CHAIN_ORDERS:
        pos = D.chain_order(order, D.CHAIN_N)
        assert np.array_equal(np.sort(pos), np.arange(D.CHAIN_N))
        for cut in (None, 700):
            c = D.chain(order, 2000, cut)
            assert c.brute
            label, ncomp, _ = R.components(c.pts, [1.0])[1.0]
            assert ncomp == c.closed["at"][0] == (1 if cut is None else 2)
            for thr, keep in c.closed["at"][1].items():
                assert np.array_equal(R.select(label, thr), keep)
    c = D.all_cases(mvr)["chain_permuted_cut_%d" % D.CHAIN_N]
    label, ncomp, _ = R.components(c.pts, [1.0])[1.0]
    assert ncomp == 2 and len(c.pts) == D.CHAIN_N - 1
    for thr, keep in c.closed["at"][1].items():
        assert np.array_equal(R.select(label, thr), keep)
    assert len(c.closed["at"][1][D.CHAIN_N // 3 + 1]) == D.CHAIN_N - 1 - D.CHAIN_N // 3          # only the longer part


def test_grid_edge_cases_are_what_they_claim(mvr):
    cases = D.all_cases(mvr)
    for name, tag, least in (("clusters_and_a_far_point", "fraction_of_a_cell", 1023), ("clusters_and_a_far_point", "partial", 5.0e5),
                             ("huge_coordinates", "zero_r2", 1.0e30), ("bbox_corners_4096", "at", 4 * 1023)):
        P = cases[name].pts[:, :3].astype(np.float64)               # extent / r above 1023: cells larger than r
        print(name, tag, (P.max(0) - P.min(0)).max() / cases[name].radii[tag])
        assert (P.max(0) - P.min(0)).max() / cases[name].radii[tag] > least
    P = cases["huge_coordinates"].pts[:, :3].astype(np.float64)     # (its cell is set by the point count, not by extent / 512: 47 cells across)
    assert 40 < (P.max(0) - P.min(0)).max() / cases["huge_coordinates"].radii["fraction_of_a_cell"] < 60
    for name in ("planar_sheet", "collinear", "regular_grid_midpoints"):                     # a flat axis
        P = cases[name].pts[:, :3]
        assert (P.max(0) == P.min(0)).any()
    t = cases["duplicated_r_zero"].pts
    assert np.array_equal(t[:3000], t[:2999:-1]) and len(np.unique(t[:3000], axis=0)) == 3000
    for name in W.NAMES:                                     # whole_cloud is beyond the diagonal
        P = cases[name].pts[:, :3].astype(np.float64)
        assert cases[name].radii["whole_cloud"] > np.linalg.norm(P.max(0) - P.min(0))
    assert sorted(len(cases["size_%d" % n].pts) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1025)) == [1, 2, 63, 64, 65, 255, 256, 257, 1025]
    # the far patches are the patch at 0 moved and rounded: not the same cloud, so their own reference decides
    a, b = cases["patch_at_0"].pts, cases["patch_far_1e6"].pts
    assert not np.array_equal((b[:, :3].astype(np.float64) - W.FAR_DIR * 1.0e6).astype(np.float32), a[:, :3])
    w = cases["patch_non_finite_w"]
    assert w.finite and not np.isfinite(w.pts[:, 3]).all() and np.array_equal(w.pts[:, :3], a[:, :3])


def test_the_gpu_test_leaves_nothing_out():
    import test_gpu_denoise_cases as G
    assert G.CASES == D.NAMES and len(G.LEFT_OUT) / len(D.NAMES) == LEFT_OUT_SHARE
