"""The preconditions that tests/walk_cases.py states for the cases of tests/test_gpu_walk_fuzz.py, checked on the numpy
references alone (no GPU): the share of points the eigen-gap rule excludes stays within each case's cap, the statistical
filter's gap to the threshold is at least 1e-9 wherever inlier sets are compared, the far-frame patch really has the ties it
is there for, and the reference's normal on the line is orthogonal to it."""
import importlib

import numpy as np
import pytest

import normals_ref as N
import outlier_ref as O
import walk_cases as W
from conftest import PKG

MIN_GAP = 1e-9          # tests/test_gpu_outlier.py


@pytest.fixture(scope="module")
def mvr():
    return importlib.import_module(PKG)          # the scan generator is host code


def excluded_share(ref, w):
    ok = ~np.isnan(ref[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    return float((ok & ~(gap >= 1e-4)).sum()) / max(int(ok.sum()), 1), ok


@pytest.mark.parametrize("name", W.NAMES)
def test_case_preconditions_hold_for_the_reference(mvr, name):
    q, t = W.get(name, mvr)
    kind, cap, no_sets = W.TABLE[name]
    idx, d2 = N.knn_brute(t, t, 64)
    if cap is not None:
        ref, rc, w = N.normals_from_lists(t, idx[:, :16])
        ex_k, ok = excluded_share(ref, w)
        ref_r, rc_r, w_r = N.normals_from_sets(t, *N.radius_sets(t, W.radii(name, t)["several_cells"]))
        ex_r, _ = excluded_share(ref_r, w_r)
        print("%s: excluded share %.4f (k = 16), %.4f (radius), cap %g" % (name, ex_k, ex_r, cap))
        assert ex_k <= cap and ex_r <= cap
    for k in W.MEAN_KS:
        r = O.statistical(t, k, 1.0)
        print("%s: mean_k %d gap %.1e" % (name, k, r["gap"]))
        assert r["gap"] >= MIN_GAP or k in no_sets
    if kind == "line":
        ref, rc, w = N.normals_from_lists(t, idx[:, :16])
        assert np.abs(ref[:, 0]).max() == 0          # what the docstring of the GPU test quotes
    if name == "patch_far_1e6":
        assert (d2[:, 15] == d2[:, 16]).mean() > 0.01 and (d2[:, 1] == 0).mean() > 0.001
    if name in ("patch_at_0", "patch_far_1e5"):
        assert (d2[:, 15] == d2[:, 16]).sum() == 0 and (d2[:, 1] == 0).sum() == 0
    if name == "lattice_3d":
        assert (d2[:, 1:7] == np.float32(W.LATTICE_STEP ** 2)).all(1).any() and (d2[:, 26] == np.float32(3 * W.LATTICE_STEP ** 2)).any()
