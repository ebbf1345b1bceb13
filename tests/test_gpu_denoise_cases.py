"""mvr_cloud_denoise (csrc/mvr_denoise.hip) on the case table of tests/denoise_cases.py, against the brute-force reference of
tests/denoise_ref.py and the table's closed forms: for every (case, radius, threshold) the kept indices in order, n_components,
n_kept, the downloaded cloud bit for bit and kept_index.  Nothing here has a tolerance.  The non-finite cases are judged by the
rule of include/mvr_hip.h alone (the oracle is never handed such a cloud).  tests/test_denoise_cases_host.py proves the table's
preconditions on the references; DESIGN.md 24 has the table and what the run showed."""
import importlib

import numpy as np
import pytest

import denoise_cases as D
import denoise_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

CASES = list(D.NAMES)
LEFT_OUT = []                 # tests/test_denoise_cases_host.py asserts it stays empty
SLOT, FRESH = 40, 41


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)          # one context: denoise does not depend on the NN kernel variant
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(ctx, pts, thr, r, nrm=None):
    """one call on a fresh upload: (kept_index, n_components, downloaded cloud, downloaded normals or None)"""
    ctx.upload(SLOT, pts)
    if nrm is not None:
        ctx.upload_normals(SLOT, nrm)
    keep, ncomp = ctx.denoise(SLOT, thr, r)
    assert ctx.size(SLOT) == len(keep)                                      # n_kept, and the slot's new size
    return keep, ncomp, ctx.download(SLOT), ctx.download_normals(SLOT) if nrm is not None else None


def expected(case, tag, thr):
    """(kept indices in output order, n_components): the closed form where the table has one, else the brute force"""
    if tag in case.closed and thr in case.closed[tag][1]:
        return np.asarray(case.closed[tag][1][thr], np.uint32), case.closed[tag][0]
    assert case.brute
    label, ncomp, _ = D.reference(case)[tag]
    return R.select(label, thr), ncomp


def normals_for(pts):
    """a normal per point that names its point: (index, -index, 0.5, 0), exact in f32"""
    n = len(pts)
    return np.stack([np.arange(n), -np.arange(n), np.full(n, 0.5), np.zeros(n)], 1).astype(np.float32)


@pytest.mark.parametrize("name", CASES)
def test_denoise_case(ctx, mvr, name):
    case = D.all_cases(mvr)[name]
    pts = case.pts
    for tag, r, thr in case.calls():
        okeep, oncomp = expected(case, tag, thr)
        for rep in range(2 if case.twice else 1):
            keep, ncomp, out, _ = run(ctx, pts, thr, r)
            what = "%s %s r=%.17g threshold=%d run %d" % (name, tag, r, thr, rep)
            assert ncomp == oncomp, what
            assert len(keep) == len(okeep), what
            assert np.array_equal(keep, okeep), what
            assert np.array_equal(bits(out), bits(pts[okeep])), what


@pytest.mark.parametrize("name", ["patch_at_0", "pairs_3000", "patch_sprinkled_one", "nan_between_components", "size_2"])
def test_normals_follow_their_points(ctx, mvr, name):
    case = D.all_cases(mvr)[name]
    nrm = normals_for(case.pts)
    sizes = set()
    for tag, r, thr in case.calls():
        okeep, oncomp = expected(case, tag, thr)
        keep, ncomp, out, onrm = run(ctx, case.pts, thr, r, nrm)
        assert ncomp == oncomp and np.array_equal(keep, okeep)
        assert np.array_equal(bits(out), bits(case.pts[okeep]))
        assert onrm.shape == (len(okeep), 4) and np.array_equal(bits(onrm), bits(nrm[okeep]))
        sizes.add(len(okeep))
    assert 0 in sizes and len(case.pts) in sizes          # a call that keeps nothing (threshold n + 1) and one that keeps all


def test_refusals_change_nothing(ctx, mvr):
    case = D.all_cases(mvr)["size_257"]
    ctx.upload(SLOT, case.pts)
    for slot, thr, r in ((SLOT, 2, float("nan")), (SLOT, 2, -1.0), (SLOT, 2, -float("inf")), (-1, 2, 1.0), (mvr.MAX_SLOTS, 2, 1.0)):
        with pytest.raises(mvr.MvrError) as e:
            ctx.denoise(slot, thr, r)
        assert e.value.status == mvr.E_ARG
        assert np.array_equal(bits(ctx.download(SLOT)), bits(case.pts))
    okeep, oncomp = expected(case, "fraction_of_a_cell", 2)                      # and the slot still works
    keep, ncomp = ctx.denoise(SLOT, 2, case.radii["fraction_of_a_cell"])
    assert ncomp == oncomp and np.array_equal(keep, okeep)


@pytest.mark.parametrize("name", ["patch_sprinkled_all", "lattice_sprinkled_one", "equal_inf_points"])
def test_knn_after_non_finite_input(ctx, mvr, name):
    """the slot is a new point set after the call: it answers mvr_knn like a fresh upload of the same points"""
    case = D.all_cases(mvr)[name]
    tag = next(iter(case.radii))
    for thr in (1, 2):
        okeep, _ = expected(case, tag, thr)
        ctx.upload(SLOT, case.pts)
        ctx.knn(SLOT, SLOT, 9)                                                   # an ordering and a grid of the OLD point set
        keep, _ = ctx.denoise(SLOT, thr, case.radii[tag])
        assert np.array_equal(keep, okeep)
        ctx.upload(FRESH, case.pts[okeep])
        for k in (1, 9):
            idx, d2 = ctx.knn(SLOT, SLOT, k)
            fidx, fd2 = ctx.knn(FRESH, FRESH, k)
            assert np.array_equal(idx, fidx) and np.array_equal(bits(d2), bits(fd2))
            assert len(idx) == len(okeep)
