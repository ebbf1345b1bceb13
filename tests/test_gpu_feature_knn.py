"""GPU tests of the exact k-NN in feature space (mvr_feature_knn; rules M1-M3 in include/mvr_hip.h) against the numpy reference
of tests/align_ref.py: indices and squared distances bit for bit, every query and every entry, nothing excluded."""
import importlib

import numpy as np
import pytest

import align_cases as AC
import align_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

F32 = np.float32


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


def same(got, want):
    gi, gd = got
    wi, wd = want
    return gi.shape == wi.shape and gd.shape == wd.shape and np.array_equal(gi, wi) and np.array_equal(bits(gd), bits(wd))


_ref = {}


def reference(name, k):
    """the reference of a case at k = 64, computed once; a smaller k is its leading columns (the order is total)"""
    if name not in _ref:
        q, t = getattr(AC, "knn_" + name)()
        _ref[name] = (q, t) + R.feature_knn(q, t, 64)
    q, t, idx, d2 = _ref[name]
    return q, t, (idx[:, :k], d2[:, :k])


@pytest.mark.parametrize("k", AC.KNN_KS)
@pytest.mark.parametrize("name", ["plain", "duplicates", "non_finite"])
def test_lists_match_the_reference(name, k, ctx):
    q, t, want = reference(name, k)
    got = ctx.feature_knn(q, t, k)
    assert same(got, want)
    if name == "duplicates":
        assert (k == 1 or (np.diff(want[1], axis=1) == 0).any()) and (want[1][:, 0] == 0).sum() >= len(q) // 10      # ties, and d2 = 0
    if name == "non_finite":
        badq = ~np.isfinite(q).all(1)
        assert badq.any() and (got[0][badq] == R.NONE).all() and np.isinf(got[1][badq]).all()


@pytest.mark.parametrize("nt", AC.KNN_TAILS)
def test_tails_of_short_targets(nt, ctx):
    q, t = AC.knn_non_finite(nq=130, nt=nt) if nt > 1 else AC.knn_plain(nq=130, nt=1)
    want = R.feature_knn(q, t, 64)
    got = ctx.feature_knn(q, t, 64)
    assert same(got, want)
    live = int(np.isfinite(t).all(1).sum())
    assert (got[0][:, min(live, 64):] == R.NONE).all()


def test_one_query_and_no_rows(ctx):
    q, t = AC.knn_duplicates(nq=1)
    for k in (1, 10, 64):
        assert same(ctx.feature_knn(q, t, k), R.feature_knn(q, t, k))
    idx, d2 = ctx.feature_knn(q, t[:0], 3)
    assert (idx == R.NONE).all() and np.isinf(d2).all()
    idx, d2 = ctx.feature_knn(q[:0], t, 3)
    assert idx.shape == (0, 3) and d2.shape == (0, 3)


def test_every_split_gives_the_same_bits(ctx):
    q, t, want = reference("non_finite", 10)
    try:
        for split in AC.KNN_SPLITS:
            ctx.tune(feat_split=split)
            assert same(ctx.feature_knn(q, t, 10), want), split
            assert same(ctx.feature_knn(q, t, 64), reference("non_finite", 64)[2]), split
    finally:
        ctx.tune(feat_split=0)


def test_target_split_and_merge_at_5000_by_20000(ctx):
    """20 blocks of queries: the automatic split deals the target to blocks as well; rows repeat (4 000 distinct ones), so equal
    d2 meet across splits"""
    nq, nt = AC.KNN_BIG
    rng = np.random.default_rng(8)
    base = AC.features(rng, 4000)
    t = base[rng.integers(0, len(base), nt)]
    q = AC.features(rng, nq)
    q[::7] = base[rng.integers(0, len(base), len(q[::7]))]
    want = R.feature_knn(q, t, 10)
    got = ctx.feature_knn(q, t, 10)
    assert same(got, want)
    assert (np.diff(want[1], axis=1) == 0).mean() > 0.2
    ctx.tune(feat_split=1)
    try:
        assert same(ctx.feature_knn(q, t, 10), want)
    finally:
        ctx.tune(feat_split=0)
