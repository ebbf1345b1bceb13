"""GPU tests of the exact k-NN in feature space (mvr_feature_knn; rules M1-M3 in include/mvr_hip.h) against the numpy reference
of tests/align_ref.py: indices and squared distances bit for bit, every query and every entry, nothing excluded.

The tables of align_cases.features() hold multiples of 4: they are rich in ties and blind to the order and the rounding of M1's
sum (tests/test_align_host.py asserts it).  The tables of align_cases.KNN_REAL are real-valued: there the same host test shows
that an fma chain, four accumulators, the reverse order, a tree or an f64 accumulator change the d2 bits of 32-73 % of the pairs,
and on the twins the index of the nearest row of 57-152 of 300 queries.

NOT measured on a GPU when the real-valued cases were written: no device could be had.  They were run once against a stand-in
context whose k-NN is the numpy reference, so they are known to hold for a correct implementation."""
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


# ------------------------------------------------------------------ real-valued rows: the order and the rounding of M1 show

@pytest.mark.parametrize("k", AC.KNN_KS)
@pytest.mark.parametrize("name", AC.KNN_REAL)
def test_real_valued_lists_match_the_reference(name, k, ctx):
    q, t, want = reference(name, k)
    got = ctx.feature_knn(q, t, k)
    assert same(got, want)
    if name == "range":
        assert (got[0][40, :min(k, 10)] != R.NONE).all() and (got[0][40, 10:] == R.NONE).all() and np.isinf(got[1][40, 10:]).all()
        if k >= 2:
            assert (bits(got[1][50:130, :2]) == 0).all() and (got[0][50:130, 0] < got[0][50:130, 1]).all()
    if name == "key_zero":
        assert got[0][0, 0] == 0 and bits(got[1])[0, 0] == 0             # the key (d2 = +0.0, row 0) is the integer 0, and it is listed
        assert list(got[0][0, :6]) == [0, 1, 2, 3, 4, 5][:k] and (bits(got[1][0, :6]) == 0).all()


@pytest.mark.parametrize("nq", AC.KNN_EDGE_NQ)
def test_real_valued_rows_at_the_launch_edges(nq, ctx):
    """one query, one short of a block of 256, a block, one past it; one row, one short of a tile of 64, a tile, one past it,
    and the same around four tiles"""
    for nt in AC.KNN_EDGE_NT:
        q, t = AC.knn_real(seed=100 + nt, nq=nq, nt=nt)
        ref = R.feature_knn(q, t, 64)
        for k in (1, 10, 33, 64):
            assert same(ctx.feature_knn(q, t, k), (ref[0][:, :k], ref[1][:, :k])), (nq, nt, k)
        assert (ref[0][:, min(nt, 64):] == R.NONE).all() and (ref[0][:, :min(nt, 64)] != R.NONE).all()


def rows_per_split(nt, split):
    """feature_knn_device's arithmetic for feat_split > 0: the rows of a split are a whole number of tiles"""
    rows = -(-nt // min(split, 64))
    return max(-(-rows // AC.FEAT_TILE) * AC.FEAT_TILE, AC.FEAT_TILE)


@pytest.mark.parametrize("name", ["real", "twins"])
def test_every_split_gives_the_same_bits_on_real_valued_rows(name, ctx):
    """257 x 4 161: one query past a block, 66 tiles.  The partial lists of the splits are merged under the same total order, so
    the bits are the reference's at every split -- also for the twins whose two rows fall into different splits: the first
    twins sit at the rows 64 m - 1 (align_cases.twin_rows), and a split ends at a multiple of rows_per_split(), itself a
    multiple of 64; the count below is taken from the rows the case reports, for every split"""
    nq, nt = AC.KNN_SPLIT_SHAPE
    q, t = getattr(AC, "knn_" + name)(nq=nq, nt=nt)
    ref = R.feature_knn(q, t, 64)
    if name == "twins":
        first = AC.twin_first_rows(nq=nq, nt=nt)
        assert np.array_equal(np.sort(ref[0][:, :2], axis=1), np.stack([first, first + 1], 1))
    try:
        for split in (0,) + AC.KNN_SPLITS:
            ctx.tune(feat_split=split)
            for k in (1, 10, 33, 64):
                assert same(ctx.feature_knn(q, t, k), (ref[0][:, :k], ref[1][:, :k])), (split, k)
            if name == "twins" and split > 1:
                rows = rows_per_split(nt, split)
                across = int(((first + 1) % rows == 0).sum())
                print("feat_split %d: %d rows per split, %d twin pairs straddle a split boundary" % (split, rows, across))
                if split == 7:
                    assert rows == 640 and across >= 1
    finally:
        ctx.tune(feat_split=0)


# ------------------------------------------------------------------ short targets, empty sides, splits

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
