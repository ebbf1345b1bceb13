"""GPU tests of the PFH descriptors (mvr_cloud_pfh; rules P1-P8 in include/mvr_hip.h) against the numpy reference of
tests/pfh_ref.py, and of the matcher and the sample-consensus aligner on rows of 125 floats against tests/align_ref.py.

The descriptor is compared as COUNTS, which the call returns: per query and bin the GPU's c must lie between the reference's sure
counts and the sure counts plus the slack pairs whose candidate set holds the bin (pfh_ref: the pairs f32 arithmetic cannot be
held to their f64 bin); the total of a query between the sure total and that plus its slack pairs; a query without a slack pair
matches bin for bin; no query is excluded.  The signature is compared as BITS with (float)c * (100.0f / (float)m) of the
returned counts.  Order-freedom (P8) is compared as bits between grid resolutions, runs, and the staged and the tiled path.

Measured on an MI355X (profiles/pfh_pytest_gpu.log, this file's own prints): neighbour counts exact on every case; count
differences from the reference's f64 bins, summed over bins, 0 on the view (2 065 446 pairs, 5 707 of them slack), the box, the
view with 72 invalid points, the duplicates, the 384-point ball (all queries on the tiled path) and the patch, and 0 for k = 1,
2, 16 and 64; the same bits at every grid resolution, at pfh_stage 64 / 100 / 256 and 1e5 / 1e6 mm from the origin; on the pair
of tests/test_gpu_align.py the worst displacement of the recovered pose is 2.858 mm from FPFH rows and 3.128 mm from PFH rows."""
import contextlib
import ctypes as C
import importlib

import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
import fpfh_cases as FC
import pfh_cases as PC
import pfh_ref as PR
from conftest import PKG

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


@contextlib.contextmanager
def align_ref_width(dim):
    """align_ref.feature_knn / eligible reshape their tables to align_ref.DIM floats per row"""
    old, AR.DIM = AR.DIM, dim
    try:
        yield AR
    finally:
        AR.DIM = old


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def run(ctx, p, nrm, radius=None, k=None, fma=False, slot=0):
    ctx.upload(slot, p)
    if len(p):
        ctx.upload_normals(slot, nrm)
    f, c, nb = ctx.pfh(slot, radius=radius, k=k, fma=fma, return_counts=True, return_neighbors=True)
    assert f.shape == c.shape == (len(p), 125) and nb.shape == (len(p),) and c.dtype == np.uint32
    return f, c, nb


def values_are_the_scaled_counts(f, c, nb, valid):
    """P5, on every row: the bits of (float)c * (100.0f / (float)m); NaN rows for invalid points and empty neighbourhoods"""
    assert same_bits(f, PR.rows_from_counts(c, nb, valid))
    assert np.isnan(f[~valid]).all() and (nb[~valid] == 0).all() and (c[~valid] == 0).all()
    m = nb.astype(np.int64) * (nb.astype(np.int64) - 1) // 2
    assert (c.sum(1, dtype=np.int64) <= np.maximum(m, 0)).all()


def within_slack(got, ref):
    """the count bounds of the module docstring for the rows ref["queries"]"""
    got = got[ref["queries"]].astype(np.int64)
    sure, maybe, slack = ref["sure"], ref["maybe"], ref["slack"]
    assert (got >= sure).all() and (got <= sure + maybe).all()
    tot, st = got.sum(1), sure.sum(1)
    assert (tot >= st).all() and (tot <= st + slack).all()
    none = slack == 0
    assert np.array_equal(got[none], ref["full"][none])
    return int(np.abs(got - ref["full"]).sum()), int((~none).sum())


_inputs, _refs, _gpu, _stats = {}, {}, {}, {}


def inputs(name, mvr, ctx):
    """(points, normals, radius, reference queries) of a radius case; the normals of a surface are the library's own"""
    if name in _inputs:
        return _inputs[name]
    if name in ("view", "invalid"):
        if "view" not in _inputs:
            p = PC.view(mvr)
            ctx.upload(2, p)
            ctx.estimate_normals(2, radius=PC.VIEW_NORMAL_RADIUS)
            _inputs["view"] = (p, ctx.download_normals(2), PC.VIEW_RADIUS, None)
        if name == "invalid":
            p, nrm, radius, _ = _inputs["view"]
            q, m, bad = PC.with_invalid(p, nrm)
            _inputs["invalid"] = (q, m, radius, None)
    elif name == "box":
        _inputs[name] = PC.box() + (None,)
    elif name == "duplicates":
        _inputs[name] = PC.duplicates() + (None,)
    elif name == "blob":
        _inputs[name] = PC.blob() + (np.array(PC.BLOB_QUERIES),)
    elif name == "patch":
        p = PC.patch(mvr)
        ctx.upload(2, p)
        ctx.estimate_normals(2, radius=PC.patch_normal_radius(p))
        _inputs[name] = (p, ctx.download_normals(2), PC.patch_radius(p), None)
    return _inputs[name]


def reference(name, mvr, ctx, fma=False):
    if (name, fma) not in _refs:
        p, nrm, radius, queries = inputs(name, mvr, ctx)
        _refs[(name, fma)] = PR.pfh(p, nrm, radius=radius, fma=fma, queries=queries)[1]
    return _refs[(name, fma)]


def gpu(name, mvr, ctx, fma=False):
    if (name, fma) not in _gpu:
        p, nrm, radius, _ = inputs(name, mvr, ctx)
        _gpu[(name, fma)] = run(ctx, p, nrm, radius, fma=fma)
        _stats[(name, fma)] = (ctx.stat("pfh_tiled_queries"), ctx.stat("pfh_pairs"))
    return _gpu[(name, fma)]


CASES = ["view", "box", "invalid", "duplicates", "blob", "patch"]


# ------------------------------------------------------------------ counts and values

@pytest.mark.parametrize("name", CASES)
def test_counts_and_values(name, mvr, ctx):
    p, nrm, radius, queries = inputs(name, mvr, ctx)
    f, c, nb = gpu(name, mvr, ctx)
    tiled, pairs = _stats[(name, False)]
    ref = reference(name, mvr, ctx)
    assert np.array_equal(nb[ref["queries"]].astype(np.int64), ref["n"])
    off, with_slack = within_slack(c, ref)
    valid = np.isfinite(p[:, :3]).all(1) & np.isfinite(nrm[:, :3]).all(1)
    values_are_the_scaled_counts(f, c, nb, valid)
    assert (nb[valid] >= 1).all() and np.isfinite(f[valid]).all() and (f[valid] >= 0).all()
    m = nb.astype(np.int64) * (nb.astype(np.int64) - 1) // 2
    assert pairs == m.sum() and tiled == (nb > PC.STAGE).sum()
    print("%s: %d queries (%d compared), %.1f neighbours (max %d), %d invalid, %d on the tiled path; %d pairs, %d slack pairs in %d "
          "queries; count differences from the reference's f64 bins, summed over bins: %d (a pair off its bin gives 2)"
          % (name, len(p), len(ref["queries"]), nb.mean(), nb.max(), int((~valid).sum()), int(tiled), ref["pairs"], int(ref["slack"].sum()),
             with_slack, off))
    if name == "blob":
        # every query, by the sum rule: distinct points and random normals -- f4 > 0, and v = dp x n1 vanishes in f32 only when
        # three rounded products cancel exactly -- so every pair has features and the row's counts add up to m_i
        assert (nb == PC.BLOB_N).all() and tiled == PC.BLOB_N
        assert (c.sum(1, dtype=np.int64) == m).all()
        assert (np.abs(f.astype(F64).sum(1) - 100.0) < 1e-3).all()


def test_fma_distance(mvr, ctx):
    f, c, nb = gpu("duplicates", mvr, ctx, True)
    ref = reference("duplicates", mvr, ctx, True)
    assert np.array_equal(nb.astype(np.int64), ref["n"])
    within_slack(c, ref)
    a = gpu("duplicates", mvr, ctx)
    same = reference("duplicates", mvr, ctx)["n"] == ref["n"]
    print("duplicates: the fma chain changes the neighbour count of %d queries; rows differing among the others: %d"
          % (int((~same).sum()), int((c[same] != a[1][same]).any(1).sum())))


# ------------------------------------------------------------------ P8: nothing depends on an order

@pytest.mark.parametrize("name", ["box", "patch", "blob"])
def test_counts_do_not_depend_on_grid_run_or_path(name, mvr, ctx):
    p, nrm, radius, _ = inputs(name, mvr, ctx)
    base = gpu(name, mvr, ctx)
    again = run(ctx, p, nrm, radius, slot=3)                              # a fresh slot: a new grid over the same points
    assert all(same_bits(x, y) for x, y in zip(base, again))
    ctx.upload(3, p); ctx.upload_normals(3, nrm)
    assert same_bits(ctx.pfh(3, radius=radius), base[0])                 # the optional outputs change nothing
    try:
        for cp in PC.CELL_POINTS:
            ctx.tune(seq_cell_points=cp)
            got = run(ctx, p, nrm, radius, slot=7)
            assert all(same_bits(x, y) for x, y in zip(base, got)), (name, cp)
    finally:
        ctx.tune(seq_cell_points=4)
    try:
        for stage in (64, 100, PC.STAGE):                                 # queries above `stage` neighbours take the tiled path, in tiles of `stage`
            ctx.tune(pfh_stage=stage)
            got = run(ctx, p, nrm, radius, slot=7)
            tiled = int(ctx.stat("pfh_tiled_queries"))
            assert tiled == int((base[2] > stage).sum())
            assert all(same_bits(x, y) for x, y in zip(base, got)), (name, stage)
            print("%s pfh_stage=%d: %d of %d queries on the tiled path, the same bits" % (name, stage, tiled, len(p)))
    finally:
        ctx.tune(pfh_stage=PC.STAGE)


def test_staged_and_tiled_paths_agree_on_one_ball(mvr, ctx):
    """200 points in one ball: staged whole at the default capacity, four tiles at 64, two at 100"""
    p, nrm, radius = PC.blob()
    p, nrm = p[:200], nrm[:200]
    staged = run(ctx, p, nrm, radius, slot=7)
    assert ctx.stat("pfh_tiled_queries") == 0 and (staged[2] == 200).all()
    try:
        for stage in (64, 100, 199, 200):
            ctx.tune(pfh_stage=stage)
            got = run(ctx, p, nrm, radius, slot=7)
            assert ctx.stat("pfh_tiled_queries") == (200 if stage < 200 else 0)
            assert all(same_bits(x, y) for x, y in zip(staged, got)), stage
    finally:
        ctx.tune(pfh_stage=PC.STAGE)
    ref = PR.pfh(p, nrm, radius=radius, queries=np.array([0, 99, 199]))[1]
    within_slack(staged[1], ref)


# ------------------------------------------------------------------ k mode

@pytest.mark.parametrize("k", PC.KS)
def test_k_mode(k, mvr, ctx):
    p, nrm = PC.knn_cloud()
    f, c, nb = run(ctx, p, nrm, k=k, slot=4)
    idx, d2 = ctx.knn(4, 4, k)
    ref = PR.counts(p, nrm, PR.hoods_knn(p, nrm, idx, d2))                # radius mode's arithmetic on the library's own lists
    assert np.array_equal(nb.astype(np.int64), ref["n"])
    off, with_slack = within_slack(c, ref)
    valid = np.isfinite(p[:, :3]).all(1) & np.isfinite(nrm[:, :3]).all(1)
    values_are_the_scaled_counts(f, c, nb, valid)
    assert np.isnan(f[nb == 0]).all() and (f[nb == 1] == 0).all() and np.isfinite(f[nb >= 1]).all()
    assert (nb <= k).all() and ctx.stat("pfh_tiled_queries") == 0
    print("k=%d: %d queries, n_i == 0: %d (%d of them valid points), n_i == 1: %d; %d pairs, %d slack; differences from the f64 bins: %d"
          % (k, len(p), int((nb == 0).sum()), int(((nb == 0) & valid).sum()), int((nb == 1).sum()), ref["pairs"], int(ref["slack"].sum()), off))
    if k == 1:
        assert ((nb == 0) & valid).sum() == 10                            # the copies of point 0, which list point 0 alone
    again = run(ctx, p, nrm, k=k, slot=3)
    assert all(same_bits(x, y) for x, y in zip((f, c, nb), again))


@pytest.mark.parametrize("k", [16, 64])
def test_k_mode_on_a_cloud_smaller_than_k(k, mvr, ctx):
    for n in FC.TINY_SIZES:
        p, nrm, _ = PC.tiny(n)
        f, c, nb = run(ctx, p, nrm, k=k, slot=4)
        if n == 0:
            continue
        assert (nb == n).all()
        ref = PR.counts(p, nrm, PR.hoods_knn(p, nrm, *PR.knn_lists(p, k)))
        within_slack(c, ref)
        values_are_the_scaled_counts(f, c, nb, np.ones(n, bool))
        r = run(ctx, p, nrm, radius=100.0, slot=4)                        # the same neighbourhoods by radius
        assert all(same_bits(x, y) for x, y in zip((f, c, nb), r))


# ------------------------------------------------------------------ small clouds, invalid points, far frames

def test_small_clouds(mvr, ctx):
    for n in FC.TINY_SIZES:
        p, nrm, radius = PC.tiny(n)
        f, c, nb = run(ctx, p, nrm, radius, slot=4)
        assert (nb == 1).all() and (f == 0).all() and (c == 0).all()      # every point alone: n_i = 1, 125 zeros
    p, nrm, radius = PC.tiny(5)
    f, c, nb = run(ctx, p, nrm, 2.5, slot=4)
    assert list(nb) == [2, 3, 3, 3, 2]
    within_slack(c, PR.pfh(p, nrm, radius=2.5)[1])
    nrm[2, 1] = np.nan                                                    # a point with a NaN normal is nobody's neighbour
    f, c, nb = run(ctx, p, nrm, 2.5, slot=4)
    assert list(nb) == [2, 2, 0, 2, 2] and np.isnan(f[2]).all() and np.isfinite(np.delete(f, 2, 0)).all()


def test_invalid_points_are_as_if_removed(mvr, ctx):
    p, nrm, radius, _ = inputs("invalid", mvr, ctx)
    f, c, nb = gpu("invalid", mvr, ctx)
    valid = np.isfinite(p[:, :3]).all(1) & np.isfinite(nrm[:, :3]).all(1)
    assert (~valid).sum() > 20 and np.isnan(f[~valid]).all() and (nb[~valid] == 0).all()
    g = run(ctx, p[valid], nrm[valid], radius, slot=5)
    assert same_bits(g[0], f[valid]) and np.array_equal(g[1], c[valid]) and np.array_equal(g[2], nb[valid])


@pytest.mark.parametrize("far", PC.PATCH_FARS)
def test_far_frames(far, mvr, ctx):
    p, nrm, radius, _ = inputs("patch", mvr, ctx)
    base = gpu("patch", mvr, ctx)
    q = PC.patch_moved(p, far)                                            # every coordinate an exact translation
    got = run(ctx, q, nrm, radius, slot=5)
    assert all(same_bits(x, y) for x, y in zip(base, got))
    print("patch %g mm from the origin: %d rows, the bits of the patch at the origin" % (far, len(q)))


# ------------------------------------------------------------------ P6, P7

def raw(mvr, ctx, slot, radius, k, out, cnt, nb, fma=0):
    prm = mvr.PfhParams(radius, k, fma)
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    return mvr._lib.mvr_cloud_pfh(ctx._h, slot, C.byref(prm), ptr(out, C.c_float), ptr(cnt, C.c_uint32), ptr(nb, C.c_uint32))


def test_refusals_on_the_device(mvr, ctx):
    p, nrm, radius = PC.tiny(5)
    ctx.upload(5, p)                                                       # a new upload drops the normals
    out, cnt, nb = np.full((5, 125), 9.0, F32), np.full((5, 125), 9, np.uint32), np.full(5, 9, np.uint32)
    untouched = lambda: (out == 9.0).all() and (cnt == 9).all() and (nb == 9).all()
    assert raw(mvr, ctx, 5, 2.5, 0, out, cnt, nb) == mvr.E_ARG and untouched()
    assert raw(mvr, ctx, 5, 0.0, 3, out, cnt, nb) == mvr.E_ARG and untouched()
    with pytest.raises(mvr.MvrError):
        ctx.pfh(5, radius=2.5)
    ctx.upload_normals(5, nrm)
    for r, k in ((0.0, 0), (2.5, 3), (-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, -1), (0.0, 65)):
        assert raw(mvr, ctx, 5, r, k, out, cnt, nb) == mvr.E_ARG and untouched(), (r, k)
    assert raw(mvr, ctx, mvr.MAX_SLOTS, 2.5, 0, out, cnt, nb) == mvr.E_ARG and untouched()
    assert raw(mvr, ctx, 5, 2.5, 0, None, None, None) == mvr.OK            # all outputs NULL: the work, no copy
    assert raw(mvr, ctx, 5, 0.0, 3, None, None, None) == mvr.OK
    ctx.upload(5, p[:0])
    assert ctx.pfh(5, radius=2.5).shape == (0, 125) and ctx.pfh(5, k=8).shape == (0, 125)      # an empty cloud is MVR_OK
    p, nrm, radius = FC.box(500)
    ctx.upload(5, p); ctx.upload_normals(5, nrm)
    ctx.pfh(5, radius=radius); ctx.pfh(5, k=16)
    assert same_bits(p, ctx.download(5)) and same_bits(nrm, ctx.download_normals(5))      # the slot is not modified


def test_a_neighbourhood_above_65535_points_is_refused(mvr, ctx):
    """P6: 65 536 copies of one point plus one more, n_i = 65 537 for every query"""
    n = 65537
    p = np.tile(np.array([1.0, 2.0, 900.0, 1.0], F32), (n, 1))
    nrm = np.tile(np.array([0.0, 0.0, 1.0, 0.0], F32), (n, 1))
    ctx.upload(6, p); ctx.upload_normals(6, nrm)
    out, nb = np.full((n, 125), 9.0, F32), np.full(n, 9, np.uint32)
    assert raw(mvr, ctx, 6, 0.5, 0, out, None, nb) == mvr.E_ARG
    assert (out == 9.0).all() and (nb == 9).all()
    ctx.upload(6, p[:300]); ctx.upload_normals(6, nrm[:300])              # within the range: every pair at f4 == 0
    f, c, nb = ctx.pfh(6, radius=0.5, return_counts=True, return_neighbors=True)
    assert (nb == 300).all() and (c == 0).all() and (f == 0).all() and ctx.stat("pfh_tiled_queries") == 300
    ctx.upload(6, p[:0])


# ------------------------------------------------------------------ the matcher at 125 floats per row

def same_table(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))


def wide_rows(rng, n):
    """rows like PFH signatures: most of the mass in few of the 125 bins, real-valued"""
    return (rng.uniform(0, 100, (n, 125)) * rng.uniform(0, 1, (n, 125)) ** 6).astype(F32)


def ref_knn(q, t, k):
    with align_ref_width(125) as A:
        return A.feature_knn(q, t, k)


@pytest.mark.parametrize("k", AC.KNN_KS)
def test_matcher_on_random_rows(k, ctx):
    rng = np.random.default_rng(100 + k)
    q, t = wide_rows(rng, 300), wide_rows(rng, 1000)
    same_table(ctx.feature_knn(q, t, k), ref_knn(q, t, k))


def test_matcher_on_pfh_rows_nan_rows_and_short_targets(mvr, ctx):
    f = gpu("box", mvr, ctx)[0]
    q, t = f[:700], f[700:]
    for k in (1, 2, 5):
        same_table(ctx.feature_knn(q, t, k), ref_knn(q, t, k))
    g = gpu("invalid", mvr, ctx)[0]                                       # NaN rows on both sides
    q, t = g[:600], g[600:3000]
    assert np.isnan(q).any() and np.isnan(t).any()
    idx, d2 = ctx.feature_knn(q, t, 3)
    same_table((idx, d2), ref_knn(q, t, 3))
    assert (idx[np.isnan(q).any(1)] == AR.NONE).all()
    rng = np.random.default_rng(5)
    q = wide_rows(rng, 40)
    for nt in AC.KNN_TAILS:                                               # nt < k and around a tile
        t = wide_rows(rng, nt)
        same_table(ctx.feature_knn(q, t, 64), ref_knn(q, t, 64))
    idx, d2 = ctx.feature_knn(q, q[:0], 4)
    assert (idx == AR.NONE).all() and np.isinf(d2).all()


def test_matcher_does_not_depend_on_the_split(ctx):
    rng = np.random.default_rng(9)
    nq, nt = AC.KNN_SPLIT_SHAPE
    q, t = wide_rows(rng, nq), wide_rows(rng, nt)
    want = ref_knn(q, t, 9)
    try:
        for split in (0,) + AC.KNN_SPLITS:
            ctx.tune(feat_split=split)
            same_table(ctx.feature_knn(q, t, 9), want)
    finally:
        ctx.tune(feat_split=0)


def test_matcher_refuses_other_widths(mvr, ctx):
    for dim in (32, 34, 124, 126, 128):
        rows = np.ones((4, dim), F32)
        with pytest.raises(mvr.MvrError):
            ctx.feature_knn(rows, rows, 1)


# ------------------------------------------------------------------ the aligner on PFH rows

S, T_ = 10, 11
ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_align.py:27


def wide_pair():
    """align_cases.align_pair with its 33 rounded random features repeated to 125: the same twins, the same noise"""
    s, t, sf, tf = AC.align_pair()
    widen = lambda a: np.ascontiguousarray(np.concatenate([a, a, a, a], 1)[:, :125] + np.arange(125, dtype=F32)[None, :] * F32(0.25))
    return s, t, widen(sf), widen(tf)


def test_aligner_trace_equals_the_replay_on_wide_rows(ctx):
    s, t, sf, tf = wide_pair()
    ctx.upload(S, s); ctx.upload(T_, t)
    a = dict(max_iterations=AC.ALIGN_ITERS, nr_samples=3, k=AC.ALIGN_K, similarity=AC.ALIGN_SIMILARITY, max_dist=AC.ALIGN_MAX_DIST,
             inlier_fraction=AC.ALIGN_FRACTION, seed=AC.ALIGN_SEED)
    res, tr = ctx.align_prerejective(S, T_, sf, tf, return_trace=True, **a)
    with align_ref_width(125) as A:
        el = A.eligible(s, sf)
        want = A.feature_knn(sf[el], tf, a["k"])
    idx, d2 = ctx.feature_knn(sf[el], tf, a["k"])
    same_table((idx, d2), want)
    st, src, tgt = AR.replay(s, t, el, idx, a["max_iterations"], 3, a["seed"], a["similarity"])
    assert np.array_equal(tr["status"], st) and np.array_equal(tr["src"], src) and np.array_equal(tr["tgt"], tgt)
    assert res["rejected"] == int((st == 0).sum()) and res["scored"] == int((st == 1).sum()) and (st == 1).any() and (st == 0).any()
    scored = np.nonzero(st == 1)[0]
    T = tr["T"][scored]
    inl, err = ctx.pose_scores(S, T_, T, a["max_dist"])                   # the scores: the library's own rule S on the traced poses
    assert np.array_equal(tr["inliers"][scored], inl) and np.array_equal(tr["error"][scored].view(np.uint64), err.view(np.uint64))
    for i in scored[:40]:
        K, sv = AR.kabsch(s[src[i], :3], t[tgt[i], :3])
        assert np.abs(tr["T"][i][:3, :3] - K[:3, :3]).max() <= ROT_TOL and np.abs(tr["T"][i][:3, 3] - K[:3, 3]).max() <= TRANS_TOL, (i, sv)
    conv, best = AR.select(st, tr["inliers"], tr["error"], len(s), a["inlier_fraction"])
    assert res["converged"] == conv and res["best_iteration"] == best and conv
    assert same_bits(res["T"], tr["T"][best]) and res["inliers"] == tr["inliers"][best] and res["error"] == tr["error"][best]
    x = s[:, :3].astype(F64) @ res["T"][:3, :3].astype(F64).T + res["T"][:3, 3].astype(F64)
    y = s[:, :3].astype(F64) @ AC.ALIGN_POSE[:3, :3].astype(F64).T + AC.ALIGN_POSE[:3, 3].astype(F64)
    assert np.linalg.norm(x - y, axis=1).max() < AC.ALIGN_MAX_DIST
    # tables of two widths, of a width that is neither, or not one row per point
    for bad_s, bad_t in ((sf, tf[:, :33]), (sf[:, :34], tf[:, :34]), (sf[:-1], tf), (sf.reshape(-1), tf)):
        with pytest.raises(ValueError):
            ctx.align_prerejective(S, T_, bad_s, bad_t, **a)


def test_wrapper_on_33_wide_rows_returns_what_the_old_entry_returns(mvr, ctx):
    s, t, sf, tf = AC.align_pair()
    ctx.upload(S, s); ctx.upload(T_, t)
    a = dict(max_iterations=AC.ALIGN_ITERS, nr_samples=3, k=AC.ALIGN_K, similarity=AC.ALIGN_SIMILARITY, max_dist=AC.ALIGN_MAX_DIST,
             inlier_fraction=AC.ALIGN_FRACTION, seed=AC.ALIGN_SEED)
    res, tr = ctx.align_prerejective(S, T_, sf, tf, return_trace=True, **a)
    prm = mvr.PrerejParams(a["max_iterations"], 3, a["k"], a["similarity"], a["max_dist"], a["inlier_fraction"], a["seed"], 0)
    old, old_tr = mvr.PrerejResult(), (mvr.PrerejTrace * a["max_iterations"])()
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    assert mvr._lib.mvr_align_prerejective(ctx._h, S, T_, fp(sf), fp(tf), C.byref(prm), None, C.byref(old), old_tr) == mvr.OK
    assert (old.converged, old.best_iteration, old.inliers, old.rejected, old.scored) == \
        (int(res["converged"]), res["best_iteration"], res["inliers"], res["rejected"], res["scored"])
    assert old.error == res["error"] and same_bits(mvr.from_cm(np.array(old.T, F32)), res["T"])
    assert [e.status for e in old_tr] == list(tr["status"]) and [e.inliers for e in old_tr] == list(tr["inliers"])
    assert all(list(e.tgt)[:3] == list(tr["tgt"][i]) for i, e in enumerate(old_tr))


def test_pose_error_with_pfh_beside_fpfh(mvr, ctx):
    """the synthetic pair tests/test_gpu_align.py recovers a pose on, aligned from FPFH and from PFH rows at the same settings: the
    two figures are reported, neither is held to the other; the first iterations of the PFH run are replayed"""
    s_raw, t_raw = AC.recovery_view(mvr)
    inv = np.linalg.inv(AC.REC_POSE.astype(F64))
    rows = {}
    for slot, raw_pts in ((20, s_raw), (21, t_raw)):
        ctx.upload(slot, raw_pts)
        ctx.voxel_grid(slot, slot, AC.REC_LEAF)
        ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS)
        rows[slot] = (ctx.download(slot), ctx.fpfh(slot, AC.REC_FPFH_RADIUS), ctx.pfh(slot, radius=AC.REC_FPFH_RADIUS))
    (s, sf33, sf125), (t, tf33, tf125) = rows[20], rows[21]
    y = s[:, :3].astype(F64) @ inv[:3, :3].T + inv[:3, 3]
    for name, sf, tf in (("FPFH", sf33, tf33), ("PFH", sf125, tf125)):
        res, tr = ctx.align_prerejective(20, 21, sf, tf, return_trace=True, **AC.REC_PARAMS)
        x = s[:, :3].astype(F64) @ res["T"][:3, :3].astype(F64).T + res["T"][:3, 3].astype(F64)
        print("%s: %d / %d points, converged %d at iteration %d, %d inliers, error %.4f, rejected %d, scored %d, worst displacement "
              "%.3f mm; matching %.1f ms, hypotheses %.1f ms, scoring %.1f ms"
              % (name, len(s), len(t), res["converged"], res["best_iteration"], res["inliers"], res["error"], res["rejected"], res["scored"],
                 float(np.linalg.norm(x - y, axis=1).max()), ctx.stat("prerej_match_ms"), ctx.stat("prerej_hypotheses_ms"),
                 ctx.stat("prerej_score_ms")))
    with align_ref_width(125) as A:
        el = A.eligible(s, sf125)
    idx, d2 = ctx.feature_knn(sf125[el], tf125, AC.REC_PARAMS["k"])
    same_table((idx, d2), ref_knn(sf125[el], tf125, AC.REC_PARAMS["k"]))
    m = 300
    st, src, tgt = AR.replay(s, t, el, idx, m, 3, AC.REC_PARAMS["seed"], AC.REC_PARAMS["similarity"])
    assert np.array_equal(tr["status"][:m], st) and np.array_equal(tr["src"][:m], src) and np.array_equal(tr["tgt"][:m], tgt)
