"""GPU tests of the radius search (mvr_radius_search; rules RS1-RS11 in include/mvr_hip.h) against the numpy reference of
tests/radius_ref.py on the adversarial clouds of tests/walk_cases.py.  Every comparison is exact: offsets, idx and the bits of
d2; sets only where RS5 leaves the order open.  The whole_cloud radius is used where len(q) * len(t) <= 2e6.

RS8 (a total above MVR_RADIUS_MAX_TOTAL) is not run: the refusal needs 2^31 entries.  tests/test_radius_host.py checks the
arithmetic of the bound."""
import ctypes as C
import importlib

import numpy as np
import pytest

import normals_ref as N
import radius_ref as R
import walk_cases as W
from conftest import PKG

pytestmark = pytest.mark.gpu

F32 = np.float32
WHOLE_MAX = 2e6


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


def same(got, ref):
    return np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(bits(got[2]), bits(ref[2]))


def case_radii(name, q, t):
    return {tag: r for tag, r in W.radii(name, t).items() if tag != "whole_cloud" or len(q) * len(t) <= WHOLE_MAX}


_refs = {}


def ref_of(name, side, q, t, tag, r, fma):
    """the uncapped reference of a case, computed once (the capped lists are its rows' prefixes: the order is total)"""
    key = (name, side, tag, bool(fma))
    if key not in _refs:
        _refs[key] = R.radius_search(q, t, r, fma=fma)
    return _refs[key]


def capped(ref, max_nn):
    """the leading max_nn entries of every row of an ordered reference"""
    o, idx, d2 = ref
    o = o.astype(np.int64)
    rank = np.arange(len(idx)) - np.repeat(o[:-1], np.diff(o))
    keep = rank < max_nn
    out = np.zeros(len(o), np.uint64)
    out[1:] = np.cumsum(np.minimum(np.diff(o), max_nn))
    return out, idx[keep], d2[keep]


# ------------------------------------------------------------------ sorted rows on every case

@pytest.mark.parametrize("name", W.NAMES)
def test_sorted_rows_equal_the_reference(ctx, mvr, name):
    """every case, self and cross, fma off and on, every radius of W.radii: offsets, idx and the bits of d2.  On the lattices
    d2 == r2 counts: the row lengths there are also checked against the closed form, independently of the reference"""
    q, t = W.get(name, mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    for side, qs, qq in (("self", 1, t), ("cross", 0, q)):
        for tag, r in case_radii(name, qq, t).items():
            for fma in (False, True):
                got = ctx.radius_search(qs, 1, r, fma=fma)
                assert same(got, ref_of(name, side, qq, t, tag, r, fma)), (name, side, tag, fma)
    if name == "lattice_3d":
        for tag in ("lattice_distance", "lattice_diagonal"):
            o, idx, d2 = ctx.radius_search(1, 1, W.radii(name, t)[tag])
            g = np.stack(np.meshgrid(np.arange(16), np.arange(15), np.arange(14), indexing="ij"), -1).reshape(-1, 3)
            inner = [((g[:, a] > 0) & (g[:, a] < d - 1)).astype(np.int64) for a, d in enumerate((16, 15, 14))]
            # at one step: the point, one neighbour per axis on a face and a second inside: 1 + 3 + (axes the point is inside on)
            want = 3 + sum(inner) + 1
            if tag == "lattice_diagonal":                    # ... plus the in-plane diagonals: per pair of axes (1 + inner_a) * (1 + inner_b)
                want = want + sum((1 + inner[a]) * (1 + inner[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
            assert np.array_equal(np.diff(o.astype(np.int64)), want), tag
            assert (d2 <= F32(W.radii(name, t)[tag] ** 2)).all() and (d2 == F32(W.radii(name, t)[tag] ** 2)).any()


@pytest.mark.parametrize("name", ["patch_at_0", "lattice_3d", "duplicates_41", "every_target_duplicated", "size_257"])
def test_self_rows_are_the_outlier_counts_plus_one(ctx, mvr, name):
    """RS1: the ball of the radius filter: row length = radius_outlier_removal's count + 1 (the point itself)"""
    _, t = W.get(name, mvr)
    ctx.upload(1, t)
    for tag, r in case_radii(name, t, t).items():
        o, total = ctx.radius_search(1, 1, r, count_only=True)
        n, cnt = ctx.radius_outlier_removal(2, 1, r, 0, return_counts=True)
        assert np.array_equal(np.diff(o.astype(np.int64)), cnt.astype(np.int64) + 1) and total == int(o[-1]), (name, tag)


# ------------------------------------------------------------------ sorted = False

@pytest.mark.parametrize("name", ["patch_far_1e6", "all_identical", "lattice_3d", "clusters_and_a_far_point", "size_65"])
def test_unsorted_rows_hold_the_same_multisets_and_repeat(ctx, mvr, name):
    q, t = W.get(name, mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    for tag, r in case_radii(name, q, t).items():
        ref = ref_of(name, "cross", q, t, tag, r, False)
        a = ctx.radius_search(0, 1, r, sorted=False)
        b = ctx.radius_search(0, 1, r, sorted=False)
        assert same(a, b), (name, tag, "two identical calls")
        assert np.array_equal(a[0], ref[0])
        si, sd = R.sort_rows(a[0], a[1], a[2])
        assert np.array_equal(si, ref[1]) and np.array_equal(bits(sd), bits(ref[2])), (name, tag)


# ------------------------------------------------------------------ max_nn

MAX_NNS = (1, 9, 17, 33, 63, 64, 65, 300)


@pytest.mark.parametrize("name", ["patch_far_1e5", "patch_far_1e6", "duplicates_41", "all_identical", "lattice_3d", "exactly_257_and_1025"])
def test_max_nn(ctx, mvr, name):
    """RS4: the smallest max_nn entries in order, whatever `sorted` says; for max_nn <= 64 also the d2 <= r2 prefix of ctx.knn; at
    the whole_cloud radius with max_nn = k the rows ARE ctx.knn's"""
    q, t = W.get(name, mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    for tag, r in case_radii(name, q, t).items():
        r2 = R.clamp_r2(r)
        for fma in (False, True):
            ref = ref_of(name, "cross", q, t, tag, r, fma)
            for mx in MAX_NNS:
                want = capped(ref, mx)
                got = ctx.radius_search(0, 1, r, max_nn=mx, fma=fma, sorted=(mx % 2 == 0))
                assert same(got, want), (name, tag, mx, fma)
                if mx <= 64:
                    ki, kd = ctx.knn(0, 1, mx, fma=fma)
                    inside = (ki != N.NONE) & (kd <= r2)
                    assert np.array_equal(np.diff(got[0].astype(np.int64)), inside.sum(1))
                    assert np.array_equal(got[1], ki[inside]) and np.array_equal(bits(got[2]), bits(kd[inside])), (name, tag, mx, fma)
                    if tag == "whole_cloud" and len(t) >= mx:
                        assert np.array_equal(got[1].reshape(len(q), mx), ki) and np.array_equal(bits(got[2]).reshape(len(q), mx), bits(kd))


# ------------------------------------------------------------------ the stage and the long-row path

def stage_cloud(counts, seed=3):
    """clusters far from each other (1000 apart): cluster c holds counts[c] points within 0.2 of its centre, so at radius 1
    every point of cluster c has exactly counts[c] neighbours"""
    rng = np.random.default_rng(seed)
    pts = [rng.uniform(-0.1, 0.1, (m, 3)) + [1000.0 * c, 0.0, 900.0] for c, m in enumerate(counts)]
    p = W.cloud(np.concatenate(pts))
    return p[rng.permutation(len(p))]


def test_stage_edges(ctx, mvr):
    """radius_stage = 64: rows of exactly 63, 64, 65, 127, 128, 129 and 1025 neighbours; every row equals the reference and
    radius_long_rows is the number of rows above the stage.  Once at the default stage with rows of 1025 just above it.  The same
    arrays at every stage, sorted or capped or neither"""
    counts = (63, 64, 65, 127, 128, 129, 1025)
    p = stage_cloud(counts)
    ctx.upload(0, p)
    ref = R.radius_search(p, p, 1.0)
    lens = np.diff(ref[0].astype(np.int64))
    assert sorted(set(lens)) == sorted(counts) and all((lens == m).sum() == m for m in counts)
    try:
        for stage in (64, 100, 128, mvr.RADIUS_STAGE):
            ctx.tune(radius_stage=stage)
            assert ctx.stat("radius_stage") == stage
            assert same(ctx.radius_search(0, 0, 1.0), ref), stage
            assert ctx.stat("radius_long_rows") == (lens > stage).sum(), stage
            for mx in (1, 64, 65, 200, 2000):
                assert same(ctx.radius_search(0, 0, 1.0, max_nn=mx, sorted=False), capped(ref, mx)), (stage, mx)
            u = ctx.radius_search(0, 0, 1.0, sorted=False)
            assert ctx.stat("radius_long_rows") == (lens > stage).sum()
            si, sd = R.sort_rows(*u)
            assert np.array_equal(u[0], ref[0]) and np.array_equal(si, ref[1]) and np.array_equal(bits(sd), bits(ref[2])), stage
            assert same(u, ctx.radius_search(0, 0, 1.0, sorted=False))
        assert (lens > mvr.RADIUS_STAGE).sum() == 1025                    # the default stage met rows just above it
        for bad in (63, mvr.RADIUS_STAGE + 1):
            with pytest.raises(mvr.MvrError):
                ctx.tune(radius_stage=bad)
    finally:
        ctx.tune(radius_stage=mvr.RADIUS_STAGE)


@pytest.mark.parametrize("name", ["patch_at_0", "duplicates_41", "lattice_3d"])
def test_results_do_not_depend_on_the_stage_or_the_grid_resolution(ctx, mvr, name):
    """RS11: seq_cell_points 1, 4 (the default), 64 and 4096 change the cell edge of every grid built afterwards (the clouds are
    uploaded again after each tune); radius_stage 64 sends the rows above it through the long-row path"""
    q, t = W.get(name, mvr)
    r = W.radii(name, t)["several_cells"]
    ref = ref_of(name, "cross", q, t, "several_cells", r, False)
    try:
        for cp in (4, 1, 64, 4096):
            for stage in (mvr.RADIUS_STAGE, 64):
                ctx.tune(seq_cell_points=cp, radius_stage=stage)
                ctx.upload(0, q); ctx.upload(1, t)
                assert same(ctx.radius_search(0, 1, r), ref), (name, cp, stage)
                assert same(ctx.radius_search(0, 1, r, max_nn=17), capped(ref, 17)), (name, cp, stage)
    finally:
        ctx.tune(seq_cell_points=4, radius_stage=mvr.RADIUS_STAGE)


def test_all_identical_rows_are_ordered_by_index(ctx, mvr):
    """1 500 equal keys per row: the index decides (the long-row path at the default stage)"""
    q, t = W.get("all_identical", mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    o, idx, d2 = ctx.radius_search(0, 1, 0.5)
    assert ctx.stat("radius_long_rows") == len(q)
    assert np.array_equal(o, np.arange(len(q) + 1, dtype=np.uint64) * len(t))
    assert np.array_equal(idx.reshape(len(q), len(t)), np.tile(np.arange(len(t), dtype=np.uint32), (len(q), 1))) and not d2.any()


# ------------------------------------------------------------------ non-finite points (RS2)

def with_non_finite(p, count=60, seed=5):
    """the construction of tests/test_gpu_walk_fuzz.py: `count` scattered points get NaN, +inf or -inf in one coordinate, some
    in two, one in all three"""
    p = p.copy()
    rng = np.random.default_rng(seed)
    bad = rng.choice(len(p), count, replace=False)
    vals = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(bad):
        p[i, j % 3] = vals[(j // 3) % 3]
        if j % 5 == 0:
            p[i, (j + 1) % 3] = vals[(j // 2) % 3]
    p[bad[0], :3] = np.nan
    p[bad[1], :3] = (np.inf, -np.inf, np.nan)
    return p, bad


@pytest.mark.parametrize("fma", [False, True])
def test_non_finite_points(ctx, mvr, fma):
    q, t = W.get("patch_at_0", mvr)
    tq, bad_q = with_non_finite(q, 40, 6)
    tt, bad_t = with_non_finite(t)
    ctx.upload(0, tq); ctx.upload(1, tt)
    r = W.radii("patch_at_0", t)["several_cells"]
    for qs, qq, bad in ((0, tq, bad_q), (1, tt, bad_t)):
        ref = R.radius_search(qq, tt, r, fma=fma)
        got = ctx.radius_search(qs, 1, r, fma=fma)
        assert same(got, ref)
        lens = np.diff(got[0].astype(np.int64))
        assert (lens[bad] == 0).all() and not np.isin(got[1], bad_t).any() and np.isfinite(got[2]).all()
    # a cloud without a grid (3 points, one of them non-finite) and a cloud with no finite point
    small = W.cloud([[0.0, 0.0, 900.0], [np.nan, 0.0, 900.0], [0.1, 0.0, 900.0]])
    ctx.upload(2, small)
    assert same(ctx.radius_search(2, 2, 1.0, fma=fma), R.radius_search(small, small, 1.0, fma=fma))
    assert same(ctx.radius_search(0, 2, 1.0e4, fma=fma), R.radius_search(tq, small, 1.0e4, fma=fma))
    none = W.cloud(np.full((50, 3), np.nan))
    ctx.upload(2, none)
    for qs, n in ((2, 50), (0, len(tq))):
        o, idx, d2 = ctx.radius_search(qs, 2, 10.0, fma=fma)
        assert not o.any() and len(o) == n + 1 and len(idx) == 0 and len(d2) == 0
    o, total = ctx.radius_search(2, 1, 10.0, fma=fma, count_only=True)
    assert total == 0 and not o.any()


@pytest.mark.parametrize("fma", [False, True])
def test_finite_points_whose_distance_overflows(ctx, fma):
    """two groups of finite points 3e19 apart: the f32 d2 between them is +inf, so they are in no row of each other, with a grid
    (7 points) and without (3), at a radius whose square overflows too"""
    rng = np.random.default_rng(19)
    for n in (4, 2):
        t = np.concatenate([W.cloud(rng.standard_normal((n, 3))), W.cloud(rng.standard_normal((n - 1, 3)) + [3.0e19, 0.0, 0.0])])
        ctx.upload(0, t)
        for r in (100.0, 1.0e30):
            got = ctx.radius_search(0, 0, r, fma=fma)
            assert same(got, R.radius_search(t, t, r, fma=fma)), (n, r)
            assert np.array_equal(np.diff(got[0].astype(np.int64)), [n] * n + [n - 1] * (n - 1)) and np.isfinite(got[2]).all()


# ------------------------------------------------------------------ the protocol (RS7 - RS9)

def raw(mvr, ctx, qs, ts, prm, offsets, idx, d2, capacity, total):
    ptr = lambda a, ty: a.ctypes.data_as(C.POINTER(ty)) if a is not None else None
    return mvr._lib.mvr_radius_search(ctx._h, qs, ts, C.byref(prm) if prm is not None else None, ptr(offsets, C.c_uint64), ptr(idx, C.c_uint32),
                                      ptr(d2, C.c_float), capacity, C.byref(total) if total is not None else None)


def last_error(mvr, ctx):
    return mvr._lib.mvr_last_error(ctx._h).decode()


def test_sizing_protocol(ctx, mvr):
    q, t = W.get("size_257", mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    r = W.radii("size_257", t)["several_cells"]
    ref = R.radius_search(q, t, r)
    m = len(ref[1])
    assert m > 100
    prm = mvr.RadiusParams()
    mvr._lib.mvr_radius_default_params(C.byref(prm))
    assert (prm.radius, prm.max_nn, prm.sorted, prm.fma_dist) == (0.0, 0, 1, 0)
    prm.radius = r
    GUARD = 0xDEADBEEF
    # count-only: capacity ignored; offsets or total alone
    o, total = np.full(len(q) + 2, GUARD, np.uint64), C.c_size_t(GUARD)
    assert raw(mvr, ctx, 0, 1, prm, o, None, None, 0, total) == mvr.OK
    assert total.value == m and np.array_equal(o[:-1], ref[0]) and o[-1] == GUARD
    assert raw(mvr, ctx, 0, 1, prm, None, None, None, 0, None) == mvr.OK
    # a short capacity: total and offsets written, no entry written, both numbers named
    o[:] = GUARD; total.value = GUARD
    idx, d2 = np.full(m + 2, GUARD, np.uint32), np.full(m + 2, -7.0, F32)
    assert raw(mvr, ctx, 0, 1, prm, o, idx[1:], d2[1:], m - 1, total) == mvr.E_ARG
    assert total.value == m and np.array_equal(o[:-1], ref[0]) and (idx == GUARD).all() and (d2 == -7.0).all()
    assert str(m) in last_error(mvr, ctx) and str(m - 1) in last_error(mvr, ctx)
    # capacity = total exactly; the guards around the buffers stay
    assert raw(mvr, ctx, 0, 1, prm, o, idx[1:], d2[1:], m, total) == mvr.OK
    assert np.array_equal(idx[1:-1], ref[1]) and np.array_equal(bits(d2[1:-1]), bits(ref[2]))
    assert idx[0] == GUARD and idx[-1] == GUARD and d2[0] == -7.0 and d2[-1] == -7.0 and o[-1] == GUARD
    # either output alone
    idx[:] = GUARD; d2[:] = -7.0
    assert raw(mvr, ctx, 0, 1, prm, None, idx[1:], None, m, None) == mvr.OK and np.array_equal(idx[1:-1], ref[1])
    assert raw(mvr, ctx, 0, 1, prm, None, None, d2[1:], m + 5, None) == mvr.OK and np.array_equal(bits(d2[1:-1]), bits(ref[2]))
    assert idx[-1] == GUARD and d2[-1] == -7.0


def test_refusals_write_nothing(ctx, mvr):
    q, t = W.get("size_65", mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    GUARD = 0xDEADBEEF
    o, total = np.full(len(q) + 1, GUARD, np.uint64), C.c_size_t(GUARD)
    idx, d2 = np.full(64, GUARD, np.uint32), np.full(64, -7.0, F32)

    def untouched():
        return (o == GUARD).all() and total.value == GUARD and (idx == GUARD).all() and (d2 == -7.0).all()

    ok = mvr.RadiusParams(1.0, 0, 1, 0)
    assert mvr._lib.mvr_radius_search(None, 0, 1, C.byref(ok), None, None, None, 0, None) == mvr.E_ARG
    ctx.size(0)                                                           # (a call that succeeds: the error text below is this test's)
    assert raw(mvr, ctx, 0, 1, None, o, idx, d2, 64, total) == mvr.E_ARG and untouched()
    assert "no parameters" in last_error(mvr, ctx)
    for qs, ts in ((-1, 1), (0, -1), (mvr.MAX_SLOTS, 1), (0, mvr.MAX_SLOTS), (1 << 20, 0)):
        assert raw(mvr, ctx, 0, 1, mvr.RadiusParams(-1.0, 0, 1, 0), None, None, None, 0, None) == mvr.E_ARG      # (another text in between)
        assert raw(mvr, ctx, qs, ts, ok, o, idx, d2, 64, total) == mvr.E_ARG and untouched(), (qs, ts)
        assert "slot" in last_error(mvr, ctx), (qs, ts)
    for r in (0.0, -1.0, np.nan, np.inf, -np.inf):
        assert raw(mvr, ctx, 0, 1, mvr.RadiusParams(r, 0, 1, 0), o, idx, d2, 64, total) == mvr.E_ARG and untouched(), r
        assert "radius" in last_error(mvr, ctx)
        for kw in (dict(), dict(count_only=True)):
            with pytest.raises(ValueError):
                ctx.radius_search(0, 1, r, **kw)
    with pytest.raises(ValueError):
        ctx.radius_search(0, mvr.MAX_SLOTS, 1.0)
    with pytest.raises(ValueError):
        ctx.radius_search(0, 1, 1.0, max_nn=-1)


def test_empty_slots(ctx, mvr):
    q, t = W.get("size_65", mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    ctx.upload(3, np.zeros((0, 4), F32))
    o, idx, d2 = ctx.radius_search(3, 1, 5.0)                               # no query: offsets[0] = 0
    assert o.tolist() == [0] and len(idx) == 0 and len(d2) == 0
    o, total = ctx.radius_search(3, 3, 5.0, count_only=True)
    assert o.tolist() == [0] and total == 0
    o, idx, d2 = ctx.radius_search(0, 3, 5.0)                               # no target: empty rows
    assert len(o) == len(q) + 1 and not o.any() and len(idx) == 0


# ------------------------------------------------------------------ RS10

def test_slots_are_left_as_they_were(ctx, mvr):
    q, t = W.get("patch_at_0", mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    ctx.estimate_normals([0, 1], k=16)
    r = W.radii("patch_at_0", t)["several_cells"]
    before = [(ctx.size(s), ctx.download(s).tobytes(), ctx.download_normals(s).tobytes()) for s in (0, 1)]
    knn_before = [a.tobytes() for a in ctx.knn(0, 1, 9)]
    for kw in (dict(), dict(sorted=False), dict(max_nn=5), dict(count_only=True)):
        ctx.radius_search(0, 1, r, **kw)
        ctx.radius_search(1, 1, r, **kw)
    assert before == [(ctx.size(s), ctx.download(s).tobytes(), ctx.download_normals(s).tobytes()) for s in (0, 1)]
    assert knn_before == [a.tobytes() for a in ctx.knn(0, 1, 9)]
    nrm = ctx.download_normals(1).tobytes()
    ctx.estimate_normals([1], k=16)
    assert ctx.download_normals(1).tobytes() == nrm
