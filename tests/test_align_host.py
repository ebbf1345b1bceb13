"""CPU tests of the feature matching and the sample-consensus alignment that need no device: the numpy reference
(tests/align_ref.py) checked against itself and against the written formulas, the conditions on the shared inputs
(tests/align_cases.py), the exported symbols, their argument refusals, and the resources of the kernels of csrc/mvr_feature.hip.

Measured here: 0.53 of the 200 iterations of the align case are polygon-rejected (similarity 0.5, k = 2, three samples), 94 are
scored; chi-square of 40 000 draws over 50 bins 35.5 / 51.0 / 46.7 for the three samples (bound 86.7).

Which inputs see the order and the rounding of M1 (the five wrong accumulations of align_ref.WRONG_D2: fma chain, four
accumulators, reverse order, pairwise tree, f64 rounded once): on knn_plain and knn_duplicates 0 of 210 000 pairs differ in a bit
for any of the five.  On knn_real 0.33 / 0.66 / 0.73 / 0.63 / 0.63 of the pairs change their d2 bits and the k = 10 lists of
297 / 300 / 300 / 300 / 300 of 300 queries; on knn_fpfh_like 0.32 / 0.65 / 0.72 / 0.63 / 0.63 and 294 / 300 / 300 / 300 / 300; on
knn_signatures (810 000 pairs) 0.32 / 0.64 / 0.72 / 0.60 / 0.62 and 293 / 300 / 300 / 299 / 300 -- but an index of those lists
changes for at most 1 query.  On knn_twins the two d2 differ in f32 for 201 of 300 queries and the nearest row changes for
57 / 121 / 152 / 113 / 104 of 300 queries; 10 twin pairs straddle a tile boundary."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import align_cases as AC
import align_ref as R
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ the draws

def mix_int(z):
    """rule A2's mix in Python integers"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_int(seed, i, j, m):
    return ((mix_int((seed + 0x9E3779B97F4A7C15 * (16 * i + j + 1)) & M64) >> 32) * m) >> 32


# (seed, i, j, m) -> draw: written out once from align_ref.draw; every row is checked below against the formula in Python integers
FROZEN_DRAWS = [((0, 0, 0, 1000), 883), ((0, 0, 1, 999), 431), ((1, 5, 2, 7), 2), ((2026, 199, 10, 2), 0),
                ((0xFFFFFFFFFFFFFFFF, 3, 0, 400), 315), ((12345678901234567890, 100000, 7, 1 << 31), 1324887866)]


def test_draws_match_the_formula_and_the_frozen_table():
    assert int(R.mix(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF == mix_int(0x9E3779B97F4A7C15)      # splitmix64's first output for the seed 0
    assert int(R.mix(np.uint64(1))) == 0x5692161D100B05E5 == mix_int(1) and int(R.mix(np.uint64(0))) == 0
    for args, want in FROZEN_DRAWS:
        assert int(R.draw(*args)) == want == draw_int(*args), args
    i = np.arange(1000)
    assert np.array_equal(R.draw(7, i, 3, 123), [draw_int(7, int(a), 3, 123) for a in i])      # vectorised over i
    assert R.sample_positions(2026, 0, 400, 3) == [343, 188, 266] and R.sample_positions(1, 0, 5, 5) == [2, 3, 4, 0, 1]


def test_samples_are_distinct_and_cover_the_range():
    for ne, nr in ((3, 3), (8, 8), (9, 8), (400, 3), (400, 5)):
        seen = set()
        for i in range(300):
            pos = R.sample_positions(11, i, ne, nr)
            assert len(set(pos)) == nr and min(pos) >= 0 and max(pos) < ne, (ne, nr, i, pos)
            seen.update(pos)
        if ne <= 9:
            assert seen == set(range(ne))


def test_samples_are_uniform():
    """chi-square of every sample position over ne = 50 bins, 40 000 iterations: 49 degrees of freedom, whose 0.9995 quantile is
    86.7 -- three tests (sample 0, 1, 2), so a correct generator fails this with probability below 0.002, and the seed is fixed"""
    ne, n = 50, 40000
    counts = np.zeros((3, ne))
    for i in range(n):
        for j, r in enumerate(R.sample_positions(5, i, ne, 3)):
            counts[j, r] += 1
    chi = ((counts - n / ne) ** 2 / (n / ne)).sum(1)
    print("chi-square per sample:", chi)
    assert (chi < 86.7).all()


# ------------------------------------------------------------------ the polygon rule

def tri(*pts):
    return np.array(pts, F32)


def test_polygon_rule_on_hand_made_triangles():
    a = tri((0, 0, 0), (3, 0, 0), (0, 4, 0))                             # squared edges 9, 25, 16
    assert R.polygon_ok(a, a, 0.99) and R.polygon_ok(a, a + F32(100.0), 0.99)
    b = tri((0, 0, 0), (6, 0, 0), (0, 8, 0))                             # every squared edge four times as long: sim = 0.25
    assert R.polygon_ok(a, b, 0.5) and R.polygon_ok(b, a, 0.5)          # 0.25 >= 0.5^2: the threshold itself passes
    assert not R.polygon_ok(a, b, 0.51) and not R.polygon_ok(b, a, 0.51)
    c = tri((0, 0, 0), (3, 0, 0), (0, 8, 0))                             # one edge equal, two longer: the worst edge decides
    assert R.polygon_ok(a, c, 0.5) and not R.polygon_ok(a, c, 0.51)
    z = tri((0, 0, 0), (0, 0, 0), (0, 4, 0))                             # a zero edge on both sides: 0 / 0 fails, whatever the threshold
    assert not R.polygon_ok(z, z, 0.0)
    assert R.polygon_ok(a, z, 0.0) and not R.polygon_ok(a, z, 0.01)     # 0 / 9 = 0 passes only the threshold 0
    n = a.copy(); n[1, 0] = np.nan
    assert not R.polygon_ok(a, n, 0.0)
    sq = tri((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0))                 # nr = 4: the closing edge (3, 0) is tested
    sk = tri((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 3, 0))
    assert R.polygon_ok(sq, sq, 0.9) and not R.polygon_ok(sq, sk, 0.9)


def test_align_case_rejects_between_a_quarter_and_three_quarters():
    """a condition on the input: both arms of the polygon test stay exercised"""
    s, t, sf, tf = AC.align_pair()
    el = R.eligible(s, sf)
    assert len(el) == AC.ALIGN_NS
    idx, _ = R.feature_knn(sf[el], tf, AC.ALIGN_K)
    st, src, tgt = R.replay(s, t, el, idx, AC.ALIGN_ITERS, 3, AC.ALIGN_SEED, AC.ALIGN_SIMILARITY)
    share = float((st == 0).mean())
    print("rejected %.3f, scored %d" % (share, int((st == 1).sum())))
    assert 0.25 <= share <= 0.75 and (st != 2).all()
    s2, t2, sf2, tf2 = AC.align_with_invalid()
    el2 = R.eligible(s2, sf2)
    assert len(el2) == AC.ALIGN_NS - 30 and np.isfinite(s2[el2, :3]).all() and np.isfinite(sf2[el2]).all()


def test_reference_knn_order_and_non_finite_rows():
    q, t = AC.knn_non_finite()
    idx, d2 = R.feature_knn(q, t, 10)
    badq, badt = ~np.isfinite(q).all(1), ~np.isfinite(t).all(1)
    assert badq.sum() >= 15 and badt.sum() >= 35
    assert (idx[badq] == R.NONE).all() and np.isinf(d2[badq]).all()
    assert not np.isin(idx[~badq], np.nonzero(badt)[0]).any() and (idx[~badq] != R.NONE).all()
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
    assert (np.diff(key[~badq].astype(object), axis=1) > 0).all()
    D = R.feat_d2(q[~badq][:5], t)
    assert np.array_equal(np.sort(D[:, ~badt], axis=1)[:, :10], d2[~badq][:5])
    x = R.feat_d2(q[~badq][:1], t[~badt][:1])[0, 0]                      # M1 by hand, scalar by scalar
    acc = F32(0)
    for b in range(33):
        diff = F32(q[~badq][0, b] - t[~badt][0, b])
        acc = F32(acc + F32(diff * diff))
    assert acc == x


# ------------------------------------------------------------------ which inputs can see the order and the rounding of M1

def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def real_tables():
    return {name: getattr(AC, "knn_" + name)() for name in ("plain", "real", "fpfh_like", "signatures", "twins")}


def test_feat_d2_is_the_scalar_loop_on_real_values(real_tables):
    """M1 written out on np.float32 scalars, one rounded operation after the other, on 200 random pairs of every table"""
    rng = np.random.default_rng(9)
    for name, (q, t) in real_tables.items():
        D = R.feat_d2(q, t)
        for i, j in zip(rng.integers(0, len(q), 200), rng.integers(0, len(t), 200)):
            acc = F32(0)
            for b in range(AC.DIM):
                diff = F32(q[i, b] - t[j, b])
                acc = F32(acc + F32(diff * diff))
            assert acc.view(np.uint32) == D[i, j].view(np.uint32), (name, i, j)


def test_integer_valued_tables_cannot_tell_a_wrong_accumulation_from_m1(real_tables):
    """the blind spot of knn_plain and of everything built from align_cases.features(): every partial sum is an exact integer
    below 2^24, so the fma chain, four accumulators, the reverse order, a tree and an f64 sum all give the bits of M1"""
    for q, t in (real_tables["plain"], AC.knn_duplicates()):
        D = R.feat_d2(q, t)
        assert D.max() < 2.0 ** 24 and (D == np.round(D)).all()
        for what, wrong in R.WRONG_D2.items():
            assert np.array_equal(bits(wrong(q, t)), bits(D)), what


@pytest.mark.parametrize("name", ["real", "fpfh_like", "signatures"])
def test_real_valued_tables_tell_every_wrong_accumulation_from_m1(name, real_tables):
    """a condition on the inputs: where it fails the input changes, not the bar.  Every wrong accumulation changes the d2 bits
    of at least a tenth of the pairs and the d2 bits of the k = 10 list of at least half of the queries"""
    q, t = real_tables[name]
    D = R.feat_d2(q, t)
    assert np.isfinite(D).all()
    want = R.knn_from_d2(D, 10)
    ri, rd = R.feature_knn(q, t, 10)
    assert np.array_equal(ri, want[0]) and np.array_equal(bits(rd), bits(want[1]))
    for what, wrong in R.WRONG_D2.items():
        W = wrong(q, t)
        pairs = float((bits(W) != bits(D)).mean())
        got = R.knn_from_d2(W, 10)
        lists = int((bits(got[1]) != bits(want[1])).any(1).sum())
        index = int((got[0] != want[0]).any(1).sum())
        print("%s, %s: %.3f of %d pairs change their d2 bits; the k = 10 list of %d of %d queries changes in d2, of %d in an index"
              % (name, what, pairs, D.size, lists, len(q), index))
        assert pairs >= 0.10, (name, what)
        assert lists >= len(q) // 2, (name, what)


def test_twins_turn_a_wrong_accumulation_into_a_wrong_index(real_tables):
    """a condition on the input: the two twins of a query have the same d2 in exact arithmetic, different bits under M1 for most
    queries, and every wrong accumulation names the other twin first for at least 20 of the 300 queries"""
    q, t = real_tables["twins"]
    first = AC.twin_first_rows()
    rows = np.arange(len(q))
    exact = ((q.astype(F64)[:, None, :] - np.stack([t[first], t[first + 1]], 1).astype(F64)) ** 2).sum(2)
    assert (exact[:, 0] == exact[:, 1]).all()                            # sums of 33 multiples of 2^-20 below 2^12: exact in f64
    D = R.feat_d2(q, t)
    differ = int((bits(D[rows, first]) != bits(D[rows, first + 1])).sum())
    want = R.knn_from_d2(D, 2)[0]
    assert np.array_equal(np.sort(want, axis=1), np.stack([first, first + 1], 1))      # the twins lead every list
    edge = int(((first + 1) % AC.FEAT_TILE == 0).sum())
    print("twins: the two d2 differ in f32 for %d of %d queries; %d pairs straddle a tile boundary" % (differ, len(q), edge))
    assert differ >= len(q) // 2 and edge >= 10
    for what, wrong in R.WRONG_D2.items():
        got = R.knn_from_d2(wrong(q, t), 2)[0]
        assert np.array_equal(np.sort(got, axis=1), np.sort(want, axis=1)), what
        swapped = int((got[:, 0] != want[:, 0]).sum())
        print("twins, %s: the nearest row changes for %d of %d queries" % (what, swapped, len(q)))
        assert swapped >= 20, what


def test_range_and_key_zero_cases_hold_what_they_say():
    q, t = AC.knn_range()
    idx, d2 = R.feature_knn(q, t, 10)
    D = R.feat_d2(q, t)
    assert np.isfinite(q).all() and np.isfinite(t).all() and np.isinf(D).sum() >= 40 + 10 * (len(q) - 1) + len(t) - 10
    twin = np.array([np.nonzero((t[:, :] == q[i]).sum(1) == AC.DIM - 1)[0][0] for i in range(40)])      # the copy but for one component
    assert np.isinf(D[np.arange(40), twin]).all() and not (idx[:40] == twin[:, None]).any()
    assert (idx[40] != R.NONE).all()
    assert (t[idx[40].astype(np.int64), 7] >= F32(AC.RANGE_BIG)).all()
    assert (R.feature_knn(q, t, 64)[0][40] != R.NONE).sum() == 10
    under = np.arange(50, 130)
    assert (d2[under, :2] == 0).all() and (d2[under, 2] > 0).all() and (idx[under, 0] < idx[under, 1]).all()
    near = (t[idx[under, 0].astype(np.int64)] != q[under]).any(1)        # the leading row is the near copy ...
    assert np.array_equal(near, under % 2 == 0)                          # ... for the even queries, the exact one for the odd
    q, t = AC.knn_key_zero()
    idx, d2 = R.feature_knn(q, t, 10)
    assert list(idx[0, :6]) == [0, 1, 2, 3, 4, 5] and (bits(d2[0, :6]) == 0).all() and d2[0, 6] > 0
    assert (d2[::3, 0] == 0).all() and (d2[:, 0] == 0).sum() == len(q[::3])


# ------------------------------------------------------------------ the C-ABI

NEW = ("mvr_feature_knn", "mvr_pose_scores", "mvr_align_prerejective")


def test_library_exports_the_new_symbols(mvr):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    for name in NEW:
        assert name in mvr.SIGNATURES and re.search(r" T %s$" % name, r.stdout, re.M), name
    assert C.sizeof(mvr.PrerejParams) == 56 and C.sizeof(mvr.PrerejResult) == 96 and C.sizeof(mvr.PrerejTrace) == 144
    assert all(hasattr(mvr.Context, m) for m in ("feature_knn", "pose_scores", "align_prerejective"))
    hdr = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    assert re.search(r"#define MVR_PREREJ_MAX_SAMPLES 8\b", hdr) and mvr.PREREJ_MAX_SAMPLES == 8


def params(mvr, **kw):
    d = dict(max_iterations=10, nr_samples=3, k=2, similarity=0.5, max_dist=2.0, inlier_fraction=0.25, seed=1, fma_dist=0)
    d.update(kw)
    return mvr.PrerejParams(d["max_iterations"], d["nr_samples"], d["k"], d["similarity"], d["max_dist"], d["inlier_fraction"], d["seed"],
                            d["fma_dist"])


def test_refusals_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                                  # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    f = (C.c_float * 66)(*[1.0] * 66)
    idx, d2 = (C.c_uint32 * 128)(*[9] * 128), (C.c_float * 128)(*[9.0] * 128)
    knn = L.mvr_feature_knn
    assert knn(None, f, 1, f, 1, 33, 1, idx, d2) == mvr.E_ARG
    for dim in (0, 3, 32, 34, 66, -33):
        assert knn(ctx, f, 1, f, 1, dim, 1, idx, d2) == mvr.E_ARG
    for k in (0, -1, 65, 1 << 20):
        assert knn(ctx, f, 1, f, 1, 33, k, idx, d2) == mvr.E_ARG
    assert list(idx) == [9] * 128 and list(d2) == [9.0] * 128
    T = (C.c_float * 16)(*np.eye(4, dtype=F32).ravel())
    inl, err = (C.c_uint32 * 1)(9), (C.c_double * 1)(9.0)
    sc = L.mvr_pose_scores
    assert sc(None, 0, 1, T, 1, 2.0, 0, inl, err) == mvr.E_ARG
    for s, t in ((-1, 0), (0, mvr.MAX_SLOTS), (1 << 20, 0)):
        assert sc(ctx, s, t, T, 1, 2.0, 0, inl, err) == mvr.E_ARG
    for md in (0.0, -1.0, math.nan, math.inf):
        assert sc(ctx, 0, 1, T, 1, md, 0, inl, err) == mvr.E_ARG
    assert sc(ctx, 0, 1, None, 1, 2.0, 0, inl, err) == mvr.E_ARG
    assert inl[0] == 9 and err[0] == 9.0
    al = L.mvr_align_prerejective
    res = mvr.PrerejResult()
    res.inliers = 77
    ok = params(mvr)
    assert al(None, 0, 1, f, f, C.byref(ok), None, C.byref(res), None) == mvr.E_ARG
    assert al(ctx, 0, 1, f, f, None, None, C.byref(res), None) == mvr.E_ARG
    assert al(ctx, 0, 1, f, f, C.byref(ok), None, None, None) == mvr.E_ARG
    assert al(ctx, 0, 1, None, f, C.byref(ok), None, C.byref(res), None) == mvr.E_ARG
    assert al(ctx, -1, 1, f, f, C.byref(ok), None, C.byref(res), None) == mvr.E_ARG
    bad = [dict(similarity=v) for v in (-0.1, 1.0, 1.5, math.nan)] + [dict(inlier_fraction=v) for v in (0.0, -0.5, 1.01, math.nan)] + \
          [dict(nr_samples=v) for v in (0, 2, 9, -3)] + [dict(k=v) for v in (0, 65, -1)] + [dict(max_dist=v) for v in (0.0, -2.0, math.nan, math.inf)] + \
          [dict(max_iterations=-1)]
    for kw in bad:
        p = params(mvr, **kw)
        assert al(ctx, 0, 1, f, f, C.byref(p), None, C.byref(res), None) == mvr.E_ARG, kw
    assert res.inliers == 77
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the kernels' resources

def test_feature_kernels_use_no_scratch(built, tmp_path):
    """the k-NN and the scoring kernels keep their lists and sums in registers; the hypotheses kernel (one thread per
    iteration, a few thousand threads in all) indexes its eight samples at run time and is left out"""
    from test_fpfh_host import _usage
    assert "mvr_feature.hip" in built.HIP_SOURCES
    use = _usage(built, tmp_path, "mvr_feature.hip")
    print([(re.sub(r"^_ZN3mvr12_GLOBAL__N_1\d+", "", n), v, s, l) for n, v, s, l in use])
    hot = [u for u in use if "prerej_hypotheses" not in u[0]]
    assert len(hot) == 4 + 4 + 2 + 1, use                               # k-NN and merge per bucket, scoring x fma, the pose sums
    assert all(s == 0 for _, _, s, _ in hot), [(n, s) for n, _, s, _ in hot if s]
    knn = [u for u in hot if "feature_knn_kernel" in u[0]]
    assert len(knn) == 4 and all(l == 64 * 36 * 4 for _, _, _, l in knn)      # one tile of 64 padded rows
    assert all(v <= 256 for _, v, _, _ in hot)                          # two waves per SIMD at least
