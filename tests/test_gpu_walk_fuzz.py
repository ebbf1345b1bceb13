"""Adversarial inputs for the kernels that walk a cloud's OWN grid (GPU): mvr_knn, mvr_cloud_estimate_normals and the two
outlier filters, on the degenerate geometries of tests/test_gpu_fuzz.py and more (tests/walk_cases.py: far frames, lattices
with mass ties, clusters with thousands of points per cell, scattered duplicates, sizes around every launch edge), with
non-finite points (the rule N1 - N6 of include/mvr_hip.h), under every grid resolution and on random shapes.

Lists, distances, mean distances and counts are compared BIT FOR BIT with the brute-force references (tests/normals_ref.py,
tests/outlier_ref.py).  The only tolerances are those of tests/test_gpu_normals.py -- 1e-5 rad where the eigen-gap is at least
1e-4, curvature within 1e-6 -- and the orthogonality bar of the collinear case (test_normals_k_mode)."""
import importlib
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import normals_ref as N
import outlier_ref as O
import walk_cases as W
from conftest import PKG
from test_gpu_outlier import MIN_GAP, check_sor, same_bits, sor

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NONE = N.NONE


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


_knn_refs = {}


def knn_ref(tag, q, t, fma):
    """knn_brute at k = 64, cached: the list at any smaller k is its prefix (the order is total)"""
    key = (tag, bool(fma))
    if key not in _knn_refs:
        _knn_refs[key] = N.knn_brute(q, t, 64, fma=fma)
    return _knn_refs[key]


def check_knn(ctx, qs, ts, ref, ks, fma, what):
    ri, rd = ref
    for k in ks:
        gi, gd = ctx.knn(qs, ts, k, fma=fma)
        assert np.array_equal(gi, ri[:, :k]), (what, k, fma)
        assert np.array_equal(bits(gd), bits(rd[:, :k])), (what, k, fma)
    ni, nd = ctx.nn(qs, ts, fma=fma)
    assert np.array_equal(ni, ri[:, 0]) and np.array_equal(bits(nd), bits(rd[:, 0])), (what, "k = 1 is mvr_nn", fma)


# ------------------------------------------------------------------ k-NN lists

@pytest.mark.parametrize("name", W.NAMES)
def test_knn_lists(ctx, mvr, name):
    """k just above every list bucket (9, 17, 33), just below the largest (63) and the ends, fma off and on, the target against
    itself and the query cloud against it: idx and the bits of d2 equal the brute force; k = 1 equals mvr_nn"""
    q, t = W.get(name, mvr)
    ctx.upload(0, q); ctx.upload(1, t)
    for fma in (False, True):
        check_knn(ctx, 1, 1, knn_ref((name, "self"), t, t, fma), W.KS, fma, (name, "self"))
        check_knn(ctx, 0, 1, knn_ref((name, "cross"), q, t, fma), W.KS, fma, (name, "cross"))


# ------------------------------------------------------------------ statistical filter

@pytest.mark.parametrize("name", W.NAMES)
def test_statistical_filter(ctx, mvr, name):
    """mean_dist bit-identical at mean_k just above the buckets (fma off and on); index, points and statistics through
    check_sor (tests/test_gpu_outlier.py) with its gap precondition on the reference -- except at the mean_k the case table
    names (no_sets), where mean distances and statistics alone are compared"""
    _, t = W.get(name, mvr)
    no_sets = W.TABLE[name][2]
    for k in W.MEAN_KS:
        ref = O.statistical(t, k, 1.0)
        got = sor(ctx, t, k, 1.0)
        if k in no_sets:
            assert same_bits(got[2], ref["mean_dist"]) and got[3]["n_valid"] == ref["stats"]["n_valid"]
            for key in ("mean", "stddev", "threshold"):
                a, b = got[3][key], ref["stats"][key]
                assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= 1e-12 * abs(b), (name, k, key, a, b)
        else:
            assert ref["gap"] >= MIN_GAP, (name, k, ref["gap"])
            check_sor(t, got, ref)
        n, md = ctx.statistical_outlier_removal(2, 0, k, 1.0, fma=True, return_dist=True)
        assert same_bits(md, O.mean_dist(t, k, True)[0]), (name, k, "fma")


# ------------------------------------------------------------------ radius filter and radius-mode normals

@pytest.mark.parametrize("name", W.NAMES)
def test_radius_counts(ctx, mvr, name):
    """balls of a fraction of a cell, several cells, more than the whole cloud, (float)(r * r) == 0 (exact duplicates only)
    and, on the lattices, exact lattice distances (d2 == r2 counts): counts equal the reference, fma off and on"""
    _, t = W.get(name, mvr)
    ctx.upload(0, t)
    for tag, r in W.radii(name, t).items():
        for fma in (False, True):
            n, idx, cnt = ctx.radius_outlier_removal(1, 0, r, 1, fma=fma, return_index=True, return_counts=True)
            ref = O.neighbor_counts(t, r, fma)
            assert np.array_equal(cnt, ref), (name, tag, r, fma)
            assert np.array_equal(idx, np.nonzero(ref >= 1)[0])
        if tag == "whole_cloud":
            assert (cnt == len(t) - 1).all()
        if tag == "lattice_distance" and name == "lattice_3d":
            g = np.stack(np.meshgrid(np.arange(16), np.arange(15), np.arange(14), indexing="ij"), -1).reshape(-1, 3)
            inner = ((g > 0) & (g < np.array([15, 14, 13]))).sum(1)
            assert np.array_equal(cnt, 3 + inner)            # independent of the reference: the 6 lattice neighbours, fewer on faces
        if tag == "zero_r2":
            d1 = knn_ref((name, "self"), t, t, False)[1]
            assert np.array_equal(cnt > 0, d1[:, min(1, d1.shape[1] - 1)] == 0) or len(t) < 2


def compare_normals(nrm, curv, ref, rc, w, p, cap, what, vp=(0.0, 0.0, 0.0)):
    """the bars of tests/test_gpu_normals.py: equal NaN masks, 1e-5 rad where gap >= 1e-4, curvature within 1e-6, the same
    orientation where rounding does not decide it; at most `cap` of the points with a normal excluded by the gap rule
    (cap None: no angle is compared -- the direction is not defined)"""
    ok = ~np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(nrm[:, :3]).any(1), ~ok) and np.array_equal(np.isnan(curv), ~ok), what
    assert (nrm[:, 3] == 0).all()
    if ok.any():
        assert np.abs(curv[ok].astype(F64) - rc[ok]).max() <= 1e-6, what
        assert np.abs(np.linalg.norm(nrm[ok, :3].astype(F64), axis=1) - 1.0).max() <= 1e-6, what
    if cap is None:
        return
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    good = ok & (gap >= 1e-4)
    assert (ok & ~good).sum() <= cap * ok.sum(), (what, int((ok & ~good).sum()), int(ok.sum()))
    if good.any():
        ang = N.angle_between(nrm[good], ref[good], unsigned=True)
        assert ang.max() <= 1e-5, (what, ang.max())
        v = np.asarray(vp, F64)[None, :] - p[:, :3].astype(F64)
        cs = np.sum(v * ref[:, :3], 1)
        sure = good & (np.abs(cs) > 1e-4 * np.linalg.norm(v, axis=1))
        assert (np.sum(nrm[sure, :3].astype(F64) * ref[sure, :3], 1) > 0).all(), what


def check_exact_shapes(kind, nrm, curv, ok, what, w=None):
    """answers that need no reference"""
    if kind == "plane":
        with np.errstate(invalid="ignore", divide="ignore"):       # (a neighbourhood that is itself collinear has no plane)
            ok = ok & ((w[:, 1] - w[:, 0]) / w[:, 2] >= 1e-4)
        assert (nrm[ok, 0] == 0).all() and (nrm[ok, 1] == 0).all() and (nrm[ok, 2] == -1).all(), what      # towards the origin
        assert (curv[ok] == 0).all(), what
    if kind == "line":
        # orthogonal to the line (the x axis).  The numpy reference achieves |n . x| = 0 exactly on this input (the covariance
        # is exactly diagonal; tests/test_walk_cases_host.py asserts the 0), and ten times 0 is 0 -- so the bar is the
        # precision of the f32 the normal is stored in, 2^-23
        assert np.isfinite(nrm[ok, :3]).all() and (np.abs(nrm[ok, 0]) <= 2.0 ** -23).all(), what
    if kind == "point":
        assert np.isfinite(nrm[ok, :3]).all() and (curv[ok] == 0).all(), what


@pytest.mark.parametrize("name", W.NAMES)
def test_normals_k_mode(ctx, mvr, name):
    """k = 16 and 17 (a full bucket and one more) against normals_ref on the reference's own lists; fma off and on.
    Collinear case: the reference's normal has |n . x| = 0 exactly (measured on the CPU), the bar is 2^-23 (check_exact_shapes)"""
    _, t = W.get(name, mvr)
    kind, cap, _ = W.TABLE[name]
    ctx.upload(0, t)
    for k, fma in ((16, False), (17, False), (16, True)):
        curv = ctx.estimate_normals(0, k=k, curvature=True, fma=fma)
        nrm = ctx.download_normals(0)
        ri, _ = knn_ref((name, "self"), t, t, fma)
        ref, rc, w = N.normals_from_lists(t, ri[:, :k])
        compare_normals(nrm, curv, ref, rc, w, t, cap if kind in ("surface", "volume", "plane") else None, (name, k, fma))
        check_exact_shapes(kind, nrm, curv, ~np.isnan(ref[:, 0]), (name, k, fma), w)


@pytest.mark.parametrize("name", W.NAMES)
def test_normals_radius_mode(ctx, mvr, name):
    """the radii of test_radius_counts; the cap applies at `several_cells` (walk_cases.py), the whole-cloud ball is taken on
    clouds of at most 1100 points (its sets are the cloud squared)"""
    _, t = W.get(name, mvr)
    kind, cap, _ = W.TABLE[name]
    ctx.upload(0, t)
    for tag, r in W.radii(name, t).items():
        if tag == "whole_cloud" and len(t) > 1100:
            continue
        for fma in (False, True):
            curv = ctx.estimate_normals(0, radius=r, curvature=True, fma=fma)
            nrm = ctx.download_normals(0)
            flat, offs = N.radius_sets(t, r, fma=fma)
            cnt = np.diff(offs)
            assert np.array_equal(cnt, O.neighbor_counts(t, r, fma).astype(np.int64) + 1)       # the two references agree
            ref, rc, w = N.normals_from_sets(t, flat, offs)
            use_cap = cap if (tag == "several_cells" and kind in ("surface", "volume", "plane")) else None
            if use_cap is None and kind in ("surface", "volume", "plane"):
                use_cap = 1.0                  # other radii: angles wherever the gap rule allows, no share promised
            compare_normals(nrm, curv, ref, rc, w, t, use_cap, (name, tag, fma))
            check_exact_shapes(kind, nrm, curv, ~np.isnan(ref[:, 0]), (name, tag, fma), w)


# ------------------------------------------------------------------ the grid's resolution must not show

def _everything(ctx, p, r):
    out = []
    ctx.upload(0, p)
    for k in (9, 17, 64):
        i, d = ctx.knn(0, 0, k)
        out += [i.tobytes(), d.tobytes()]
    ctx.upload(0, p)
    out.append(ctx.statistical_outlier_removal(1, 0, 9, 1.0, return_dist=True)[1].tobytes())
    out.append(ctx.radius_outlier_removal(1, 0, r, 1, return_counts=True)[1].tobytes())
    for kw in (dict(k=16), dict(radius=r)):
        out.append(ctx.estimate_normals(0, curvature=True, **kw).tobytes())
        out.append(ctx.download_normals(0).tobytes())
    return out


@pytest.mark.parametrize("name", ["view_20k", "patch_far_1e6", "lattice_3d", "clusters_and_a_far_point", "collinear", "duplicates_41"])
def test_results_do_not_depend_on_the_grid_resolution(ctx, mvr, name):
    """seq_cell_points 1, 4 (the default), 64 and 4096 change the cell edge of every grid built afterwards (a slot keeps its
    grid until its points change: the cloud is uploaded again after each tune): identical bytes from knn, mean_dist, counts and
    normals with curvature"""
    p = mvr.synth_view(mvr.synth_params(12, 2), 0, 20000) if name == "view_20k" else W.get(name, mvr)[1]
    r = W.radii(name, p)["several_cells"]
    try:
        base = None
        for cp in (4, 1, 64, 4096):
            ctx.tune(seq_cell_points=cp)
            got = _everything(ctx, p, r)
            if base is None:
                base = got
            assert all(a == b for a, b in zip(got, base)), (name, cp, [a == b for a, b in zip(got, base)])
    finally:
        ctx.tune(seq_cell_points=4)
    if name != "view_20k":                                   # ... and they are the right bytes
        ri, rd = knn_ref((name, "self"), p, p, False)
        assert base[4] == ri.tobytes() and base[5] == rd.tobytes()


# ------------------------------------------------------------------ random shapes

def test_random_shapes(ctx):
    """25 seeded trials as in tests/test_gpu_fuzz.py: nq, nt in 1..6000, scale 0.5 / 5 / 50, sprinkled duplicates, random k and
    radius: knn (cross and self), mean_dist and counts bit for bit"""
    run_random_shapes(ctx, 25, 11)


def run_random_shapes(ctx, trials, seed, log=None):
    rng = np.random.default_rng(seed)
    for trial in range(trials):
        nq, nt = int(rng.integers(1, 6001)), int(rng.integers(1, 6001))
        scale = float(rng.choice([0.5, 5.0, 50.0]))
        q = W.cloud(rng.standard_normal((nq, 3)) * scale + [0, 0, 900])
        t = W.cloud(rng.standard_normal((nt, 3)) * scale + [0, 0, 900])
        if trial % 3 == 0 and nt >= 10:                      # sprinkle duplicates
            t[rng.integers(0, nt, nt // 10)] = t[rng.integers(0, nt, nt // 10)]
        k, mk = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        fma = bool(rng.integers(0, 2))
        r = scale * float(rng.choice([0.02, 0.2, 1.0]))
        ctx.upload(0, q); ctx.upload(1, t)
        for qs, qq in ((0, q), (1, t)):
            gi, gd = ctx.knn(qs, 1, k, fma=fma)
            ri, rd = N.knn_brute(qq, t, k, fma=fma)
            assert np.array_equal(gi, ri) and np.array_equal(bits(gd), bits(rd)), (trial, nq, nt, scale, k, fma, qs)
        n, md = ctx.statistical_outlier_removal(2, 1, mk, 1.0, fma=fma, return_dist=True)
        assert same_bits(md, O.mean_dist(t, mk, fma)[0]), (trial, nt, scale, mk, fma)
        n, cnt = ctx.radius_outlier_removal(2, 1, r, 1, fma=fma, return_counts=True)
        assert np.array_equal(cnt, O.neighbor_counts(t, r, fma)), (trial, nt, scale, r, fma)
        if log:
            log("trial %d: nq %d nt %d scale %g k %d mean_k %d radius %g fma %d ok" % (trial, nq, nt, scale, k, mk, r, fma))


# ------------------------------------------------------------------ the enlargement loop: 2M points in a cube

def _top_of_chunks(q, t, k, workers=8, chunk=8192):
    """the k smallest (plain d2, index) keys of every query over all of t, brute force in chunks of targets"""
    def part(c0):
        D = N.dist2_f32(q, t[c0:c0 + chunk])
        key = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(c0, c0 + D.shape[1], dtype=np.uint64)[None, :]
        kk = min(k, key.shape[1])
        return np.partition(key, kk - 1, axis=1)[:, :kk]
    with ThreadPoolExecutor(workers) as ex:
        parts = list(ex.map(part, range(0, len(t), chunk)))
    key = np.concatenate(parts, axis=1)
    key = np.partition(key, k - 1, axis=1)[:, :k]
    key.sort(axis=1)
    return key


def test_two_million_points_in_a_cube(ctx):
    """a uniform cube of 2M points with seq_cell_points = 1: the edge of the sizing formula gives 513^3 cells and the loop
    enlarges it until at most 32e6 remain.  2 000 of the points, uploaded as a query cloud, against a chunked brute force.
    The fma arm: a pair's fma d2 and plain d2 start from the same rounded differences and round three times each, so both lie
    within 3 * 2^-24 of the same exact sum and every entry of the fma top 64 has a plain d2 of at most (1 + 1e-6) times the
    plain 64th; the plain top 128 holds them all as long as its last entry is beyond that bound, which is asserted."""
    rng = np.random.default_rng(2000000)
    n = 2000000
    t = W.cloud(rng.uniform(0.0, 100.0, (n, 3)) + [-50.0, -50.0, 850.0])
    sample = np.sort(rng.choice(n, 2000, replace=False))
    q = np.ascontiguousarray(t[sample])
    t0 = time.time()
    key = _top_of_chunks(q, t, 128)
    ri = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rd = (key >> np.uint64(32)).astype(np.uint32).view(F32)
    assert (rd[:, 127].astype(F64) > rd[:, 63].astype(F64) * (1.0 + 1e-6)).all()
    fd = O.d2_f32(q[:, None, :3], t[ri.astype(np.int64), :3], True)
    fkey = (fd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ri.astype(np.uint64)
    fkey.sort(axis=1)
    fi, fdd = (fkey & np.uint64(0xFFFFFFFF)).astype(np.uint32), (fkey >> np.uint64(32)).astype(np.uint32).view(F32)
    print("reference: %.1f s" % (time.time() - t0))
    assert (ri[:, 0] == sample).all() and (rd[:, 0] == 0).all()
    try:
        ctx.tune(seq_cell_points=1)
        ctx.upload(0, q); ctx.upload(1, t)
        t0 = time.time()
        for k in W.KS:
            gi, gd = ctx.knn(0, 1, k)
            assert np.array_equal(gi, ri[:, :k]) and np.array_equal(bits(gd), bits(rd[:, :k])), k
            gi, gd = ctx.knn(0, 1, k, fma=True)
            assert np.array_equal(gi, fi[:, :k]) and np.array_equal(bits(gd), bits(fdd[:, :k])), (k, "fma")
        print("12 searches of 2 000 queries in 2M points (the first builds the grid): %.2f s" % (time.time() - t0))
        ni, nd = ctx.nn(0, 1)
        assert np.array_equal(ni, ri[:, 0]) and np.array_equal(bits(nd), bits(rd[:, 0]))
    finally:
        ctx.tune(seq_cell_points=4)
        ctx.clear(1)


# ------------------------------------------------------------------ non-finite points (mvr_hip.h N1 - N6)

def with_non_finite(p, count=60, seed=5):
    """the construction of test_non_finite_points_are_outliers (tests/test_gpu_outlier.py): `count` scattered points get NaN,
    +inf or -inf in one coordinate, some in two, one in all three"""
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


@pytest.fixture(scope="module")
def dirty20k(mvr):
    p, bad = with_non_finite(mvr.synth_view(mvr.synth_params(12, 2), 0, 20000))
    assert (~N.finite_mask(p)).sum() == 60
    return p, bad


def check_non_finite_lists(p_q, p_t, gi, gd, ri, rd, what):
    assert np.array_equal(gi, ri) and np.array_equal(bits(gd), bits(rd)), what
    fq, ft = N.finite_mask(p_q), N.finite_mask(p_t)
    # N2: a non-finite query gets nothing;  N1: a non-finite target is never listed;  N3: the tail counts finite points
    assert (gi[~fq] == NONE).all() and np.isposinf(gd[~fq]).all(), what
    listed = gi[gi != NONE]
    assert ft[listed].all(), what
    kk = min(gi.shape[1], int(ft.sum()))
    assert (gi[fq][:, :kk] != NONE).all() and (gi[fq][:, kk:] == NONE).all() and np.isposinf(gd[fq][:, kk:]).all(), what
    assert np.isfinite(gd[gi != NONE]).all()


@pytest.mark.parametrize("fma", [False, True])
def test_non_finite_points_knn(ctx, dirty20k, fma):
    """the 20k view with 60 non-finite points against itself and a clean query cloud / a dirty query cloud against it, k = 1, 8
    and 17: bit-identical to the reference with the rule, which the assertions of check_non_finite_lists restate one by one"""
    p, bad = dirty20k
    clean = p[N.finite_mask(p)][:3000]
    dirty_q = np.ascontiguousarray(p[np.concatenate([bad[:30], np.arange(0, 3000)])])
    ctx.upload(0, p)
    ref = N.knn_brute(p, p, 17, fma=fma)
    for k in (1, 8, 17):
        gi, gd = ctx.knn(0, 0, k, fma=fma)
        check_non_finite_lists(p, p, gi, gd, ref[0][:, :k], ref[1][:, :k], ("self", k))
    for q in (clean, dirty_q):
        ctx.upload(1, q)
        ref = N.knn_brute(q, p, 17, fma=fma)
        for k in (1, 8, 17):
            gi, gd = ctx.knn(1, 0, k, fma=fma)
            check_non_finite_lists(q, p, gi, gd, ref[0][:, :k], ref[1][:, :k], ("cross", k))
    # the other way round: a clean target searched by the dirty cloud
    ctx.upload(1, clean)
    gi, gd = ctx.knn(0, 1, 8, fma=fma)
    ref = N.knn_brute(p, clean, 8, fma=fma)
    check_non_finite_lists(p, clean, gi, gd, ref[0], ref[1], "dirty queries, clean target")


@pytest.mark.parametrize("fma", [False, True])
def test_non_finite_points_without_a_grid_and_without_a_finite_point(ctx, fma):
    """the same rule where there is no grid (fewer than 4 points), where fewer than k finite points exist, and where no point
    is finite at all (the grid is refused and the target counts as empty)"""
    rng = np.random.default_rng(8)
    few = W.cloud(rng.standard_normal((3, 3)) + [0, 0, 900]); few[1, 1] = np.nan
    ten = W.cloud(rng.standard_normal((10, 3)) + [0, 0, 900]); ten[[0, 2, 3, 5, 6, 8, 9], 0] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf]
    none = np.full((50, 4), np.nan, F32); none[::2, 0] = np.inf; none[::3, 1] = -np.inf
    q = W.cloud(rng.standard_normal((40, 3)) + [0, 0, 900]); q[7, 2] = np.inf
    for t in (few, ten, none):
        for qq, qs in ((t, 1), (q, 0)):
            ctx.upload(0, q); ctx.upload(1, t)
            for k in (1, 4, 9):
                gi, gd = ctx.knn(qs, 1, k, fma=fma)
                ri, rd = N.knn_brute(qq, t, k, fma=fma)
                check_non_finite_lists(qq, t, gi, gd, ri, rd, (len(t), qs, k))
    assert int(N.finite_mask(ten).sum()) == 3 and not N.finite_mask(none).any()


def check_non_finite_normals(p, nrm, curv, ref, rc, w, what):
    fin = N.finite_mask(p)
    assert np.isnan(nrm[~fin, :3]).all() and np.isnan(curv[~fin]).all(), what                  # N4, first half
    compare_normals(nrm, curv, ref, rc, w, p, 0.01, what)
    assert np.isfinite(nrm[~np.isnan(ref[:, 0])]).all(), what                                     # N4: no non-finite neighbour got in


@pytest.mark.parametrize("fma", [False, True])
def test_non_finite_points_normals(ctx, dirty20k, fma):
    """k mode and radius mode with curvature on the dirty 20k view; then one call over four slots: the dirty view, a slot that
    is all NaN, one with fewer than 4 finite points and one too small for a grid"""
    p, bad = dirty20k
    ctx.upload(0, p)
    ri, _ = N.knn_brute(p, p, 16, fma=fma)
    curv = ctx.estimate_normals(0, k=16, curvature=True, fma=fma)
    check_non_finite_normals(p, ctx.download_normals(0), curv, *N.normals_from_lists(p, ri), ("k", fma))
    curv = ctx.estimate_normals(0, radius=1.0, curvature=True, fma=fma)
    check_non_finite_normals(p, ctx.download_normals(0), curv, *N.normals_from_sets(p, *N.radius_sets(p, 1.0, fma=fma)), ("radius", fma))
    rng = np.random.default_rng(9)
    all_nan = np.full((300, 4), np.nan, F32)
    three = W.cloud(rng.standard_normal((40, 3)) + [0, 0, 900]); three[3:, rng.integers(0, 3, 37)] = np.nan
    tiny = W.cloud(rng.standard_normal((3, 3)) + [0, 0, 900]); tiny[2, 0] = -np.inf
    clouds = [p, all_nan, three, tiny]
    assert int(N.finite_mask(three).sum()) == 3
    for mode in (dict(k=16), dict(radius=1.0), dict(k=3), dict(radius=50.0)):
        for s, c in enumerate(clouds):
            ctx.upload(10 + s, c)
        curvs = ctx.estimate_normals([10, 11, 12, 13], curvature=True, fma=fma, **mode)
        for s, c in enumerate(clouds):
            nrm = ctx.download_normals(10 + s)
            if "k" in mode:
                ref = N.normals_from_lists(c, N.knn_brute(c, c, mode["k"], fma=fma)[0])
            else:
                if s == 0 and mode["radius"] > 5:
                    continue                        # (the reference's sets on 20k points at 50 mm are the cloud squared)
                ref = N.normals_from_sets(c, *N.radius_sets(c, mode["radius"], fma=fma))
            check_non_finite_normals(c, nrm, curvs[s], *ref, (mode, s, fma))
            if s == 1:
                assert np.isnan(nrm[:, :3]).all() and np.isnan(curvs[s]).all()
        # three finite points and k = 3 or a wide ball: they do have a normal, made of the three of them
        if mode in (dict(k=3), dict(radius=50.0)):
            assert np.isfinite(ctx.download_normals(12)[:3, :3]).all()


def test_non_finite_queries_walk_nothing(ctx, mvr):
    """N5: 2 000 NaN points in a 200k view.  A NaN query that walked the grid until its list were full would visit every cell
    -- millions of dependent lookups per thread, seconds per launch -- where the search of the clean view takes milliseconds
    (both times are printed).  The bar for the dirty search is one second, host copies included: far above the one, far
    below the other, so that a loaded machine does not trip it."""
    v = mvr.synth_view(mvr.synth_params(12, 2), 0, 200000)
    d = v.copy()
    d[np.random.default_rng(3).choice(len(v), 2000, replace=False), 1] = np.nan
    times = []
    for p in (v, d):
        ctx.upload(0, p)
        ctx.knn(0, 0, 16)                                  # builds the grid
        t0 = time.time()
        gi, gd = ctx.knn(0, 0, 16)
        ctx.estimate_normals(0, k=16)
        times.append(time.time() - t0)
    print("knn + normals at k = 16 on 200k points: clean %.4f s, with 2 000 NaN points %.4f s" % tuple(times))
    fin = N.finite_mask(d)
    assert (gi[~fin] == NONE).all() and fin[gi[fin]].all()
    assert times[1] <= 1.0


# ------------------------------------------------------------------ the margin of the stopping bound, where it is needed

def test_a_neighbour_rounded_into_the_next_cell(ctx):
    """walk_cases.boundary_case: the nearest point P is assigned to the unvisited cell c by the f32 cell arithmetic while it
    lies 1.2e-5 cells on the near side of that cell's boundary, and the runner-up A, in the query's own cell, is farther than
    P but nearer than the boundary less 1e-6 cells and the 1e-5 of d2.  A stopping bound without its margin for the cell
    assignment's rounding returns A.  The preconditions are asserted here in the kernel's own arithmetic; then k-NN across,
    k-NN and the mean distance with the query inside the cloud, at every k, bit for bit."""
    q, t, f = W.boundary_case()
    inv_h = f["inv_h"]
    assert W.grid_edge(t) == f["h64"] and t[:, 0].min() == 0                       # the grid the library will build
    cell = lambda x: int(np.floor(F32(F32(x) * inv_h)))
    P, A = t[f["iP"]], t[f["iA"]]
    assert cell(P[0]) == f["c"] and cell(q[0, 0]) == cell(A[0]) == f["c"] - 1      # P in the unvisited cell, A in the query's
    assert float(P[0]) * float(inv_h) < f["c"]                                     # ... though P lies before the boundary
    ri, rd = N.knn_brute(q, t, 64)
    assert ri[0, 0] == f["iP"] and ri[0, 1] == f["iA"]
    assert float(rd[0, 0]) < float(rd[0, 1]) < f["b_plain"] ** 2 * (1.0 - 1.0e-5)  # a bound without the margin stops at A
    ctx.upload(0, q); ctx.upload(1, t)
    for fma in (False, True):
        check_knn(ctx, 0, 1, N.knn_brute(q, t, 64, fma=fma), W.KS, fma, "boundary, cross")
    both = np.concatenate([t, q])
    ctx.upload(1, both)
    for fma in (False, True):
        ref = N.knn_brute(both, both, 64, fma=fma)
        assert ref[0][-1, 0] == len(t) and ref[0][-1, 1] == f["iP"]
        check_knn(ctx, 1, 1, ref, (1, 2, 9, 17), fma, "boundary, self")
        for k in (1, 2, 9):
            n, md = ctx.statistical_outlier_removal(2, 1, k, 1.0, fma=fma, return_dist=True)
            assert same_bits(md, O.mean_dist(both, k, fma)[0]), ("boundary, mean_dist", k, fma)


@pytest.mark.parametrize("fma", [False, True])
def test_finite_points_whose_distance_overflows(ctx, fma):
    """N1, second sentence: two groups of finite points 3e19 apart -- the f32 d2 between them is +inf, so they are not
    neighbours of each other: lists end in UINT32_MAX / +inf after the own group, with a grid (8 points) and without (3)"""
    rng = np.random.default_rng(19)
    for n in (4, 2):
        a = W.cloud(rng.standard_normal((n, 3)))
        b = W.cloud(rng.standard_normal((n - 1, 3)) + [3.0e19, 0.0, 0.0])
        t = np.concatenate([a, b])
        ctx.upload(0, t)
        gi, gd = ctx.knn(0, 0, 6, fma=fma)
        ri, rd = N.knn_brute(t, t, 6, fma=fma)
        assert np.array_equal(gi, ri) and np.array_equal(bits(gd), bits(rd)), n
        assert (gi[:n, :n] < n).all() and (gi[:n, n:] == NONE).all() and (gi[n:, n - 1:] == NONE).all() and np.isposinf(gd[:n, n:]).all()
