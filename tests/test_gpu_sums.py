"""GPU tests of the f64 sum kernels of csrc/mvr_reduce.hip (pass1 / pass2, moments2, accept_moments2 and its batched by-position
form, p2plane, fitness) and the machinery of csrc/mvr_block_sums.h they share, against independent references.

EXACT TIER.  On the lattice pairs of tests/sum_cases.py every term of every sum is an integer and every partial sum is below 2^53
(tests/test_sum_cases_host.py proves it), so the f64 result is the same in every order of addition and must equal plain integer
arithmetic on the accepted set the construction states: `same()` compares the bit patterns of the doubles, nothing else.  That
holds on every route -- every search mode, fma on or off, one pair, the batch, the ring step, any reduce_rows, any split into
sub-ranges or ranks.

BOUNDED TIER.  Where integers cannot reach (the centred covariance, real scan data) the reference is math.fsum over the terms as
the kernels form them ((double)p - o, then f64 products, -ffp-contract=off: numpy's terms are the kernel's bit for bit), which is
the exactly rounded sum s of those n terms t_i.  Any order of n - 1 rounded additions gives a result within
(n - 1) u / (1 - (n - 1) u) * sum |t_i| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4), u = 2^-53, and that
is <= n u sum |t_i| whenever n (n - 1) u <= 1; the reference's own rounding (u |s|) is inside the slack between the two.  So
    |got - ref| <= n * 2^-53 * sum |t_i|        per column,
about 1e-11 sum |t_i| at the largest size, while one lost term is about sum |t_i| / n.  For sigma, whose terms are taken about the
two means and whose sum is divided by n, the effect of the two rounded means, 2^-53 (|m_p| sum |q - m_q| + |m_q| sum |p - m_p|), is
added and everything divided by n (the division's own rounding, 2^-53 |ref|, is far inside the first term).  Every bounded test prints
its worst ratio |got - ref| / bound; it must be below 1.  The bounds come from the references, never from the device."""
import numpy as np
import pytest

import reject_cases as RC
import sum_cases as SC
import sum_ref as SR
import walk_cases as WC

pytestmark = pytest.mark.gpu

S, T_, E_ = 20, 21, 22
U = 2.0 ** -53
DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def ctx(mvr):
    with mvr.Context(0) as c:
        yield c


def n_cu_of(c):
    return c.device_info()[1]


def row29(m2):
    return np.array([m2.n] + list(m2.sp) + list(m2.sq) + list(m2.spp) + list(m2.sqq) + list(m2.spq) + [m2.sum_d2], np.float64)


def table29(row32):
    r = np.asarray(row32, np.float64)
    return np.concatenate([r[:1], r[4:32]])


def same(got, ints):
    """the doubles are the integers, bit for bit (a zero is +0.0)"""
    got = np.ascontiguousarray(got, np.float64)
    return np.array_equal(got.view(np.uint64), np.asarray(ints, np.int64).astype(np.float64).view(np.uint64))


def same_f(got, want):
    return np.array_equal(np.ascontiguousarray(got, np.float64).view(np.uint64), np.ascontiguousarray(want, np.float64).view(np.uint64))


def load(c, case, s=S, t=T_):
    c.upload(s, case["src"])
    c.upload(t, case["tgt"])


def check_pair(c, case, what):
    for rec in (False, True):
        for fma in (False, True):
            got = row29(c.pair_moments2(S, T_, case["max_dist"], case["origin"], reciprocal=rec, fma=fma))
            assert same(got, case["sums"][rec]), (what, rec, fma, got - case["sums"][rec])


# ------------------------------------------------------------------------------------------------------------ exact tier
MODE_NAMES = SC.SMALL_NAMES + ("rowcap-1", "rowcap+1", "empty")
OWN = [(n, "near") for n in SC.LARGE_NAMES if n not in MODE_NAMES] + [("all_rows", "near")] + \
      [(n, "far") for n in SC.SMALL_NAMES + SC.LARGE_NAMES] + [(n, "far0") for n in SC.FAR0_NAMES]


@pytest.mark.parametrize("name", MODE_NAMES)
def test_pair_moments2_in_every_search_mode(gpu, name):
    """brute force reduces through the compacted reverse list, the culled modes through qperm and tinv"""
    case = SC.case(name, "near", n_cu_of(gpu))
    load(gpu, case)
    check_pair(gpu, case, (name, gpu.mode))


@pytest.mark.parametrize("name,frame", OWN)
def test_pair_moments2_at_every_size_and_frame(ctx, name, frame):
    case = SC.case(name, frame, n_cu_of(ctx))
    load(ctx, case)
    check_pair(ctx, case, (name, frame))


def positions(c, n, slot=S):
    """source index -> position in the walk of slot `slot` (after a search has run on it)"""
    order = np.arange(n)
    if c.mode != "brute":
        order = c.debug_order(slot)
        assert order is not None and np.array_equal(np.sort(order), np.arange(n))
    position = np.empty(n, np.int64)
    position[order.astype(np.int64)] = np.arange(n)
    return position


def splits(n, seed=3):
    fixed = [(0, 1), (1, 255), (256, 1), (257, n - 257)]
    cut = np.sort(np.random.default_rng(seed).choice(np.arange(1, n), 4, replace=False))
    edges = [0] + cut.tolist() + [n]
    return fixed, [(a, b - a) for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("name", ["257", "rowcap+1", "blockcap"])
def test_sub_ranges_are_exact_and_add_up(gpu, name):
    """a sub-range is a range of the walk's positions (include/mvr_hip.h at mvr_pair_moments2): of the source's indices under the
    brute-force search, of the context's ordering of the source (debug_order: position -> index, a permutation) under the culled
    one.  Each range's row is the exact sum over ITS queries, and the rows of a split add up to the whole."""
    case = SC.case(name, "near", n_cu_of(gpu))
    load(gpu, case)
    n = len(case["src"])
    for rec in (False, True):
        q, m, d = case["accepted"][rec]
        whole = row29(gpu.pair_moments2(S, T_, case["max_dist"], case["origin"], reciprocal=rec))
        assert same(whole, case["sums"][rec])
        position = positions(gpu, n)
        for parts in splits(n):
            total = np.zeros(29)
            for b, cnt in parts:
                got = row29(gpu.pair_moments2(S, T_, case["max_dist"], case["origin"], reciprocal=rec, q_begin=b, q_count=cnt))
                k = (position[q] >= b) & (position[q] < b + cnt)
                assert same(got, SR.exact_sums(case["src"][q[k]], case["tgt"][m[k]], d[k], case["origin"])), (name, rec, b, cnt)
                total += got
            assert same(total, case["sums"][rec]), (name, rec)


@pytest.mark.parametrize("name,frame", [("3", "near"), ("65", "near"), ("257", "near"), ("rowcap+1", "near"), ("blockcap", "near"), ("257", "far"),
                                        ("4097", "far0")])
def test_pair_moments2_from_corr(ctx, name, frame):
    """the entry scatters the list into match[]: its order must not matter; no keys, so the sum of d2 stays 0"""
    case = SC.case(name, frame, n_cu_of(ctx))
    load(ctx, case)
    rng = np.random.default_rng(11)
    origins = [case["origin"]] + ([np.array(SC.FRAMES["far"][1], np.float64), np.zeros(3)] if len(case["src"]) <= SC.FAR0_MAX else [])
    for rec in (False, True):
        q, m, d = case["accepted"][rec]
        for origin in origins:
            want = SR.exact_sums(case["src"][q], case["tgt"][m], np.zeros(len(q)), origin)
            assert SR.abs_sums(case["src"][q], case["tgt"][m], d, origin).max(initial=0.0) < 2.0 ** 53
            for order in (np.arange(len(q)), np.arange(len(q))[::-1], rng.permutation(len(q))):
                m2 = ctx.pair_moments2_from_corr(S, T_, q[order], m[order], origin)
                assert same(row29(m2), want) and same_f(list(m2.origin), origin), (name, frame, rec, origin)


@pytest.mark.parametrize("name", ["257", "rowcap+1"])
def test_pair_moments2_batch(gpu, name):
    """(s, t), (t, s), a self pair, a repeated pair and an empty cloud on either side, three times over in rotated order: 18 pairs.
    The fused batch runs its pairs in G = pair_groups groups -- group 0 on the context's stream, the others on worker streams with
    work buffers and partial rows of their own -- only when n_pairs >= 4 * pair_groups (mvr_pair_moments2_batch in csrc/mvr_ctx.hip;
    the two other conditions there, pose_from_table and single_group, are set inside a ring run alone), so 18 pairs reach G = 2
    (9 + 9) and G = 4 (4 + 5 + 4 + 5) and the rotation puts every kind of pair into a worker's group.  No counter tells which path
    ran; the condition above is the argument.  Under the brute-force search every pair runs on a worker stream whatever the key.
    After a fused batch the lists of a pair of the LAST group are read back too (mvr_pair_batch_correspondences)."""
    case = SC.case(name, "near", n_cu_of(gpu))
    load(gpu, case)
    gpu.clear(E_)
    n = len(case["src"])
    zero = np.zeros(29, np.int64)
    six = [(S, T_), (T_, S), (S, S), (S, T_), (E_, T_), (S, E_)]
    sub = (1, 255)
    assert same(row29(gpu.pair_moments2(S, T_, case["max_dist"], case["origin"])), case["sums"][True])
    position = positions(gpu, n)                                            # (a sub-range is a range of these: test_sub_ranges_...)
    turn = [(e + r) % 6 for r in range(3) for e in range(6)]               # which of the six is pair k
    pairs = [six[e] for e in turn]
    assert len(pairs) >= 4 * 4
    try:
        for groups in (1, 2, 4):
            gpu.tune(pair_groups=groups)
            for rec in (False, True):
                q, m, d = case["accepted"][rec]
                k = (position[q] >= sub[0]) & (position[q] < sub[0] + sub[1])
                want = [case["sums"][rec], SC.swapped(case)[3], SC.self_pair(case)[3], case["sums"][rec], zero, zero]
                part = SR.exact_sums(case["src"][q[k]], case["tgt"][m[k]], d[k], case["origin"])
                six_ranges = [(0, None), (0, None), (0, n), sub, (0, None), (0, 5)]
                for ranges, exp in ((None, want), (six_ranges, want[:3] + [part, zero, zero])):
                    rows = gpu.pair_moments2_batch(pairs, case["max_dist"], case["origin"], reciprocal=rec,
                                                   ranges=None if ranges is None else [ranges[e] for e in turn])
                    assert len(rows) == len(pairs)
                    for e, got in zip(turn, rows):
                        assert same(row29(got), exp[e]), (name, gpu.mode, groups, rec, ranges is not None, e)
                    if gpu.mode != "brute" and ranges is None:
                        last = max(i for i, e in enumerate(turn) if e == 0)   # an (s, t) pair of the last group
                        assert last >= len(pairs) * 3 // 4
                        lq, lm, ld = gpu.pair_batch_correspondences(last, n)
                        assert np.array_equal(lq, q) and np.array_equal(lm, m) and np.array_equal(ld.view(np.uint32), d.view(np.uint32))
    finally:
        gpu.tune(pair_groups=2)


def test_reduce_rows(ctx):
    """1, 2, 7, 8, 9, 33 rows on the 256 R + 1 case (one row, fewer than the 8 row groups, exactly 8, one more, more than 4 per
    group), and all kMaxBlocks = 1024 rows on the 64^3 case"""
    try:
        case = SC.case("rowcap+1", "near", n_cu_of(ctx))
        load(ctx, case)
        for rows in (1, 2, 7, 8, 9, 33, 1024):
            ctx.tune(reduce_rows=rows)
            check_pair(ctx, case, ("reduce_rows", rows))
        case = SC.case("all_rows", "near", n_cu_of(ctx))
        assert len(case["src"]) >= 1024 * 256 - 255
        load(ctx, case)
        ctx.tune(reduce_rows=1024)
        for rec in (False, True):
            assert same(row29(ctx.pair_moments2(S, T_, case["max_dist"], case["origin"], reciprocal=rec)), case["sums"][rec]), rec
    finally:
        ctx.tune(reduce_rows=0)


@pytest.fixture(scope="module")
def ring(ctx):
    """three lattice views under exact poses: view 0 = the target under the identity, view 1 = a source under a quarter turn about z
    through an integer pivot, view 2 = a second source under an integer translation; the posed points are the integers again"""
    c1, c2 = SC.ring_views(n_cu_of(ctx))
    world = [c1["tgt"], c1["src"], c2["src"]]
    poses = [SC.translation((0.0, 0.0, 0.0)), SC.quarter_turn((192, 160)), SC.translation((24.0, -40.0, 16.0))]
    raw = [SC.unposed(w, T) for w, T in zip(world, poses)]
    edges = [(1, 0), (2, 0), (0, 1), (0, 2)]
    want = [c1["sums"][True], c2["sums"][True], SC.swapped(c1)[3], SC.swapped(c2)[3]]
    want_one_way = [c1["sums"][False], c2["sums"][False], SC.swapped(c1)[3], SC.swapped(c2)[3]]
    return dict(world=world, poses=poses, raw=raw, edges=edges, want={True: want, False: want_one_way}, origin=c1["origin"], max_dist=c1["max_dist"])


def test_ring_step_rows(mvr, ctx, ring):
    V = 3
    posed, raw = list(range(V)), [V + v for v in range(V)]
    for v in range(V):
        ctx.upload(V + v, ring["raw"][v])
    for rec in (True, False):
        new, info = ctx.ring_step(posed, raw, ring["edges"], ring["poses"], ring["max_dist"], ring["origin"], reciprocal=rec, steps=1)
        for v in range(V):
            assert np.array_equal(ctx.download(v).view(np.uint32), ring["world"][v].view(np.uint32)), v
        for e, w in enumerate(ring["want"][rec]):
            assert same(table29(info["rows"][e]), w), (rec, e, table29(info["rows"][e]) - w)
            n, sd2 = float(w[0]), float(w[28])
            assert info["pair_n"][e] == n
            assert same_f([info["pair_mse"][e]], [sd2 * (1.0 / n)]), (rec, e)     # moments_from_moments2: an exact integer times the rounded 1 / n
    assert np.isfinite(np.asarray(new)).all()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_ring_rows_of_all_ranks_add_up_exactly(ctx, ring, world):
    V = 3
    posed, raw = list(range(V)), [V + v for v in range(V)]
    for v in range(V):
        ctx.upload(V + v, ring["raw"][v])
    total = np.zeros((len(ring["edges"]), 32))
    for rank in range(world):
        total += ctx.ring_rows_sharded(rank, world, posed, raw, ring["edges"], ring["poses"], ring["max_dist"], ring["origin"])
    for e, w in enumerate(ring["want"][True]):
        assert same(table29(total[e]), w), (world, e)


@pytest.mark.parametrize("name,frame", [("3", "near"), ("65", "near"), ("257", "near"), ("rowcap+1", "near"), ("blockcap", "near"), ("blockcap", "far")])
def test_pair_moments_counts_means_and_mse(gpu, name, frame):
    """n, the two means and the mse are one correctly rounded division of exact integers; sigma is in the bounded tier"""
    case = SC.case(name, frame, n_cu_of(gpu))
    load(gpu, case)
    worst = 0.0
    for rec in (False, True):
        q, m, d = case["accepted"][rec]
        ints = SR.exact_sums(case["src"][q], case["tgt"][m], d, np.zeros(3))
        n = float(len(q))
        pm = gpu.pair_moments(S, T_, case["max_dist"], reciprocal=rec)
        assert pm.n == n
        assert same_f(list(pm.mean_src), [float(v) / n for v in ints[1:4]]) and same_f(list(pm.mean_tgt), [float(v) / n for v in ints[4:7]])
        assert same_f([pm.mse], [float(ints[28]) / n])
        worst = max(worst, sigma_ratio(pm, case["src"][q], case["tgt"][m], exact=True))
    print("%s/%s %s: sigma, worst |got - ref| / bound = %.3g" % (name, frame, gpu.mode, worst))
    assert worst < 1.0


def nearest_d2(case):
    """the squared distance of every source point to its nearest target: the construction's, and the corner's for an orphan"""
    corner = case["tgt_int"].min(0)
    far = ((case["src_int"] - corner) ** 2).sum(1)
    return np.where(case["host"] >= 0, case["d2_int"], far)


@pytest.mark.parametrize("name,frame", [("3", "near"), ("65", "near"), ("257", "near"), ("blockcap", "near"), ("blockcap", "far")])
def test_fitness(gpu, name, frame):
    """the source arrives under an integer translation (exact in the f32 transform); max_range above every d2, equal to one d2
    (<= keeps it) and negative (nothing is left: DBL_MAX)"""
    case = SC.case(name, frame, n_cu_of(gpu))
    t = np.array([16.0, -8.0, 24.0])
    moved = case["src"].copy()
    moved[:, :3] -= t.astype(np.float32)
    gpu.upload(S, moved)
    gpu.upload(T_, case["tgt"])
    d2 = nearest_d2(case)
    assert d2.max() < 2 ** 24                                                # every d2 is exact in f32
    for max_range in (float(d2.max()) + 1.0, float(d2.max()), 16.0, 12.0, 0.0, -1.0):
        got = gpu.fitness(S, T_, SC.translation(t).astype(np.float32), max_range=max_range)
        total, count = SR.exact_fitness(d2, max_range)
        want = float(total) / float(count) if count else DBL_MAX
        assert same_f([got], [want]), (name, frame, gpu.mode, max_range, got, want)


@pytest.mark.parametrize("name", ["3", "65", "257", "rowcap+1", "blockcap"])
def test_icp_align_counts_and_mse(mvr, gpu, name):
    case = SC.case(name, "near", n_cu_of(gpu))
    load(gpu, case)
    for rec in (False, True):
        q, m, d = case["accepted"][rec]
        n, sd2 = len(q), int(case["sums"][rec][28])
        prm = mvr.icp_params(reciprocal=rec, max_dist=case["max_dist"], max_iter=1)
        T, st, rc = gpu.icp_align(S, T_, -1, prm)
        T2, st2, rc2, trace = gpu.icp_align_rejected(S, T_, -1, prm, [], return_trace=True)
        assert st["n_corr"] == st2["n_corr"] == n and trace[0]["n_corr"] == n
        # (n_found is what the search found before the chain, mvr_hip.h at mvr_icp_iter_trace: the one-way count of a one-way
        # search, the reciprocal count of a reciprocal one)
        assert trace[0]["n_found"] == n
        if n < 3:
            assert rc == rc2 == mvr.E_NOCORR
            continue
        assert rc == rc2 == 0 and st["iterations"] == st2["iterations"] == 1
        assert same_f([st["mse"]], [float(sd2) / float(n)]) and same_f([st2["mse"]], [float(sd2) / float(n)]) and same_f([trace[0]["mse"]], [st2["mse"]])


# ---------------------------------------------------------------------------------------------------------- bounded tier
def sigma_ratio(pm, p, q, exact=False):
    """worst |sigma - ref| / bound over the 9 entries (module docstring); exact: the points are integers, and the reference is the
    rational value about the exact means"""
    n = len(p)
    s, a, mp, mq, ap, aq = SR.fsum_centred(p, q)
    got = np.array(pm.sigma)
    ref = s / n
    if exact:
        ref = np.array([float(v / n) for v in SR.exact_centred(p, q)])
    bound = np.empty(9)
    for r in range(3):
        for c in range(3):
            k = 3 * r + c
            bound[k] = (n * U * a[k] + U * (abs(mp[c]) * aq[r] + abs(mq[r]) * ap[c])) / n
    ok = bound > 0
    assert (got[~ok] == ref[~ok]).all()
    return float((np.abs(got - ref)[ok] / bound[ok]).max()) if ok.any() else 0.0


def sums_ratio(got, ref, tot, n):
    bound = n * U * tot
    ok = bound > 0
    assert (got[~ok] == ref[~ok]).all()
    return float((np.abs(got - ref)[ok] / bound[ok]).max()) if ok.any() else 0.0


@pytest.fixture(scope="module")
def synth(mvr):
    return RC._synth_pair(mvr, 4097, 4097)


def shifted(cloud, far):
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) + WC.FAR_DIR * far).astype(np.float32)
    return out


@pytest.mark.parametrize("far", [0.0, 1e5, 1e6])
def test_synthetic_pair_against_fsum(mvr, gpu, synth, far):
    """pair_moments (the two-pass sigma) and pair_moments2 (origin at the clouds' pivot and at 0) on 4 097-point scans, where they
    lie and moved 1e5 and 1e6 mm along walk_cases.FAR_DIR.  The far frame with origin 0 shows how much of moments_from_moments2's
    covariance survives the cancellation: printed, not asserted."""
    src, tgt = shifted(synth["src"], far), shifted(synth["tgt"], far)
    gpu.upload(S, src)
    gpu.upload(T_, tgt)
    pivot = np.array([0.0, 0.0, 900.0]) + WC.FAR_DIR * far
    worst_sigma = worst_sums = worst_means = 0.0
    for rec in (False, True):
        q, m, d = gpu.correspondences(S, T_, 4.0, reciprocal=rec)
        n = len(q)
        assert n > 1000
        pm = gpu.pair_moments(S, T_, 4.0, reciprocal=rec)
        assert pm.n == n
        mp, mq = SR.means(src[q], tgt[m])
        ap, aq = np.abs(src[q, :3].astype(np.float64)).sum(0), np.abs(tgt[m, :3].astype(np.float64)).sum(0)
        for got, ref, tot in ((pm.mean_src, mp, ap), (pm.mean_tgt, mq, aq)):      # a mean: the column's sum over n, so the bound over n
            worst_means = max(worst_means, float((np.abs(np.array(got) - ref) / (n * U * tot / n)).max()))
        worst_sigma = max(worst_sigma, sigma_ratio(pm, src[q], tgt[m]))
        for origin in (pivot, np.zeros(3)):
            m2 = gpu.pair_moments2(S, T_, 4.0, origin, reciprocal=rec)
            ref, tot = SR.fsum_sums(src[q], tgt[m], d, origin)
            got = row29(m2)
            assert got[0] == n
            worst_sums = max(worst_sums, sums_ratio(got, ref, tot, n))
            derived = np.array(mvr.moments_from_moments2(m2).sigma)
            rel = np.abs(derived - np.array(pm.sigma)).max() / np.abs(np.array(pm.sigma)).max()
            print("far %g, origin %s, reciprocal %d: sigma from the raw moments differs from the two-pass sigma by %.3g of its largest entry"
                  % (far, "0" if not origin.any() else "pivot", rec, rel))
    print("far %g %s: worst |got - ref| / bound: sigma %.3g, the 29 sums %.3g, the two means %.3g" % (far, gpu.mode, worst_sigma, worst_sums, worst_means))
    assert worst_sigma < 1.0 and worst_sums < 1.0 and worst_means < 1.0


def test_ring_rows_on_synthetic_views_against_fsum(mvr, ctx):
    V, N = 3, 4097
    sp = mvr.synth_params(12, 1)
    piv, ax = mvr.synth_prior(sp)
    scans = [mvr.synth_view(sp, v, N) for v in range(V)]
    poses = [mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, 12)) for v in range(V)]
    edges = [(0, 1), (1, 2), (2, 0)]
    posed, raw = list(range(V)), [V + v for v in range(V)]
    for v in range(V):
        ctx.upload(V + v, scans[v])
    worst = 0.0
    for origin in (np.asarray(piv, np.float64), np.zeros(3)):
        new, info = ctx.ring_step(posed, raw, edges, poses, 8.0, origin, steps=1)
        clouds = [ctx.download(v) for v in range(V)]
        for e, (s, t) in enumerate(edges):
            q, m, d = ctx.pair_batch_correspondences(e, N)
            n = len(q)
            assert n == info["rows"][e][0] and n > 100
            ref, tot = SR.fsum_sums(clouds[s][q], clouds[t][m], d, origin)
            worst = max(worst, sums_ratio(table29(info["rows"][e]), ref, tot, n))
    print("ring rows on synthetic views: worst |got - ref| / bound = %.3g" % worst)
    assert worst < 1.0


@pytest.mark.parametrize("name", SC.PLANE_NAMES + ("3",))
def test_point_to_plane_against_the_exact_solution(mvr, gpu, name):
    """icp_align(point_to_plane, one iteration) on the lattice with axis-aligned unit normals: A^T A and A^T b are integers, solved
    exactly in rationals (sum_ref.plane_expectation, which also states the allowance).  Three source points keep two
    correspondences: the align refuses them (and three rows could not fill the 6 x 6 system either: tests/test_sum_cases_host.py)."""
    case = SC.case(name, "near", n_cu_of(gpu))
    load(gpu, case)
    nrm = SC.axis_normals(len(case["tgt"]))
    gpu.upload_normals(T_, nrm)
    worst = 0.0
    for rec in (False, True):
        q, m, d = case["accepted"][rec]
        T, st, rc = gpu.icp_align(S, T_, -1, mvr.icp_params(reciprocal=rec, max_dist=case["max_dist"], max_iter=1, point_to_plane=True))
        assert st["n_corr"] == len(q)
        if name == "3":
            assert rc == mvr.E_NOCORR
            continue
        want, allow, cond, x = SR.plane_expectation(case["src"][q], case["tgt"][m], nrm[m])
        assert rc == 0 and same_f([st["mse"]], [float(case["sums"][rec][28]) / float(len(q))])
        err = np.abs(T.astype(np.float64) - want.astype(np.float64))
        assert np.array_equal(T[3], [0, 0, 0, 1])
        worst = max(worst, float((err[:3] / allow[:3]).max()))
        assert (err <= allow).all(), (name, rec, cond, err / np.maximum(allow, 1e-300))
    print("%s %s: point-to-plane, worst |T - exact| / allowance = %.3g" % (name, gpu.mode, worst))


@pytest.mark.parametrize("name", ["sheet", "row", "identical", "three", "mirrored"])
def test_degenerate_lists(mvr, ctx, name):
    """pair_moments2_from_corr -> moments_from_moments2 -> umeyama_from_moments, whose svd3 has hand-written rank-1 and rank-2 branches"""
    p, q = SC.degenerate_lists()[name]
    ctx.upload(S, p)
    ctx.upload(T_, q)
    idx = np.arange(len(p), dtype=np.int32)
    for origin in (np.zeros(3), np.array([0.0, 0.0, 896.0])):
        m2 = ctx.pair_moments2_from_corr(S, T_, idx, idx, origin)
        assert same(row29(m2), SR.exact_sums(p, q, np.zeros(len(p)), origin))
        T, sv = mvr.umeyama_from_moments(mvr.moments_from_moments2(m2))
        assert T is not None
        SR.check_rigid_fit(T, p, q, "%s about %s" % (name, origin.tolist()))
