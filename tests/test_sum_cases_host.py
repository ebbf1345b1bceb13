"""CPU tests of the inputs and references of tests/test_gpu_sums.py: the preconditions of tests/sum_cases.py proved on the
references alone (the constructed accepted sets against a kd-tree search with the lowest-index tie rule, no ties but the stated
ones, f32 round trips, every sum of absolute terms below 2^53), the fake reduction of tests/sum_ref.py against the integers, and
each of its five faults caught at a named size."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import sum_cases as SC
import sum_ref as SR

TWO53 = float(2 ** 53)
SEARCHED = [(n, "near") for n in SC.SMALL_NAMES + SC.LARGE_NAMES + ("empty",)] + [(n, "far") for n in SC.SMALL_NAMES + SC.LARGE_NAMES] + \
           [(n, "far0") for n in SC.FAR0_NAMES]
EVERY = SEARCHED + [("all_rows", "near")]


def nearest(tree_pts, queries, k=4):
    """lowest-index nearest neighbour of every query in tree_pts (integers: the distances are exact) -> (index, d2, tie)"""
    k = min(k, len(tree_pts))
    _, idx = cKDTree(tree_pts.astype(np.float64)).query(queries.astype(np.float64), k=k)
    idx = idx.reshape(len(queries), k)
    d2 = ((tree_pts[idx] - queries[:, None, :]) ** 2).sum(2)                # int64, exact
    best = d2.min(1)
    cand = np.where(d2 == best[:, None], idx, np.iinfo(np.int64).max)
    return cand.min(1), best, (d2 == best[:, None]).sum(1) > 1


@pytest.mark.parametrize("name,frame", SEARCHED)
def test_constructed_sets_equal_a_search(name, frame):
    check_search(SC.case(name, frame), name)


def test_ring_views_and_plane_case_hold_the_same_conditions():
    for c in SC.ring_views():
        check_search(c, "ring")
        for rec in (False, True):
            q, m, d = c["accepted"][rec]
            assert SR.abs_sums(c["src"][q], c["tgt"][m], d, c["origin"]).max() < TWO53
    check_search(SC.case("16"), "16")


def check_search(c, name):
    s, t, max2 = c["src_int"], c["tgt_int"], int(c["max_dist"] ** 2)
    assert np.array_equal(c["src"][:, :3].astype(np.float64), s) and np.array_equal(c["tgt"][:, :3].astype(np.float64), t)
    assert c["src"].dtype == np.float32 and max(np.abs(s).max(), np.abs(t).max()) < 2 ** 24
    j, d2, tie = nearest(t, s)
    ok = ~(d2 > max2)
    assert not tie[ok].any()                                                # no forward tie among the accepted
    q, m, d = c["accepted"][False]
    assert np.array_equal(np.nonzero(ok)[0], q) and np.array_equal(j[ok], m) and np.array_equal(d2[ok], d.astype(np.int64))
    assert name in ("1", "2", "3", "empty") or (d2[ok] == max2).sum() == 2  # the two points on the edge of the cap
    # reverse: the matched targets look for their nearest source point, the lower index on a tie
    hit = np.unique(j[ok])
    if len(hit):
        ri, rd2, rtie = nearest(s, t[hit])
        assert sorted(hit[rtie]) == sorted(w[0] for w in c["equal_winners"])    # the only ties are the stated equal rivals
        back = np.full(len(t), -1, np.int64)
        back[hit] = np.where(rd2 > max2, -1, ri)
        rec = ok & (back[np.where(ok, j, 0)] == np.arange(len(s)))
    else:
        rec = ok
    q, m, d = c["accepted"][True]
    assert np.array_equal(np.nonzero(rec)[0], q) and np.array_equal(j[rec], m) and np.array_equal(d2[rec], d.astype(np.int64))
    for tj, win, lose in c["equal_winners"]:
        assert win < lose and rec[win] and not rec[lose] and ok[lose] and j[win] == j[lose] == tj and d2[win] == d2[lose]
    # the pair read the other way round: what SC.swapped states
    sq, sm, sd, _ = SC.swapped(c)
    if len(s):
        fj, fd2, _ = nearest(s, t)
        fok = ~(fd2 > max2)
        assert np.array_equal(np.nonzero(fok)[0], sq) and np.array_equal(fj[fok], sm) and np.array_equal(fd2[fok], sd.astype(np.int64))


@pytest.mark.parametrize("name,frame", EVERY)
def test_every_sum_of_absolute_terms_is_below_2_53(name, frame):
    c = SC.case(name, frame)
    worst = 0.0
    for rec in (False, True):
        q, m, d = c["accepted"][rec]
        tot = SR.abs_sums(c["src"][q], c["tgt"][m], d, c["origin"])
        worst = max(worst, float(tot.max(initial=0.0)))
        assert np.array_equal(SR.exact_sums(c["src"][q], c["tgt"][m], d, c["origin"]), c["sums"][rec])
    q, m, d, _ = SC.self_pair(c)
    worst = max(worst, float(SR.abs_sums(c["src"][q], c["src"][m], d, c["origin"]).max()))
    print("%s/%s: the largest sum of absolute terms is %.3g of 2^53 = %.3g" % (name, frame, worst, TWO53))
    assert worst < TWO53
    if name == "empty":
        assert not c["sums"][False].any() and not c["sums"][True].any() and len(c["accepted"][False][0]) == 0


def test_exact_sums_refuses_what_is_not_integral():
    c = SC.case("65")
    q, m, d = c["accepted"][True]
    p = c["src"][q].copy()
    p[3, 1] += np.float32(0.5)
    with pytest.raises(AssertionError):
        SR.exact_sums(p, c["tgt"][m], d, c["origin"])
    with pytest.raises(AssertionError):
        SR.exact_sums(c["src"][q], c["tgt"][m], d, c["origin"] + 0.25)


def fake(c, rec, fault=None, q_begin=0, q_count=None, reduce_rows=0):
    n = len(c["src"])
    q_count = n - q_begin if q_count is None else q_count
    keep = np.zeros(n, bool)
    keep[c["accepted"][True][0]] = True
    d2 = np.where(c["host"] >= 0, c["d2_int"], np.inf)
    return SR.fake_sums(c["src"], c["tgt"], c["host"], d2, keep if rec else None, c["max_dist"] ** 2, c["origin"], q_begin, q_count,
                        SR.moments_blocks(q_count, SC.N_CU, reduce_rows), fault)


def same(got, ints):
    return np.array_equal(np.asarray(got, np.float64).view(np.uint64), np.asarray(ints, np.int64).astype(np.float64).view(np.uint64))


@pytest.mark.parametrize("name,frame", EVERY)
def test_the_fake_reduction_equals_the_integers(name, frame):
    c = SC.case(name, frame)
    for rec in (False, True):
        assert same(fake(c, rec), c["sums"][rec]), (name, frame, rec)
    if name == "rowcap+1":
        for rows in (1, 2, 7, 8, 9, 33, 1024):
            assert same(fake(c, True, reduce_rows=rows), c["sums"][True]), rows
    if name == "all_rows":
        assert SR.moments_blocks(len(c["src"]), SC.N_CU, 1024) == SR.MAX_BLOCKS
        assert same(fake(c, True, reduce_rows=1024), c["sums"][True])


def sub_sums(c, rec, b, n):
    q, m, d = c["accepted"][rec]
    k = (q >= b) & (q < b + n)
    return SR.exact_sums(c["src"][q[k]], c["tgt"][m[k]], d[k], c["origin"])


def test_every_fault_is_caught_at_a_named_size():
    """which sizes of SC.sizes() fail the bit-for-bit check under each fault of the fake (one-way acceptance, whole range unless a
    sub-range is named).  The expectations are stated, not measured: a wave with idle lanes exists at a size that is no multiple
    of 64 and no more than one stride; the last query is the third of its lane's trip only when 2 stride < q_count <= 3 stride, stride = 256 x the block count;
    more than 8 partial rows need more than 2048 queries; the cap matters wherever an edge point is (every size from 63 up)."""
    R = SC.row_cap()
    caught = {f: [] for f in SR.FAULTS}
    for name in SC.SMALL_NAMES + SC.LARGE_NAMES:
        c = SC.case(name)
        for f in SR.FAULTS:
            if not same(fake(c, False, f), c["sums"][False]):
                caught[f].append(name)
    print(caught)
    # a point is lost only if it was accepted: the orphans (3 of a case) are the exceptions allowed below
    partial = [n for n in SC.SMALL_NAMES + SC.LARGE_NAMES if SC.sizes()[n] % 64]
    assert set(caught["last_lane_of_partial_wave"]) <= set(partial) and {"1", "63", "65", "255", "257", "rowcap-1"} <= set(caught["last_lane_of_partial_wave"])
    assert not {"64", "256", "rowcap"} & set(caught["last_lane_of_partial_wave"])
    assert caught["third_query_at_the_end"] == ["2stride+1", "walk-1"]
    assert caught["rows_from_8"] == list(SC.LARGE_NAMES)
    assert caught["cap_is_a_miss"] == [n for n in SC.SMALL_NAMES + SC.LARGE_NAMES if SC.sizes()[n] >= 63]
    assert set(caught["range_starts_one_late"]) >= {"1"}
    # "walk+1": the one query of a lane's SECOND trip -- a walk that ends after one trip loses it
    c = SC.case("walk+1")
    n = len(c["src"])
    assert SR.moments_blocks(n, SC.N_CU) * SR.KRT * SR.KUN == n - 1 and c["host"][n - 1] >= 0
    # "blockcap": reduce_blocks' cap (pass1, pass2, point-to-plane, fitness): one block per CU strides twice
    assert SR.reduce_blocks(SC.sizes()["blockcap"], SC.N_CU) == SC.N_CU and SC.sizes()["blockcap"] > 256 * SC.N_CU + 256
    # the sub-range fault at the splits of the GPU test: a range of one accepted query comes back empty
    c = SC.case("257")
    for b, cnt in ((0, 1), (1, 255), (256, 1)):
        want = sub_sums(c, False, b, cnt)
        assert same(fake(c, False, None, b, cnt), want)
        first_ok = c["host"][b] >= 0
        assert same(fake(c, False, "range_starts_one_late", b, cnt), want) == (not first_ok), (b, cnt)
    assert c["host"][0] >= 0 and c["host"][256] >= 0                        # (so (0, 1) and (256, 1) do catch it)
    assert R == 64


def plane_list(c, rec):
    q, m, _ = c["accepted"][rec]
    return c["src"][q], c["tgt"][m], SC.axis_normals(len(c["tgt"]))[m]


@pytest.mark.parametrize("name", SC.PLANE_NAMES)
def test_one_lost_correspondence_moves_the_plane_solution(name):
    """a size proves something only if the exact point-to-plane solution without one correspondence differs from the full one by
    more than the GPU test allows: shown for the first, the middle and the last entry of the list (the last is what an idle-lane
    fault loses), in both acceptance modes.  The sums about the frame's own origin stay far below 2^53."""
    c = SC.case(name)
    for rec in (False, True):
        p, q, n = plane_list(c, rec)
        assert np.abs(SR.plane_terms(p, q, n)).sum(0).max() < TWO53
        assert np.array_equal(SR.fsum_plane(p, q, n)[0], SR.exact_plane(p, q, n).astype(np.float64))
        T, allow, cond, x = SR.plane_expectation(p, q, n)
        moves = []
        for drop in (0, len(p) // 2, len(p) - 1):
            keep = np.arange(len(p)) != drop
            T1 = SR.pcl_matrix(SR.plane_expectation(p[keep], q[keep], n[keep])[3])
            moves.append(float((np.abs(T1 - SR.pcl_matrix(x))[:3] / allow[:3]).max()))
        print("%s reciprocal %d: cond(A^T A) = %.3g, |x|_inf = %.3g; one entry less moves an entry by %s allowances" % (name, rec, cond, max(abs(float(v)) for v in x), ["%.3g" % v for v in moves]))
        assert min(moves) > 1.0, (name, rec, moves)


def test_three_correspondences_have_no_plane_solution():
    """a = [p x n, n] has 6 columns: 3 rows give A^T A the rank 3 at most, so no list of 3 has an exact solution to compare with
    (the smallest case of SC.PLANE_NAMES has 11 to 13 rows); size 3 itself keeps 2 correspondences and is refused by the align"""
    c = SC.case("65")
    p, q, n = plane_list(c, True)
    assert SR.plane_expectation(p[:3], q[:3], n[:3]) is None and SR.plane_expectation(p[:5], q[:5], n[:5]) is None
    assert len(SC.case("3")["accepted"][False][0]) == 2


def moments_of(mvr, p, q, origin):
    """the host chain of a caller's list: exact sums -> mvr_pair_moments2_t -> moments_from_moments2"""
    s = SR.exact_sums(p, q, np.zeros(len(p)), origin).astype(np.float64)
    row = np.concatenate([s[:1], np.asarray(origin, np.float64), s[1:28], [0.0]])
    return mvr.moments_from_moments2(mvr.moments2_from_row(row))


@pytest.mark.parametrize("name", ["sheet", "row", "identical", "three", "mirrored"])
def test_degenerate_lists_on_the_host(mvr, name):
    p, q = SC.degenerate_lists()[name]
    for origin in (np.zeros(3), np.array([0.0, 0.0, 896.0])):
        T, sv = mvr.umeyama_from_moments(moments_of(mvr, p, q, origin))
        assert T is not None
        SR.check_rigid_fit(T, p, q, "%s about %s" % (name, origin.tolist()))
