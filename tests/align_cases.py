"""The inputs the matching and alignment tests share (tests/test_align_host.py checks their conditions on the reference alone,
the tests/test_gpu_feature_knn.py, test_gpu_pose_scores.py and test_gpu_align.py compare the GPU on them)."""
import numpy as np

import mls_cases as K
import walk_cases as W

F32, F64 = np.float32, np.float64
DIM = 33


# ------------------------------------------------------------------ feature tables

def features(rng, n, step=4.0):
    """FPFH-like values: uniform in 0..100, rounded to multiples of `step` -- every difference and every partial sum of M1 is
    then an exact f32 integer and equal d2 between different rows are common"""
    return (np.round(rng.uniform(0.0, 100.0, (n, DIM)) / step) * step).astype(F32)


KNN_NQ, KNN_NT = 300, 700            # no multiple of the 256 queries of a block nor of the 64 rows of a tile
KNN_KS = (1, 2, 8, 9, 10, 16, 17, 32, 33, 63, 64)      # every list size (8 / 16 / 32 / 64) and both sides of every edge between two
KNN_TAILS = (1, 5, 63, 65)           # targets for k = 64: the tails of the lists, one row short of and past a tile
KNN_BIG = (5000, 20000)              # crosses the automatic split of the target and its merge
KNN_SPLITS = (1, 2, 3, 7, 64)        # values of the tune key "feat_split" (0, the default, besides)


def knn_plain(seed=1, nq=KNN_NQ, nt=KNN_NT):
    rng = np.random.default_rng(seed)
    return features(rng, nq), features(rng, nt)


def knn_duplicates(seed=2, nq=KNN_NQ, nt=KNN_NT):
    """40 % of the target rows are copies of other rows, the copies placed at both ends of the array (and the originals in
    the middle), so equal keys' d2 meet across tile and block boundaries; a tenth of the queries ARE target rows (d2 = 0)"""
    rng = np.random.default_rng(seed)
    q, t = features(rng, nq), features(rng, nt)
    nd = int(0.4 * nt)
    ends = np.r_[np.arange(nd // 2), np.arange(nt - (nd - nd // 2), nt)]
    mid = np.arange(nd // 2, nt - (nd - nd // 2))
    t[ends] = t[rng.choice(mid, nd, replace=True)]
    q[::10] = t[rng.choice(nt, len(q[::10]))]
    return q, t


def knn_non_finite(seed=3, nq=KNN_NQ, nt=KNN_NT):
    """5 % of the rows of either side hold a NaN, an infinity or both somewhere"""
    rng = np.random.default_rng(seed)
    q, t = knn_duplicates(seed, nq, nt)
    for a in (q, t):
        bad = rng.choice(len(a), max(len(a) // 20, 1), replace=False)
        for j, i in enumerate(bad):
            a[i, rng.integers(DIM)] = (np.nan, np.inf, -np.inf)[j % 3]
            if j % 4 == 0:
                a[i, rng.integers(DIM)] = np.inf
        a[bad[0]] = np.nan
    return q, t


# ------------------------------------------------------------------ feature tables of real values
# On the tables above every partial sum of M1 is an exact integer: any order and any rounding of the sum gives the same bits.
# The tables below are the ones on which the order and the rounding show (tests/test_align_host.py asserts both statements).

KNN_REAL = ("real", "fpfh_like", "twins", "signatures", "range", "key_zero")
KNN_SPLIT_SHAPE = (257, 4161)        # one query past a block; 66 tiles of 64 rows and one row: feat_split 7 gives 7 x 640 rows
KNN_EDGE_NQ, KNN_EDGE_NT = (1, 255, 256, 257), (1, 63, 64, 65, 255, 257)
TWIN_STEP = 2.0 ** -10               # the lattice of the twins: q, d and q - d are multiples of it below 2^7, exact in f32
FEAT_TILE = 64                       # kFeatTile of csrc/mvr_feature.hip: a split of the target is a whole number of tiles


def knn_real(seed=21, nq=KNN_NQ, nt=KNN_NT):
    """uniform in 0..100, left unrounded: every step of M1 rounds"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 100.0, (nq, DIM)).astype(F32), rng.uniform(0.0, 100.0, (nt, DIM)).astype(F32)


def fpfh_like(rng, n):
    """three blocks of 11 non-negative values that sum to 100 each, most of them small: the shape of a signature"""
    g = rng.gamma(0.3, 1.0, (n, 3, DIM // 3)) + 1e-12
    return (100.0 * g / g.sum(2, keepdims=True)).reshape(n, DIM).astype(F32)


def knn_fpfh_like(seed=22, nq=KNN_NQ, nt=KNN_NT):
    rng = np.random.default_rng(seed)
    return fpfh_like(rng, nq), fpfh_like(rng, nt)


def twin_rows(nq, nt):
    """the rows of the first twin of every query (the second is the next row): odd rows, so a pair never shares its first
    row with another, and first of all the rows 64 m - 1 -- those pairs straddle a tile boundary, and a split of the target
    ends at one"""
    odd = np.arange(1, nt - 1, 2)
    edge = odd[(odd + 1) % FEAT_TILE == 0][:nq]
    return edge, np.setdiff1d(odd, edge)


def _twins(seed, nq, nt):
    rng = np.random.default_rng(seed)
    assert nt >= 2 * nq + 1
    q = (rng.integers(0, int(100 / TWIN_STEP) + 1, (nq, DIM)) * TWIN_STEP).astype(F32)
    d = rng.integers(-int(8 / TWIN_STEP), int(8 / TWIN_STEP) + 1, (nq, DIM)) * TWIN_STEP
    dp = np.stack([row[rng.permutation(DIM)] for row in d])
    t = rng.uniform(0.0, 100.0, (nt, DIM)).astype(F32)
    edge, rest = twin_rows(nq, nt)
    first = np.r_[edge, rng.choice(rest, nq - len(edge), replace=False)][rng.permutation(nq)]
    a, b = (q.astype(F64) - d).astype(F32), (q.astype(F64) - dp).astype(F32)
    assert np.array_equal(a.astype(F64), q.astype(F64) - d) and np.array_equal(b.astype(F64), q.astype(F64) - dp)
    assert np.array_equal((q - a).astype(F64), d) and np.array_equal((q - b).astype(F64), dp)      # the f32 differences are exact
    t[first], t[first + 1] = a, b
    return q, t, first


def knn_twins(seed=23, nq=KNN_NQ, nt=KNN_NT):
    """Every query q has two target rows q - d and q - perm(d), adjacent in the table: the 33 differences of the one are a
    permutation of the other's, all exact in f32 (asserted), so the two d2 are equal in exact arithmetic and differ in f32
    by the order of the roundings alone.  The other rows are uniform in 0..100 and far away (a twin lies 33 * 8^2 at most from
    its query, any other row about 33 * 1 666): which twin leads the list of q is decided by M1's order and rounding alone."""
    return _twins(seed, nq, nt)[:2]


def twin_first_rows(seed=23, nq=KNN_NQ, nt=KNN_NT):
    """the row of the first twin of every query of knn_twins (the second is the next row)"""
    return _twins(seed, nq, nt)[2]


def knn_signatures(nq=KNN_NQ):
    """the reference's FPFH signatures of fpfh_cases.box(), the first 300 as queries and the other 2 700 as the target: rows the
    project's own descriptor produces"""
    import fpfh_cases as FC
    import fpfh_ref
    p, nrm, radius = FC.box()
    f = np.ascontiguousarray(fpfh_ref.fpfh(p, nrm, radius)[0], dtype=F32)
    assert f.shape == (FC.BOX_N, DIM) and np.isfinite(f).all()
    return f[:nq].copy(), f[nq:].copy()


RANGE_BIG, RANGE_SMALL = 3.0e19, 1.0e-30      # (3e19)^2 overflows f32; (1e-30)^2 underflows to 0


def knn_range(seed=25, nq=KNN_NQ, nt=KNN_NT):
    """finite rows at the two ends of f32's range, on the table of knn_real.
    Overflow: the first 40 queries have an exact copy among the target rows but for one component, RANGE_BIG away:
    diff * diff is +inf, d2 is not finite and the pair is not listed (M3), although every row is finite.  Query 40 holds
    RANGE_BIG itself: it lists the ten target rows that hold it in the same component, and no other.
    Underflow: queries 50..129 are 0 in one component and have two copies in the target, an exact one and one that holds
    RANGE_SMALL there: diff * diff underflows to 0, both d2 are 0 and the lower index leads -- the near copy for the even
    queries, the exact copy for the odd ones."""
    rng = np.random.default_rng(seed)
    q, t = knn_real(seed, nq, nt)
    rows = rng.permutation(nt)
    assert nq >= 130 and nt >= 300
    n_over, n_under = 40, 80
    take = iter(rows)
    for i in range(n_over):
        r, b = next(take), rng.integers(DIM)
        t[r] = q[i]
        t[r, b] = q[i, b] + F32(RANGE_BIG) * (1 if i % 2 else -1)
    q[40, 7] = RANGE_BIG
    for j in range(10):
        t[next(take), 7] = F32(RANGE_BIG) * (1.0 + 2.0 ** -20 * j)
    pairs = np.sort(np.array([next(take) for _ in range(2 * n_under)]).reshape(-1, 2), axis=1)
    for j, (lo, hi) in enumerate(pairs):
        i, b = 50 + j, rng.integers(DIM)
        q[i, b] = 0.0
        near, exact = (lo, hi) if i % 2 == 0 else (hi, lo)
        t[near], t[exact] = q[i], q[i]
        t[near, b] = RANGE_SMALL
    assert np.isfinite(q).all() and np.isfinite(t).all()
    return q, t


def knn_key_zero(seed=26, nq=KNN_NQ, nt=KNN_NT):
    """query 0 IS target row 0: its first key is (d2 = +0.0, index 0), the 64-bit integer 0 -- the value the kernels fill the
    unused slots of a list with.  Every third query is an exact copy of some other row, and rows 1..5 are copies of row 0."""
    rng = np.random.default_rng(seed)
    q, t = knn_real(seed, nq, nt)
    q[::3] = t[rng.choice(np.arange(6, nt), len(q[::3]), replace=False)]
    t[1:6] = t[0]
    q[0] = t[0]
    return q, t


# ------------------------------------------------------------------ pose scores

SCORE_MAX_DIST = 2.0                 # exact in f32, and so is its square
SCORE_NS, SCORE_NT, SCORE_LATTICE = 3000, 7000, 600
SCORE_PLANE_Z = 950.0


def score_clouds(seed=4):
    """(source [3000, 4], target [7000, 4]).  The target: 6 400 points in a slab 880 <= z <= 900 and a 30 x 20 lattice of 5 mm
    on the axis-aligned plane z = 950.  The source: 2 400 noisy copies of slab points and the same lattice, a fifth of its
    points.  Under the pose `z + 2` every lattice point lies exactly 2 mm above its twin -- x' = ((1 x + 0 y) + 0 z) + 0 and
    z' = 950 + 2 are exact -- with the next target point sqrt(29) mm away: d2 == max_dist^2 exactly, the case of the strict <."""
    rng = np.random.default_rng(seed)
    slab = np.c_[rng.uniform(-60, 60, (SCORE_NT - SCORE_LATTICE, 2)), rng.uniform(880, 900, SCORE_NT - SCORE_LATTICE)]
    i, j = np.meshgrid(np.arange(30), np.arange(20), indexing="ij")
    lat = np.c_[5.0 * i.ravel(), 5.0 * j.ravel(), np.full(SCORE_LATTICE, SCORE_PLANE_Z)]
    t = W.cloud(np.r_[slab, lat][rng.permutation(SCORE_NT)])
    pick = rng.choice(len(slab), SCORE_NS - SCORE_LATTICE, replace=False)
    s = W.cloud(np.r_[slab[pick] + rng.normal(0, 0.4, (len(pick), 3)), lat][rng.permutation(SCORE_NS)])
    return s, t


def translation(x, y, z):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = (x, y, z)
    return T


def rigid(axis, ang, shift, centre=(0.0, 0.0, 900.0)):
    c = np.asarray(centre, F64)
    T = np.eye(4)
    T[:3, :3] = K.rodrigues(axis, ang)
    T[:3, 3] = c - T[:3, :3] @ c + np.asarray(shift, F64)
    return T.astype(F32)


def score_poses(seed=5):
    """37 poses (no multiple of any chunk): the identity, z + 2 (a fifth of the points exactly at max_dist), z + 2 - 2^-13
    (the same points just inside: two f32 steps at z = 950), four poses that put the source far outside the target's grid, and 30 small rigid motions"""
    rng = np.random.default_rng(seed)
    P = [np.eye(4, dtype=F32), translation(0, 0, SCORE_MAX_DIST), translation(0, 0, SCORE_MAX_DIST - 2.0 ** -13),
         translation(1.0e4, 0, 0), translation(0, -3.0e6, 5.0e5), rigid([0, 1, 0], np.pi / 2, (0, 0, 0), centre=(5000.0, 0, 0)),
         translation(0, 0, -400.0)]
    for _ in range(30):
        P.append(rigid(rng.standard_normal(3), rng.uniform(0, 0.03), rng.normal(0, 0.8, 3)))
    return np.stack(P)


SCORE_STRICT_POSE, SCORE_INSIDE_POSE = 1, 2


# ------------------------------------------------------------------ the aligner on small tables

ALIGN_NS, ALIGN_NT, ALIGN_ITERS = 400, 600, 200
ALIGN_MAX_DIST, ALIGN_FRACTION = 1.5, 0.25
ALIGN_SIMILARITY, ALIGN_K = 0.5, 2     # test_align_host.py asserts that a quarter to three quarters of the iterations are rejected
ALIGN_SEED = 2026
ALIGN_POSE = rigid([0.2, -0.6, 0.77], 1.1, (6.0, -4.0, 9.0))      # source -> target


def align_pair(seed=6):
    """(source points, target points, source features, target features).  The target: 600 points in a 40 mm box with rounded
    random features.  The source: 300 of them moved by the inverse of ALIGN_POSE, with their features changed a little, and 100
    unrelated points -- so that matching, polygon test and scoring all have both outcomes among 200 iterations"""
    rng = np.random.default_rng(seed)
    t = W.cloud(rng.uniform(-20, 20, (ALIGN_NT, 3)) + [0.0, 0.0, 900.0])
    tf = features(rng, ALIGN_NT)
    pick = rng.choice(ALIGN_NT, 300, replace=False)
    inv = np.linalg.inv(ALIGN_POSE.astype(F64))
    twin = t[pick, :3].astype(F64) @ inv[:3, :3].T + inv[:3, 3] + rng.normal(0, 0.1, (300, 3))
    other = rng.uniform(-20, 20, (ALIGN_NS - 300, 3)) + [0.0, 0.0, 900.0]
    sf = np.r_[tf[pick] + 4.0 * rng.integers(-1, 2, (300, DIM)).astype(F32), features(rng, ALIGN_NS - 300)].astype(F32)
    perm = rng.permutation(ALIGN_NS)
    return W.cloud(np.r_[twin, other][perm]), t, np.ascontiguousarray(sf[perm]), tf


def align_with_invalid(seed=7):
    """the same pair with non-finite source points, non-finite source rows (on other points) and non-finite target rows"""
    s, t, sf, tf = align_pair()
    rng = np.random.default_rng(seed)
    bad = rng.choice(ALIGN_NS, 30, replace=False)
    s, sf, tf = s.copy(), sf.copy(), tf.copy()
    s[bad[:10], rng.integers(0, 3, 10)] = np.nan
    sf[bad[10:20], rng.integers(0, DIM, 10)] = np.inf
    sf[bad[20:], rng.integers(0, DIM, 10)] = np.nan
    tf[rng.choice(ALIGN_NT, 20, replace=False), rng.integers(0, DIM, 20)] = np.nan
    return s, t, sf, tf


# ------------------------------------------------------------------ recovery

REC_N, REC_LEAF = 60000, 4.0                     # a synthetic view, voxel-downsampled to a few thousand points
REC_NORMAL_RADIUS, REC_FPFH_RADIUS = 10.0, 20.0
REC_MAX_DIST = 6.0                               # 1.5 leaves, as PCL's alignment tutorial takes it
REC_PARAMS = dict(max_iterations=20000, nr_samples=3, k=2, similarity=0.9, max_dist=REC_MAX_DIST, inlier_fraction=0.25, seed=7)
REC_REPLAY = 1000                                # iterations of the recovery run that the GPU test replays through align_ref
REC_POSE = rigid([0.3, -0.5, 0.81], np.deg2rad(70.0), (7.0, -3.0, 11.0), centre=(0.0, 0.0, 917.0))      # target -> source


def recovery_view(mvr, n=REC_N):
    """(target view, the same view moved by REC_POSE on the host in f64): both are voxel-downsampled by the caller, so the
    two clouds hold different points of one surface"""
    t = mvr.synth_view(mvr.synth_params(12, 3), 0, n)
    s = t.copy()
    s[:, :3] = (t[:, :3].astype(F64) @ REC_POSE[:3, :3].astype(F64).T + REC_POSE[:3, 3].astype(F64)).astype(F32)
    return s, t
