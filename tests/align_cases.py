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
KNN_KS = (1, 2, 10, 64)
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
