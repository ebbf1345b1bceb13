"""numpy reference of the feature matching and of the sample-consensus alignment (include/mvr_hip.h: mvr_feature_knn rules
M1-M3, mvr_align_prerejective rules A1-A4 and A6): FLANN's L2_Simple as a 33-step f32 loop vectorised over pairs, the
(d2 bits, index) selection of normals_ref.knn_brute, the draws in np.uint64, the polygon test in f32 and the selection of the
best pose.  The pose estimate (A5) and the scores (rule S) have anchors of their own in the GPU tests: numpy's Kabsch here,
ctx.transform_f32 + ctx.nn there."""
import numpy as np

from outlier_ref import d2_f32, finite_mask

F32, F64, U64 = np.float32, np.float64, np.uint64
NONE = np.uint32(0xFFFFFFFF)
DIM = 33
G = U64(0x9E3779B97F4A7C15)
DBL_MAX = np.finfo(F64).max


# ------------------------------------------------------------------ rule M

def feat_d2(q, t):
    """M1 for every pair: acc = 0; for b: diff = q[b] - t[b]; acc = acc + diff * diff -- numpy rounds every f32 operation
    (the three operations of a step are written into preallocated arrays: the same roundings, less memory traffic)"""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    qT, tT = np.ascontiguousarray(q.T), np.ascontiguousarray(t.T)
    acc = np.zeros((len(q), len(t)), F32)
    diff = np.empty_like(acc)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(q.shape[1]):
            np.subtract(qT[b][:, None], tT[b][None, :], out=diff)
            np.multiply(diff, diff, out=diff)
            np.add(acc, diff, out=acc)
    return acc


def _steps(q, t):
    """(diff, diff * diff) of every step of M1 as f32 arrays over the pairs, component by component"""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    qT, tT = np.ascontiguousarray(q.T), np.ascontiguousarray(t.T)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(q.shape[1]):
            diff = np.subtract(qT[b][:, None], tT[b][None, :])
            yield diff, np.multiply(diff, diff)


def d2_fma_chain(q, t):
    """WRONG: acc = fma(diff, diff, acc).  The product of two f32 is exact in f64; the f64 sum rounded to f32 is the fused
    result but for a double rounding in a few cases out of a million -- near enough for a variant that is wrong anyway"""
    acc = np.zeros((len(q), len(t)), F32)
    for diff, _ in _steps(q, t):
        d = diff.astype(F64)
        acc = (acc.astype(F64) + d * d).astype(F32)
    return acc


def d2_four_accumulators(q, t):
    """WRONG: component b goes to accumulator b % 4, the four added as (a0 + a1) + (a2 + a3)"""
    acc = [np.zeros((len(q), len(t)), F32) for _ in range(4)]
    for b, (_, sq) in enumerate(_steps(q, t)):
        acc[b % 4] = acc[b % 4] + sq
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def d2_reverse_order(q, t):
    """WRONG: the sum from component 32 down to 0"""
    sq = [s for _, s in _steps(q, t)]
    acc = np.zeros((len(q), len(t)), F32)
    for s in reversed(sq):
        acc = acc + s
    return acc


def d2_pairwise_tree(q, t):
    """WRONG: neighbours added in pairs, level by level"""
    level = [s for _, s in _steps(q, t)]
    while len(level) > 1:
        level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    return level[0]


def d2_f64_rounded_once(q, t):
    """WRONG: differences, squares and sum in f64, one rounding to f32 at the end"""
    acc = np.zeros((len(q), len(t)), F64)
    for diff, _ in _steps(q, t):
        d = diff.astype(F64)
        acc += d * d
    return acc.astype(F32)


# what an "optimised" distance loop would compute instead of M1: for tests/test_align_host.py only, which asserts on which inputs
# the suite can tell them from feat_d2
WRONG_D2 = {"fma chain": d2_fma_chain, "four accumulators": d2_four_accumulators, "reverse order": d2_reverse_order,
            "pairwise tree": d2_pairwise_tree, "f64 rounded once": d2_f64_rounded_once}


def knn_from_d2(D, k):
    """the k smallest (d2 bits, index) keys per row of a finite d2 table: (idx, d2)"""
    key = (np.asarray(D, F32).view(np.uint32).astype(U64) << U64(32)) | np.arange(D.shape[1], dtype=U64)[None, :]
    key = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
    return (key & U64(0xFFFFFFFF)).astype(np.uint32), (key >> U64(32)).astype(np.uint32).view(F32)


def feature_knn(q, t, k, chunk=None):
    """(idx[nq, k] uint32, d2[nq, k] float32): the k smallest (d2 bits, index) keys per query, ascending; a pair whose d2 is not
    finite is not listed (M3: that is every pair of a non-finite row); UINT32_MAX / +inf fill the rest"""
    q, t = np.asarray(q, F32).reshape(-1, DIM), np.asarray(t, F32).reshape(-1, DIM)
    n, m = len(q), len(t)
    idx = np.full((n, k), NONE, np.uint32)
    d2 = np.full((n, k), np.inf, F32)
    if n == 0 or m == 0:
        return idx, d2
    kk = min(k, m)
    step = chunk or max(1, int(1e6) // m)      # (a chunk's arrays stay in the cache)
    ti = np.arange(m, dtype=U64)[None, :]
    for c0 in range(0, n, step):
        D = feat_d2(q[c0:c0 + step], t)
        with np.errstate(invalid="ignore"):
            D = np.where(np.isfinite(D), D, F32(np.inf))
        key = (D.view(np.uint32).astype(U64) << U64(32)) | ti
        if kk < m:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key.sort(axis=1)
        d = (key >> U64(32)).astype(np.uint32).view(F32)
        none = np.isinf(d)
        idx[c0:c0 + step, :kk] = np.where(none, NONE, (key & U64(0xFFFFFFFF)).astype(np.uint32))
        d2[c0:c0 + step, :kk] = np.where(none, F32(np.inf), d)
    return idx, d2


# ------------------------------------------------------------------ rule A2

def mix(x):
    """splitmix64's finaliser on np.uint64 arrays (arithmetic mod 2^64)"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, U64).copy()
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def draw(seed, i, j, m):
    """draw(i, j, m) = ((mix(seed + G * (16 i + j + 1)) >> 32) * m) >> 32, vectorised over i (j, m scalars or arrays)"""
    with np.errstate(over="ignore"):
        i, j, m = np.asarray(i, U64), np.asarray(j, U64), np.asarray(m, U64)
        x = U64(seed) + G * (U64(16) * i + j + U64(1))
        return (((mix(x) >> U64(32)) * m) >> U64(32)).astype(np.int64)


def sample_positions(seed, i, ne, nr):
    """the nr distinct positions in 0..ne-1 of iteration i, in sample order"""
    pos = []
    for j in range(nr):
        r = int(draw(seed, i, j, ne - j))
        for c in sorted(pos):
            if r >= c:
                r += 1
        pos.append(r)
    return pos


# ------------------------------------------------------------------ rules A1, A3, A4

def eligible(points, feat):
    """A1: indices of the points with finite coordinates and 33 finite features, ascending"""
    return np.nonzero(finite_mask(points) & np.isfinite(np.asarray(feat, F32).reshape(len(points), DIM)).all(1))[0].astype(np.uint32)


def polygon_ok(ps, pt, similarity, fma=False):
    """A4 on one polygon: ps / pt are the [nr, >=3] sampled points and their matches"""
    nr = len(ps)
    thr = F32(F64(similarity) * F64(similarity))
    ok = True
    for j in range(nr):
        n = (j + 1) % nr
        ds, dt = F32(d2_f32(ps[j, :3], ps[n, :3], fma)), F32(d2_f32(pt[j, :3], pt[n, :3], fma))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            sim = ds / dt if ds < dt else dt / ds
        ok = ok and bool(sim >= thr)
    return ok


def replay(src_pts, tgt_pts, elig, knn_idx, iters, nr, seed, similarity, fma=False):
    """A2-A4 for every iteration from a k-NN table of the eligible rows: (status[iters], src[iters, nr], tgt[iters, nr]);
    status 0 polygon-rejected, 1 to be scored, 2 no match"""
    ne = len(elig)
    status = np.full(iters, 2, np.int32)
    src = np.full((iters, nr), NONE, np.uint32)
    tgt = np.full((iters, nr), NONE, np.uint32)
    if ne < nr:
        return status, src, tgt
    kk_all = (knn_idx != NONE).sum(1)
    for i in range(iters):
        pos = sample_positions(seed, i, ne, nr)
        src[i] = elig[pos]
        matched = True
        for j, r in enumerate(pos):
            kk = int(kk_all[r])
            if kk == 0:
                matched = False
                continue
            tgt[i, j] = knn_idx[r, int(draw(seed, i, 8 + j, kk))]
        if matched:
            status[i] = 1 if polygon_ok(src_pts[src[i]], tgt_pts[tgt[i]], similarity, fma) else 0
    return status, src, tgt


# ------------------------------------------------------------------ rule A6

def select(status, inliers, error, n_src, inlier_fraction, guess=None):
    """the pose A6 takes: (converged, best_iteration); guess = (inliers, error) of the guess, scored first (-1)"""
    lowest, best, conv = DBL_MAX, -1, False
    order = ([(-1,) + tuple(guess)] if guess is not None else []) + [(i, inliers[i], error[i]) for i in np.nonzero(status == 1)[0]]
    for i, n, e in order:
        if n_src and F64(n) / F64(n_src) >= inlier_fraction and e < lowest:
            lowest, best, conv = e, int(i), True
    return conv, best


def kabsch(p, q):
    """the rigid motion of least squares from p to q ([n, 3] f64): R = U diag(1, 1, det) V^T of E[(q - mq)(p - mp)^T]"""
    p, q = np.asarray(p, F64), np.asarray(q, F64)
    pm, qm = p.mean(0), q.mean(0)
    U, S, Vt = np.linalg.svd((q - qm).T @ (p - pm) / len(p))
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))]) @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, qm - R @ pm
    return T, S
