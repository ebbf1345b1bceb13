"""numpy reference of the plane segmentation (rules P1-P11 of mvr_cloud_segment_plane in include/mvr_hip.h): every f32 step of
the draws, the model, the perpendicular test and the distance is taken on numpy float32 scalars or arrays, one rounded operation
at a time; PCL's loop (P7) is replayed by a scalar Python loop.  Used by tests/test_sac_host.py (CPU) and tests/test_gpu_sac.py.

The refinement (P10) is compared by a tolerance, not bit for bit: the library takes the eigenvector from its cyclic Jacobi, the
reference from numpy's eigh of the same covariance.  The bar is the spread between that eigh result and an f64 SVD fit of the
centred inliers -- two textbook ways to the same plane -- over the cases of tests/sac_cases.py, times 4:

    measured on the CPU (tests/test_sac_host.py::test_refinement_bars_are_the_measured_spread prints it): the largest angle
    between the two normals 8.34e-15 rad (case duplicates), the largest difference of d 2.00e-11 (case far, whose d is 1e4;
    7.5e-15 elsewhere); the library's Jacobi route restated in numpy (jacobi_fit) stays within 2.2e-16 rad and 1.9e-12 of eigh

REFINE_ANGLE_BAR / REFINE_D_BAR below are those two, times 4, rounded up to two digits.  They bound the f64 plane BEFORE the cast
to f32 that ends P10; tests/test_gpu_sac.py turns them into the interval of f32 values the cast can give."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
DBL_EPSILON = float(np.finfo(F64).eps)

REFINE_ANGLE_BAR = 3.4e-14      # rad: 4 x 8.34e-15
REFINE_D_BAR = 8.1e-11          # mm: 4 x 2.00e-11
K_MARGIN = 0.01                 # every stop decision of a case keeps `iterations` this far from k
MOMENT_BLOCK = 256
PLANE, PERPENDICULAR = 0, 1
SKIPPED, COUNTED, INVALID = 0, 1, 3


# ------------------------------------------------------------------ P2: rule A2's draws

def mix(x):
    z = x & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, i, j, m):
    return (((mix((seed + G * (16 * i + j + 1)) & MASK) >> 32) * m) >> 32) & 0xFFFFFFFF


def sample_positions(seed, t, nv):
    """the three positions (among the valid points) of attempt t: the earlier samples are passed in ASCENDING ORDER OF VALUE"""
    got = []
    for j in range(3):
        r = draw(seed, t, j, nv - j)
        for c in sorted(got):
            if r >= c:
                r += 1
        got.append(r)
    return got


def sample_positions_in_draw_order(seed, t, nv):
    """WRONG (kept for the host test that shows why P2 says 'ascending'): the earlier samples passed in the order drawn"""
    got = []
    for j in range(3):
        r = draw(seed, t, j, nv - j)
        for c in got:
            if r >= c:
                r += 1
        got.append(r)
    return got


# ------------------------------------------------------------------ P3-P5

def plane_from_samples(p0, p1, p2):
    """(status, coefficients float32[4]); p*: float32[3]"""
    p0, p1, p2 = (np.asarray(v, F32) for v in (p0, p1, p2))
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        nx = e1[1] * e2[2] - e1[2] * e2[1]
        ny = e1[2] * e2[0] - e1[0] * e2[2]
        nz = e1[0] * e2[1] - e1[1] * e2[0]
        len2 = (nx * nx + ny * ny) + nz * nz
        ln = np.sqrt(len2)
        a, b, c = nx / ln, ny / ln, nz / ln
        d = -((a * p0[0] + b * p0[1]) + c * p0[2])
    co = np.array([a, b, c, d], F32)
    assert all(type(v) is F32 for v in (nx, len2, ln, a, d))
    if not (len2 > 0 and np.isfinite(co).all()):
        return SKIPPED, np.zeros(4, F32)
    return COUNTED, co


def perpendicular_cos(co, axis):
    a, b, c = (float(v) for v in co[:3])
    ax, ay, az = (float(v) for v in axis)
    na = math.sqrt((ax * ax + ay * ay) + az * az)
    return abs((a * ax + b * ay) + c * az) / (math.sqrt((a * a + b * b) + c * c) * na)


def distances(co, P, fma=False):
    """P5's t for every row of P (float32 (n, >= 3)): float32[n]"""
    a, b, c, d = (F32(v) for v in co)
    x, y, z = (np.ascontiguousarray(P[:, k], F32) for k in range(3))
    with np.errstate(all="ignore"):
        t = a * x
        if fma:      # a product of two f32 is exact in the 64-bit mantissa of a long double, the sum is rounded there and then once more
            L = np.longdouble
            t = (L(b) * y.astype(L) + t.astype(L)).astype(F32)
            t = (L(c) * z.astype(L) + t.astype(L)).astype(F32)
        else:
            t = t + b * y
            t = t + c * z
        t = t + d
    assert t.dtype == F32
    return t


def inlier_mask(co, P, threshold, fma=False):
    with np.errstate(all="ignore"):
        return np.abs(distances(co, P, fma)).astype(F64) < float(threshold)


# ------------------------------------------------------------------ P10

def moment_sums(P, mask, q):
    """the ten sums (count, d, d d^T upper triangle) about q in P10's fixed order"""
    n = len(P)
    nb = (n + MOMENT_BLOCK - 1) // MOMENT_BLOCK
    V = np.zeros((nb * MOMENT_BLOCK, 10), F64)
    i = np.nonzero(mask)[0]
    d = P[i, :3].astype(F64) - np.asarray(q, F32)[:3].astype(F64)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    V[i] = np.stack([np.ones(len(i)), dx, dy, dz, dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz], 1)
    V = V.reshape(nb, MOMENT_BLOCK, 10)
    s = MOMENT_BLOCK // 2
    while s:
        V[:, :s] = V[:, :s] + V[:, s:2 * s]
        s //= 2
    return np.cumsum(V[:, 0, :], axis=0)[-1]      # (cumsum adds in order; np.sum would add pairwise)


def covariance(S):
    inv = 1.0 / S[0]
    m = S[1:4] * inv
    C = np.empty((3, 3), F64)
    C[0, 0] = S[4] * inv - m[0] * m[0]; C[0, 1] = C[1, 0] = S[5] * inv - m[0] * m[1]; C[0, 2] = C[2, 0] = S[6] * inv - m[0] * m[2]
    C[1, 1] = S[7] * inv - m[1] * m[1]; C[1, 2] = C[2, 1] = S[8] * inv - m[1] * m[2]; C[2, 2] = S[9] * inv - m[2] * m[2]
    return m, C


def _finish_fit(nrm, mean, ransac):
    nrm = np.asarray(nrm, F64) / np.linalg.norm(nrm)
    r = np.asarray(ransac, F32).astype(F64)
    if (nrm[0] * r[0] + nrm[1] * r[1]) + nrm[2] * r[2] < 0.0:
        nrm = -nrm
    return nrm, -((nrm[0] * mean[0] + nrm[1] * mean[1]) + nrm[2] * mean[2])


def eigh_fit(P, mask, q, ransac):
    """P10 with numpy's eigh in place of the Jacobi: (unit normal f64[3], d f64)"""
    m, C = covariance(moment_sums(P, mask, q))
    w, v = np.linalg.eigh(C)
    return _finish_fit(v[:, 0], np.asarray(q, F32)[:3].astype(F64) + m, ransac)


def svd_fit(P, mask, ransac):
    """the same plane another way: f64 SVD of the centred inliers"""
    X = P[mask, :3].astype(F64)
    mean = X.mean(0)
    _, _, vt = np.linalg.svd(X - mean, full_matrices=False)
    return _finish_fit(vt[2], mean, ransac)


def jacobi_fit(P, mask, q, ransac):
    """the library's own route (csrc/mvr_plane.h: plane_fit) restated: cyclic Jacobi, the column of the smallest eigenvalue"""
    m, A = covariance(moment_sums(P, mask, q))
    V = np.eye(3)
    for _ in range(12):
        off = A[0, 1] * A[0, 1] + A[0, 2] * A[0, 2] + A[1, 2] * A[1, 2]
        dia = A[0, 0] * A[0, 0] + A[1, 1] * A[1, 1] + A[2, 2] * A[2, 2]
        if not off > 1.0e-40 * dia:
            break
        for p, qq, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p, qq]
            if apq == 0.0:
                continue
            theta = (A[qq, qq] - A[p, p]) / (2.0 * apq)
            t = 0.5 / theta if abs(theta) > 1.0e150 else math.copysign(1.0, theta) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            A[p, p] -= t * apq
            A[qq, qq] += t * apq
            A[p, qq] = A[qq, p] = 0.0
            arp, arq = A[r, p], A[r, qq]
            A[r, p] = A[p, r] = c * arp - s * arq
            A[r, qq] = A[qq, r] = s * arp + c * arq
            vp, vq = V[:, p].copy(), V[:, qq].copy()
            V[:, p] = c * vp - s * vq
            V[:, qq] = s * vp + c * vq
    k = int(np.argmin(np.diag(A)))
    return _finish_fit(V[:, k], np.asarray(q, F32)[:3].astype(F64) + m, ransac)


def angle_between(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return math.atan2(np.linalg.norm(np.cross(a, b)), float(a @ b))


# ------------------------------------------------------------------ P1-P11

def segment(P, threshold, model=PLANE, max_iterations=1000, probability=0.99, optimize=True, axis=None, eps_angle=None, seed=0,
            fma=False, check_margin=True):
    """the whole call on float32 points P (n, >= 3).  Returns a dict: found, iterations, attempts, skipped, best_attempt, k;
    trace = dict(status, sample, coefficients, inliers, k) over the attempts made; valid; ransac_coefficients, ransac_mask;
    refined = (normal f64[3], d f64) by eigh, or None when P10 keeps the RANSAC plane; coefficients / mask = the final ones
    by the reference's own refinement; min_margin = the smallest |iterations - k| at a stop decision."""
    P = np.ascontiguousarray(P, F32)
    n = len(P)
    valid = np.isfinite(P[:, :3]).all(1) if n else np.zeros(0, bool)
    vidx = np.nonzero(valid)[0]
    nv = len(vidx)
    tr = dict(status=[], sample=[], coefficients=[], inliers=[], k=[])
    iterations = skipped = t = 0
    k, best_count, best, margin = 1.0, -1, -1, math.inf
    cos_eps = math.cos(eps_angle) if model == PERPENDICULAR else 0.0
    log_p = math.log(1.0 - probability)
    if nv >= 3:
        while True:
            margin = min(margin, abs(iterations - k))
            if not (iterations < k and skipped < 10 * max_iterations):
                break
            s = [int(vidx[r]) for r in sample_positions(seed, t, nv)]
            status, co = plane_from_samples(P[s[0], :3], P[s[1], :3], P[s[2], :3])
            if status == COUNTED and model == PERPENDICULAR and perpendicular_cos(co, axis) < cos_eps:
                status = INVALID
            count = int(inlier_mask(co, P, threshold, fma).sum()) if status == COUNTED else 0
            stop = False
            if status == SKIPPED:
                skipped += 1
            else:
                if count > best_count:
                    best_count, best = count, t
                    w = best_count / float(nv)
                    pno = min(max(1.0 - w * w * w, DBL_EPSILON), 1.0 - DBL_EPSILON)
                    k = log_p / math.log(pno)
                iterations += 1
                stop = iterations > max_iterations      # PCL's own off-by-one
            for key, v in zip(("status", "sample", "coefficients", "inliers", "k"), (status, s, co, count, k)):
                tr[key].append(v)
            t += 1
            if stop:
                break
    if check_margin:
        assert margin >= K_MARGIN, "a stop decision within %g of k" % margin
    trace = dict(status=np.array(tr["status"], np.int32), sample=np.array(tr["sample"], np.uint32).reshape(-1, 3),
                 coefficients=np.array(tr["coefficients"], F32).reshape(-1, 4), inliers=np.array(tr["inliers"], np.uint32),
                 k=np.array(tr["k"], F64))
    out = dict(found=best_count > 0, iterations=iterations, attempts=t, skipped=skipped, best_attempt=best if best_count > 0 else -1,
               k=k, trace=trace, valid=valid, nv=nv, min_margin=margin, refined=None,
               ransac_coefficients=np.zeros(4, F32), ransac_mask=np.zeros(n, bool))
    if out["found"]:
        co = trace["coefficients"][best]
        mask = inlier_mask(co, P, threshold, fma)
        assert mask.sum() == best_count and not mask[~valid].any()
        out.update(ransac_coefficients=co.copy(), ransac_mask=mask)
        if optimize and mask.sum() >= 3:
            nrm, d = eigh_fit(P, mask, P[trace["sample"][best][0]], co)
            cand = np.array([nrm[0], nrm[1], nrm[2], d], F64).astype(F32)
            if np.isfinite(cand).all():
                out["refined"] = (nrm, d)
                co = cand
                mask = inlier_mask(co, P, threshold, fma)
    out.update(coefficients=out["ransac_coefficients"] if not out["found"] else co, mask=out["ransac_mask"] if not out["found"] else mask)
    return out
