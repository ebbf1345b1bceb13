"""numpy reference of the k-NN search and of the normal estimation (include/mvr_hip.h: mvr_knn,
mvr_cloud_estimate_normals): the f32 distance expression of the library, the (d2, index) order, f64 covariance
about the query point divided by the neighbour count, numpy's eigh, PCL's f32 flip towards the viewpoint."""
import numpy as np

from outlier_ref import d2_f32, finite_mask, within_r2

NONE = np.uint32(0xFFFFFFFF)


def dist2_f32(q, t, fma=False):
    """d2[i, j] between the queries q[n] and the targets t[m] in the library's f32 expression -- outlier_ref.d2_f32, the one
    distance of both references: (dx*dx + dy*dy) + dz*dz with every operation rounded, or (fma) the fma chain"""
    q = np.asarray(q, np.float32)[:, :3]
    t = np.asarray(t, np.float32)[:, :3]
    return d2_f32(q[:, None, :], t[None, :, :], fma)


def knn_brute(q, t, k, fma=False, chunk=None):
    """exact k-NN by brute force: (idx[n, k], d2[n, k]) ascending by (d2, index); UINT32_MAX / +inf past the target.
    The non-finite rule of mvr_hip.h: a target point with a non-finite coordinate is never listed (nor is any pair whose f32
    d2 is not finite), a non-finite query gets UINT32_MAX / +inf throughout.  Queries are taken `chunk` at a time (default:
    about 2e7 distances per chunk)."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    n, m = len(q), len(t)
    idx = np.full((n, k), NONE, np.uint32)
    d2 = np.full((n, k), np.inf, np.float32)
    if m == 0 or n == 0:
        return idx, d2
    tf = np.nonzero(finite_mask(t))[0].astype(np.uint64)         # finite targets only: ascending original indices
    qf = finite_mask(q)
    if len(tf) == 0:
        return idx, d2
    T = t[tf.astype(np.int64)]
    kk = min(k, len(tf))
    step = chunk or max(1, int(2e7) // len(tf))
    for c0 in range(0, n, step):
        c1 = min(n, c0 + step)
        D = dist2_f32(q[c0:c1], T, False)
        if fma:
            D = _fma_from_plain(q[c0:c1], T, D, kk)
        with np.errstate(invalid="ignore"):
            D = np.where(np.isfinite(D), D, np.float32(np.inf))   # (a NaN from a non-finite query; an overflow)
        key = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | tf[None, :]
        if kk < key.shape[1]:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key.sort(axis=1)
        i = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        d = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
        none = np.isinf(d) | ~qf[c0:c1, None]
        idx[c0:c1, :kk] = np.where(none, NONE, i)
        d2[c0:c1, :kk] = np.where(none, np.float32(np.inf), d)
    return idx, d2


def _fma_from_plain(q, T, D, k, pad=64):
    """the fma distances that can matter for the k smallest, +inf elsewhere.  The 80-bit arithmetic of d2_f32's fma arm is
    slow, so it is spent on candidates only: both expressions start from the same rounded differences and round three times,
    so each lies within 3 * 2^-24 of the same exact sum; every entry of the fma top k therefore has a plain d2 of at most
    (1 + 1e-6) times the plain k-th.  The k + pad smallest plain d2 hold them all when the last of them is beyond that bound;
    a row where it is not (mass ties, fewer finite distances than k) is computed in full."""
    n, m = D.shape
    c = k + pad
    if c >= m:
        return d2_f32(q[:, None, :3], T[None, :, :3], True)
    with np.errstate(invalid="ignore"):
        Dp = np.where(np.isnan(D), np.float32(np.inf), D)
    cand = np.argpartition(Dp, (k - 1, c - 1), axis=1)[:, :c]
    pc = np.take_along_axis(Dp, cand, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        wide = pc[:, c - 1].astype(np.float64) > pc[:, k - 1].astype(np.float64) * (1.0 + 1e-6)
    out = np.full(D.shape, np.inf, np.float32)
    fc = d2_f32(q[:, None, :3], T[cand, :3], True)
    np.put_along_axis(out, cand, fc, 1)
    rows = np.nonzero(~wide)[0]
    if len(rows):
        out[rows] = d2_f32(q[rows][:, None, :3], T[None, :, :3], True)
    return out


def radius_sets(p, radius, fma=False):
    """neighbour lists of every point within (float)(radius * radius) under the f32 distance, the point itself included:
    (flat indices, offsets) -- candidates from a kd-tree over the FINITE points with a wide margin, then the library's exact
    rule.  A non-finite point is in no list and has an empty one (mvr_hip.h N1, N2)."""
    from scipy.spatial import cKDTree
    p = np.asarray(p, np.float32)
    r2 = np.float32(min(radius * radius, float(np.finfo(np.float32).max)))
    fin = finite_mask(p)
    fi = np.nonzero(fin)[0]
    flat, offs = [], [0]
    if len(fi) == 0:
        return np.zeros(0, np.int64), np.zeros(len(p) + 1, np.int64)
    P64 = p[fi, :3].astype(np.float64)
    tree = cKDTree(P64)
    cand = tree.query_ball_point(P64, radius * (1.0 + 1e-4) + 1e-4 + 1e-6 * float(np.abs(P64).max()))
    pos = np.full(len(p), -1, np.int64)
    pos[fi] = np.arange(len(fi))
    for i in range(len(p)):
        if not fin[i]:
            offs.append(offs[-1])
            continue
        c = fi[np.asarray(cand[pos[i]], np.int64)]
        keep = np.sort(c[within_r2(p[i, :3], p[c, :3], r2, fma)])
        flat.append(keep)
        offs.append(offs[-1] + len(keep))
    return (np.concatenate(flat) if flat else np.zeros(0, np.int64)), np.asarray(offs, np.int64)


def normals_from_sets(p, flat, offs, viewpoint=(0.0, 0.0, 0.0)):
    """normals / curvature / eigenvalues of every point from its neighbour set (flat indices, offsets)"""
    p = np.asarray(p, np.float32)
    n = len(p)
    cnt = np.diff(offs)
    q = p[:, :3].astype(np.float64)
    owner = np.repeat(np.arange(n), cnt)
    d = p[flat, :3].astype(np.float64) - q[owner]
    s1 = np.stack([np.bincount(owner, d[:, j], minlength=n) for j in range(3)], 1)
    s2 = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            s2[:, a, b] = s2[:, b, a] = np.bincount(owner, d[:, a] * d[:, b], minlength=n)
    return _solve(p, cnt, s1, s2, viewpoint)


def normals_from_lists(p, idx, viewpoint=(0.0, 0.0, 0.0), t=None):
    """the same from fixed-width neighbour lists idx[n, k] (UINT32_MAX entries are not neighbours)"""
    p = np.asarray(p, np.float32)
    t = p if t is None else np.asarray(t, np.float32)
    valid = idx != NONE
    safe = np.where(valid, idx, 0).astype(np.int64)
    d = t[safe, :3].astype(np.float64) - p[:, None, :3].astype(np.float64)
    d = np.where(valid[:, :, None], d, 0.0)
    s1 = d.sum(1)
    s2 = np.einsum("nki,nkj->nij", d, d)
    return _solve(p, valid.sum(1), s1, s2, viewpoint)


def _solve(p, cnt, s1, s2, viewpoint):
    n = len(p)
    cnt = np.asarray(cnt, np.float64)
    ok = cnt >= 3
    c = np.maximum(cnt, 1.0)
    m = s1 / c[:, None]
    C = s2 / c[:, None, None] - m[:, :, None] * m[:, None, :]
    C[~np.isfinite(C).all(axis=(1, 2))] = 0.0                   # (such a point gets NaN below)
    w, v = np.linalg.eigh(C)
    nrm = v[:, :, 0]
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    s = w.sum(1)
    curv = np.where(s != 0, np.abs(w[:, 0]) / np.where(s != 0, s, 1.0), 0.0).astype(np.float32)
    nf = nrm.astype(np.float32)
    nf = flip_towards(p, nf, viewpoint)
    ok = ok & finite_mask(p)                                    # a non-finite point: NaN normal and curvature (mvr_hip.h N4)
    nf[~ok] = np.nan
    curv[~ok] = np.nan
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = nf
    return out, curv, w


def flip_towards(p, nf, viewpoint):
    """flipNormalTowardsViewpoint in f32: cos = dot(vp - p, n); negate where cos < 0 (strictly)"""
    vp = np.asarray(viewpoint, np.float32)
    v = vp[None, :] - np.asarray(p, np.float32)[:, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        cs = (v[:, 0] * nf[:, 0] + v[:, 1] * nf[:, 1]) + v[:, 2] * nf[:, 2]
        neg = cs < 0
    nf = nf.copy()
    nf[neg] = -nf[neg]
    return nf


def knn_kdtree(p, k):
    """k-NN of a cloud against itself with scipy's kd-tree (f64 distances): (idx, d2 in f64)"""
    from scipy.spatial import cKDTree
    tree = cKDTree(np.asarray(p, np.float32)[:, :3].astype(np.float64))
    d, i = tree.query(np.asarray(p, np.float32)[:, :3].astype(np.float64), k=k, workers=16)
    return i.astype(np.int64), d * d


def angle_between(a, b, unsigned=False):
    a = np.asarray(a, np.float64)[:, :3]
    b = np.asarray(b, np.float64)[:, :3]
    c = np.sum(a * b, 1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    if unsigned:
        c = np.abs(c)
    return np.arccos(np.clip(c, -1.0, 1.0))
