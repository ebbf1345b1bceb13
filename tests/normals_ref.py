"""numpy reference of the k-NN search and of the normal estimation (include/mvr_hip.h: mvr_knn,
mvr_cloud_estimate_normals): the f32 distance expression of the library, the (d2, index) order, f64 covariance
about the query point divided by the neighbour count, numpy's eigh, PCL's f32 flip towards the viewpoint."""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)


def dist2_f32(q, t):
    """d2[i, j] = (dx*dx + dy*dy) + dz*dz in f32, every operation rounded (fma_dist = 0)"""
    q = np.asarray(q, np.float32)[:, :3]
    t = np.asarray(t, np.float32)[:, :3]
    dx = t[None, :, 0] - q[:, None, 0]
    dy = t[None, :, 1] - q[:, None, 1]
    dz = t[None, :, 2] - q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def knn_brute(q, t, k):
    """exact k-NN by brute force: (idx[n, k], d2[n, k]) ascending by (d2, index); UINT32_MAX / +inf past the target"""
    n, m = len(q), len(t)
    idx = np.full((n, k), NONE, np.uint32)
    d2 = np.full((n, k), np.inf, np.float32)
    if m == 0:
        return idx, d2
    D = dist2_f32(q, t)
    key = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(m, dtype=np.uint64)[None, :]
    key.sort(axis=1)
    kk = min(k, m)
    idx[:, :kk] = (key[:, :kk] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    d2[:, :kk] = (key[:, :kk] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2


def radius_sets(p, radius):
    """neighbour lists of every point within (float)(radius * radius) under the f32 distance, the point itself included:
    (flat indices, offsets) -- candidates from a kd-tree with a wide margin, then the library's exact rule"""
    from scipy.spatial import cKDTree
    p = np.asarray(p, np.float32)
    r2 = np.float32(radius * radius)
    tree = cKDTree(p[:, :3].astype(np.float64))
    cand = tree.query_ball_point(p[:, :3].astype(np.float64), radius * (1.0 + 1e-4) + 1e-4)
    flat, offs = [], [0]
    for i, c in enumerate(cand):
        c = np.asarray(c, np.int64)
        d = dist2_f32(p[i:i + 1], p[c])[0]
        keep = np.sort(c[d <= r2])
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
    w, v = np.linalg.eigh(C)
    nrm = v[:, :, 0]
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    s = w.sum(1)
    curv = np.where(s != 0, np.abs(w[:, 0]) / np.where(s != 0, s, 1.0), 0.0).astype(np.float32)
    nf = nrm.astype(np.float32)
    nf = flip_towards(p, nf, viewpoint)
    nf[~ok] = np.nan
    curv[~ok] = np.nan
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = nf
    return out, curv, w


def flip_towards(p, nf, viewpoint):
    """flipNormalTowardsViewpoint in f32: cos = dot(vp - p, n); negate where cos < 0 (strictly)"""
    vp = np.asarray(viewpoint, np.float32)
    v = vp[None, :] - np.asarray(p, np.float32)[:, :3]
    cs = (v[:, 0] * nf[:, 0] + v[:, 1] * nf[:, 1]) + v[:, 2] * nf[:, 2]
    nf = nf.copy()
    nf[cs < 0] = -nf[cs < 0]
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
