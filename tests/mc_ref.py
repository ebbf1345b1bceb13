"""numpy restatement of the marching-cubes rules M2-M13 (include/mvr_hip.h: mvr_cloud_marching_cubes_hoppe), every operation a
single rounded f32 operation in the order the rules give, with a brute-force 1-NN in the library's f32 d2 (outlier_ref.d2_f32:
ties to the lowest index, rule N1 for non-finite points).  The case tables are NOT restated here: they are read, once, through
the library's host accessor mvr_mc_case (rule M10), and tests/test_mc_host.py is what proves them."""
import importlib

import numpy as np

from outlier_ref import d2_f32

F32 = np.float32
NONE = 0xFFFFFFFF
# M6: the corners of a cell; M8: the corners an edge joins
OFF = np.array([(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)], np.int64)
EDGE_A = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3], np.int64)
EDGE_B = np.array([1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7], np.int64)

_tables = None


def tables():
    """(edge uint16[256], tri int8[256, 16]) through mvr_mc_case"""
    global _tables
    if _tables is None:
        mvr = importlib.import_module("multi-view-registration_amd")
        rows = [mvr.mc_case(c) for c in range(256)]
        _tables = (np.array([r[0] for r in rows], np.uint16), np.stack([r[1] for r in rows]).astype(np.int8))
    return _tables


def finite_rows(p):
    return np.isfinite(np.asarray(p, F32)[:, :3]).all(1)


def box(points, res, pct):
    """M2, M3 -> (lower f32[3], size f32[3]); None without a finite point"""
    p = np.asarray(points, F32)[:, :3]
    p = p[finite_rows(p)]
    if len(p) == 0:
        return None
    lower, upper = p.min(0), p.max(0)
    ext = (F32(0.5) * F32(pct)) * (upper - lower)
    lower = lower - ext
    upper = upper + ext
    size = (upper - lower) / np.asarray(res, F32)
    assert lower.dtype == F32 and size.dtype == F32
    return lower, size


def lattice(lower, size, res):
    """M4 -> f32[rx, ry, rz, 3]"""
    ax = [lower[a] + size[a] * np.arange(res[a], dtype=F32) for a in range(3)]
    v = np.empty(tuple(res) + (3,), F32)
    v[..., 0], v[..., 1], v[..., 2] = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
    return v


def nearest(q, pts, fma=False, chunk=None):
    """mvr_nn's answer for the positions q[n, 3] in pts: (idx uint32, d2 f32); NONE / +inf when no pair has a finite d2"""
    q = np.asarray(q, F32).reshape(-1, 3)
    pts = np.asarray(pts, F32)[:, :3]
    ok = np.nonzero(finite_rows(pts))[0]
    idx, d2 = np.full(len(q), NONE, np.uint32), np.full(len(q), np.inf, F32)
    if len(ok) == 0:
        return idx, d2
    T = pts[ok]
    step = chunk or max(1, int(2e7) // len(T))
    for a in range(0, len(q), step):
        Q = q[a:a + step]
        D = d2_f32(Q[:, None, :], T[None, :, :], False)
        if fma:      # the slow arm only where it can decide (radius_ref: the two expressions differ by less than 1e-6 relative)
            lim = D.min(1).astype(np.float64) * (1.0 + 4.0e-6)
            ii, jj = np.nonzero(D.astype(np.float64) <= lim[:, None])
            D = np.full(D.shape, np.inf, F32)
            D[ii, jj] = d2_f32(Q[ii], T[jj], True)
        with np.errstate(invalid="ignore"):
            D = np.where(np.isfinite(D), D, F32(np.inf))
        j = D.argmin(1)      # the first of equal minima: the lowest index (T ascends in index)
        dj = D[np.arange(len(Q)), j]
        hit = np.isfinite(dj)
        idx[a:a + step] = np.where(hit, ok[j], NONE)
        d2[a:a + step] = dj
    return idx, d2


def values(points, normals, res, pct=0.0, dist_ignore=-1.0, fma=False):
    """M2-M5 -> (grid f32[rx, ry, rz], lower, size, idx, d2); lower / size None without a finite point"""
    res = tuple(int(r) for r in res)
    b = box(points, res, pct)
    if b is None:
        return np.full(res, np.nan, F32), None, None, None, None
    lower, size = b
    v = lattice(lower, size, res).reshape(-1, 3)
    idx, d2 = nearest(v, points, fma)
    P, N = np.asarray(points, F32)[:, :3], np.asarray(normals, F32)[:, :3]
    j = np.where(idx == NONE, 0, idx).astype(np.int64)
    n, p = N[j], P[j]
    with np.errstate(all="ignore"):
        norm = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        d = v - p
        val = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        bad = (idx == NONE) | np.isnan(n[:, 0]) | ~(norm > F32(0.5))
        if dist_ignore > 0:
            bad |= ~(d2 < F32(dist_ignore))
    assert val.dtype == F32 and norm.dtype == F32
    return np.where(bad, F32(np.nan), val).reshape(res), lower, size, idx.reshape(res), d2.reshape(res)


def march(grid, lower, size, iso=0.0):
    """M6-M9 and M13's keys -> dict(soup f32[3 T, 3], edge_key int64[3 T], cube: the cube index of every cell in M6's order,
    skipped: the cells with a NaN corner)"""
    edge, tri = tables()
    grid = np.asarray(grid, F32)
    rx, ry, rz = grid.shape
    lower, size, iso = np.asarray(lower, F32), np.asarray(size, F32), F32(iso)
    X, Y, Z = np.meshgrid(np.arange(rx - 1), np.arange(ry - 1), np.arange(rz - 1), indexing="ij")
    x, y, z = X.ravel(), Y.ravel(), Z.ravel()      # x-major, z fastest
    corner = np.stack([grid[x + o[0], y + o[1], z + o[2]] for o in OFF], 1)
    with np.errstate(invalid="ignore"):
        cube = ((corner < iso) << np.arange(8)).sum(1)
    skipped = np.isnan(corner).any(1)
    rows = tri[cube].astype(np.int64)[:, :15]
    valid = (rows >= 0) & ~skipped[:, None]
    keep = valid.any(1)
    x, y, z, rows, valid = x[keep], y[keep], z[keep], rows[keep], valid[keep]
    e = np.where(valid, rows, 0)
    a, b = EDGE_A[e], EDGE_B[e]
    oa, ob = OFF[a], OFF[b]                          # [M, 15, 3]
    cell = np.stack([x, y, z], 1)
    ia, ib = cell[:, None, :] + oa, cell[:, None, :] + ob
    va, vb = grid[ia[..., 0], ia[..., 1], ia[..., 2]], grid[ib[..., 0], ib[..., 1], ib[..., 2]]
    c0 = lower[None, :] + size[None, :] * cell.astype(F32)      # M7
    c1 = c0 + size[None, :]
    pa = np.where(oa == 1, c1[:, None, :], c0[:, None, :])
    pb = np.where(ob == 1, c1[:, None, :], c0[:, None, :])
    with np.errstate(all="ignore"):
        mu = (iso - va) / (vb - va)                  # M8
        p = pa + mu[..., None] * (pb - pa)
    assert p.dtype == F32 and mu.dtype == F32
    low = cell[:, None, :] + (oa & ob)
    axis = (oa != ob).argmax(2)
    key = 3 * ((low[..., 0] * ry + low[..., 1]) * rz + low[..., 2]) + axis
    return dict(soup=p[valid], edge_key=key[valid], cube=cube, skipped=skipped)


def weld(soup, edge_key):
    """M13 -> (vertices f32[V, 3], indices uint32[3 T])"""
    if len(edge_key) == 0:
        return np.zeros((0, 3), F32), np.zeros(0, np.uint32)
    _, first, inv = np.unique(edge_key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")         # the edges in order of first use
    newid = np.empty(len(first), np.int64)
    newid[order] = np.arange(len(first))
    return soup[first[order]], newid[inv].astype(np.uint32)


def reconstruct(points, normals, res, iso=0.0, pct=0.0, dist_ignore=-1.0, fma=False):
    """the whole of mvr_cloud_marching_cubes_hoppe -> dict(grid, soup, edge_key, vertices, indices, lower, size, d2)"""
    grid, lower, size, _, d2 = values(points, normals, res, pct, dist_ignore, fma)
    if lower is None:
        m = dict(soup=np.zeros((0, 3), F32), edge_key=np.zeros(0, np.int64))
    else:
        m = march(grid, lower, size, iso)
    v, i = weld(m["soup"], m["edge_key"])
    return dict(grid=grid, soup=m["soup"], edge_key=m["edge_key"], vertices=v, indices=i, lower=lower, size=size, d2=d2)


# ---- what a mesh is checked for

def closed_and_oriented(indices):
    """every directed edge of the triangles once, and its reverse once"""
    t = np.asarray(indices, np.int64).reshape(-1, 3)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    n = int(max(a.max(), b.max())) + 1 if len(a) else 1
    fwd, cnt = np.unique(a * n + b, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(fwd, np.unique(b * n + a)))


def euler(n_vertices, indices):
    t = np.asarray(indices, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    return n_vertices - len(np.unique(e, axis=0)) + len(t)


def signed_volume(vertices, indices):
    v = np.asarray(vertices, np.float64)[np.asarray(indices, np.int64).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def same_bits(a, b):
    """f32 arrays equal bit for bit, every NaN counting as the same NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
