"""numpy restatement of mvr_cloud_voxel_grid (include/mvr_hip.h, rules 1-8): pcl::VoxelGrid with PCL's f32 voxel
arithmetic, a 64-bit voxel index, a stable sort, f64 centroids and normalised f64 normal sums."""
import numpy as np

NONE = 0xFFFFFFFF
F32 = np.float32


def leaf3(leaf):
    lf = np.asarray(leaf, F32).reshape(-1)
    return np.repeat(lf, 3) if lf.size == 1 else lf


def overflow(p, leaf):
    """(passthrough, geometry) of rule 3 for the finite points of p; geometry = (inv, min_b, div) or None"""
    inv = (F32(1.0) / leaf3(leaf)).astype(F32)
    xyz = np.asarray(p, F32)[:, :3]
    q = xyz[np.isfinite(xyz).all(1)]
    if len(q) == 0:
        return False, None
    mn, mx = q.min(0), q.max(0)
    with np.errstate(over="ignore", invalid="ignore"):
        prod = (mx - mn).astype(F32) * inv                 # f32 difference, f32 product
        lo, hi = mn * inv, mx * inv
    d = []
    for a in range(3):
        if not (prod[a] < F32(2.0 ** 31)) or not (abs(lo[a]) < F32(2.0 ** 62)) or not (abs(hi[a]) < F32(2.0 ** 62)):
            return True, None
        d.append(int(prod[a]) + 1)
    if d[0] * d[1] * d[2] > 2 ** 31 - 1:
        return True, None
    min_b = np.floor(lo).astype(np.int64)
    max_b = np.floor(hi).astype(np.int64)
    div = [int(max_b[a] - min_b[a] + 1) for a in range(3)]
    top = [int(F32(max_b[a]) - F32(min_b[a])) for a in range(3)]       # the largest ijk of an axis (f32 difference)
    if top[0] + top[1] * div[0] + top[2] * div[0] * div[1] + 1 >= 2 ** 64:  # last guard: an index beyond 64 bits
        return True, None
    return False, (inv, min_b, max_b - min_b + 1)


def voxel_index(q, inv, min_b, div):
    """64-bit voxel index of finite points q (n, 3) f32"""
    f = np.floor(q.astype(F32) * inv) - min_b.astype(F32)   # f32 products and floors, f32 difference
    ijk = f.astype(np.uint64)
    d0, d1 = np.uint64(div[0]), np.uint64(div[1])
    return ijk[:, 0] + ijk[:, 1] * d0 + ijk[:, 2] * (d0 * d1)


def unit(s):
    """f64 sums (m, 3) -> normalised, rounded to f32; a zero sum stays 0, NaN stays NaN"""
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        u = s / ln[:, None]
    u[ln == 0] = 0.0
    return u.astype(F32)


def voxel_grid(p, leaf, min_points=0, normals=None):
    """-> dict(pts (m, 4) f32 w = 1, nrm (m, 4) f32 w = 0 or None, voxel_of (n,) u32, passthrough, idx (m,) u64 of the kept
    voxels, counts (m,))"""
    p = np.ascontiguousarray(p, F32)
    n = len(p)
    nr = None if normals is None else np.ascontiguousarray(normals, F32)
    empty = dict(pts=np.zeros((0, 4), F32), nrm=None, voxel_of=np.full(n, NONE, np.uint32), passthrough=False,
                 idx=np.zeros(0, np.uint64), counts=np.zeros(0, np.int64))
    if n == 0:
        return empty
    passthrough, geo = overflow(p, leaf)
    if passthrough:
        out = np.ones((n, 4), F32)
        out[:, :3] = p[:, :3]
        nro = None
        if nr is not None:
            nro = np.zeros((n, 4), F32)
            nro[:, :3] = nr[:, :3]
        return dict(pts=out, nrm=nro, voxel_of=np.arange(n, dtype=np.uint32), passthrough=True, idx=None, counts=None)
    if geo is None:
        return empty
    inv, min_b, div = geo
    fin = np.nonzero(np.isfinite(p[:, :3]).all(1))[0]
    idx = voxel_index(p[fin, :3], inv, min_b, div)
    order = np.argsort(idx, kind="stable")
    sk = idx[order]
    heads = np.r_[True, sk[1:] != sk[:-1]]
    starts = np.nonzero(heads)[0]
    counts = np.diff(np.r_[starts, len(sk)])
    keep = counts >= min_points
    src = fin[order]
    sums = np.add.reduceat(p[src, :3].astype(np.float64), starts, axis=0)
    cent = (sums / counts[:, None].astype(np.float64)).astype(F32)
    pts = np.ones((int(keep.sum()), 4), F32)
    pts[:, :3] = cent[keep]
    nro = None
    if nr is not None:
        ns = np.add.reduceat(nr[src, :3].astype(np.float64), starts, axis=0)
        nro = np.zeros((int(keep.sum()), 4), F32)
        nro[:, :3] = unit(ns)[keep]
    pos = np.where(keep, np.cumsum(keep) - 1, NONE).astype(np.uint32)
    voxel_of = np.full(n, NONE, np.uint32)
    voxel_of[src] = pos[np.cumsum(heads) - 1]
    return dict(pts=pts, nrm=nro, voxel_of=voxel_of, passthrough=False, idx=sk[starts][keep], counts=counts[keep])


def rich_average(voxel_of, m, rgb, curvature):
    """ScanCloud::voxelDownsample's host side: rgb (n, 3) u8 -> per-channel integer mean (truncated), curvature (n,) f32 ->
    f64 mean rounded to f32, over the points of each of the m output voxels"""
    ok = voxel_of != NONE
    o = voxel_of[ok].astype(np.int64)
    cnt = np.bincount(o, minlength=m)
    out_rgb = np.zeros((m, 3), np.uint8)
    for c in range(3):
        s = np.bincount(o, weights=rgb[ok, c].astype(np.float64), minlength=m).astype(np.int64)
        out_rgb[:, c] = (s // np.maximum(cnt, 1)).astype(np.uint8)
    cs = np.zeros(m, np.float64)
    np.add.at(cs, o, curvature[ok].astype(np.float64))
    return out_rgb, (cs / np.maximum(cnt, 1)).astype(F32)
