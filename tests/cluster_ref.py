"""numpy reference of the Euclidean cluster extraction (rules E1-E8 of mvr_cloud_euclidean_clusters in include/mvr_hip.h): the
link matrix over ALL pairs -- the library's f32 distance in its order of operations (outlier_ref.within_r2; fma through the
80-bit emulation the other references use), the f64 dot of E3 operation by operation -- then the connected components of that
graph (scipy), then E5 (which components are clusters), E6 (their order) and E7 (lists, offsets, labels, the kept points).
There is no grid in it: it shares nothing with the kernels under test."""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from outlier_ref import within_r2

F32, F64 = np.float32, np.float64
NONE = np.uint32(0xFFFFFFFF)
F32_MAX = float(np.finfo(F32).max)


def r2_of(tolerance):
    """(float)(tolerance * tolerance), kept finite (clamp_r2)"""
    return F32(min(float(tolerance) * float(tolerance), F32_MAX))


def active_mask(n, index=None, negative=False):
    """E1"""
    if index is None:
        return np.ones(n, bool)
    a = np.zeros(n, bool)
    a[np.asarray(index, np.int64)] = True
    return ~a if negative else a


def dot_f64(a, b):
    """E3's dot of f32 normals: ((double)a.x * b.x + (double)a.y * b.y) + (double)a.z * b.z"""
    a, b = np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def link_pairs(p, tolerance, normals=None, eps_angle=None, active=None, fma=False, chunk=512):
    """(i, j) of every linked pair, i < j: E2 (and E3 with normals) between active points"""
    P = np.ascontiguousarray(np.asarray(p, F32)[:, :3])
    n = len(P)
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    ok = act & np.isfinite(P).all(axis=1)
    r2 = r2_of(tolerance)
    cos_eps = math.cos(float(eps_angle)) if normals is not None else None
    I, J = [], []
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        L = within_r2(P[c0:c1, None, :], P[None, :, :], r2, fma)
        L &= ok[c0:c1, None] & ok[None, :]
        if normals is not None:
            N = np.asarray(normals, F32)
            with np.errstate(invalid="ignore"):
                L &= dot_f64(N[c0:c1, None, :], N[None, :, :]) > cos_eps      # (a NaN dot: False)
        i, j = np.nonzero(L)
        i = i + c0
        m = i < j
        I.append(i[m]); J.append(j[m])
    return (np.concatenate(I), np.concatenate(J)) if I else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def roots_of(n, i, j):
    """root[k] = the smallest index of k's component in the graph of the pairs (i, j)"""
    if n == 0:
        return np.zeros(0, np.int64)
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab]


def clusters(p, tolerance, min_size=1, max_size=2 ** 31 - 1, normals=None, eps_angle=None, index=None, negative=False, keep=1,
             fma=False):
    """dict(result = the fields of mvr_cluster_result, lists = the clusters' member arrays in E6's order, offsets, index =
    their concatenation, labels[n], kept = the ascending indices dst_slot receives with `keep`)"""
    n = len(p)
    act = active_mask(n, index, negative)
    i, j = link_pairs(p, tolerance, normals if eps_angle is not None else None, eps_angle, act, fma)
    root = roots_of(n, i, j)
    comp_roots, sizes = np.unique(root[act], return_counts=True)          # inactive points are singletons nobody reports
    lo = max(int(min_size), 1)
    small = sizes < lo
    large = ~small & (sizes > int(max_size))
    is_cluster = ~small & ~large
    cr, cs = comp_roots[is_cluster], sizes[is_cluster]
    order = np.lexsort((cr, -cs))                                           # E6: size descending, then root ascending
    cr, cs = cr[order], cs[order]
    lists = [np.nonzero(act & (root == r))[0].astype(np.uint32) for r in cr]
    labels = np.full(n, NONE, np.uint32)
    for k, m in enumerate(lists):
        labels[m] = k
    offsets = np.concatenate([[0], np.cumsum(cs)]).astype(np.uint32)
    result = dict(n_active=int(act.sum()), n_components=int(len(comp_roots)), n_clusters=int(len(cr)), n_clustered=int(cs.sum()),
                  largest=int(cs[0]) if len(cs) else 0, too_small=int(small.sum()), too_large=int(large.sum()))
    kept = np.nonzero(labels < np.uint32(min(int(keep), len(lists))))[0] if lists else np.zeros(0, np.int64)
    return dict(result=result, lists=lists, offsets=offsets, index=np.concatenate(lists) if lists else np.zeros(0, np.uint32),
                labels=labels, kept=kept)
