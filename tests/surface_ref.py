"""numpy reference of the features at query points over a search surface (include/mvr_hip.h: mvr_cloud_estimate_normals_at,
mvr_cloud_fpfh_at, mvr_cloud_pfh_at, rules Q1-Q8), on top of the references of the calls they generalise: the neighbourhoods of
tests/radius_ref.py and tests/normals_ref.py (the library's f32 distance, the key (d2, index)), the weighting of tests/fpfh_ref.py,
the pair counts of tests/pfh_ref.py, the plane fit of tests/normals_ref.py.

A query is a row of `q` (positions only: rule Q2 for a query slot other than the surface); the surface is (t, tn) = points and
normals.  A neighbourhood is (I = row of the query, J = index in the surface, d2 f32)."""
import numpy as np

import fpfh_ref as R
import normals_ref as NR
import pfh_ref as PR
import radius_ref as RR

F32, F64 = np.float32, np.float64
ROW = R.ROW


def hoods_radius(q, t, tn=None, radius=1.0, fma=False):
    """Q3, radius mode: every surface point within the f32 radius of every query, in the order of the key (d2, index); with
    normals `tn`, the valid points only (F2 / P2).  A non-finite query has none."""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    off, idx, d2 = RR.radius_search(q, t, radius, fma=fma)
    I = np.repeat(np.arange(len(q), dtype=np.int64), np.diff(off.astype(np.int64)))
    J = idx.astype(np.int64)
    if tn is not None and len(J):
        keep = R.valid_mask(t, tn)[J]
        I, J, d2 = I[keep], J[keep], d2[keep]
    return I, J, np.ascontiguousarray(d2, F32)


def hoods_knn(q, t, tn, k, fma=False):
    """Q3, k mode (PFH): the listed entries of the k-NN lists of the queries in the surface whose normal is finite"""
    idx, d2 = NR.knn_brute(q, t, k, fma)
    I = np.repeat(np.arange(len(idx), dtype=np.int64), k)
    J, d = idx.reshape(-1).astype(np.int64), d2.reshape(-1)
    keep = idx.reshape(-1) != NR.NONE
    if keep.any():
        keep[keep] &= np.isfinite(np.asarray(tn, F32)[J[keep], :3]).all(1)
    return I[keep], J[keep], np.ascontiguousarray(d[keep], F32)


def neighbor_count(rows, I):
    return np.bincount(I, minlength=rows).astype(np.int64)


def fpfh_from_spfh(rows, spfh, I, J, d2):
    """F6 over the neighbourhoods of the queries, on a GIVEN SPFH table of the surface (by surface index): [rows, 33] f32; a
    query without a neighbour gets 33 NaN (Q4)"""
    spfh = np.asarray(spfh, F32)
    acc = np.zeros((rows, ROW), F64)
    if len(I):
        with np.errstate(divide="ignore", over="ignore"):
            w = F32(1.0) / d2
        use = (d2 != 0) & np.isfinite(w)
        Iu, val = I[use], (spfh[J[use]] * w[use, None]).astype(F32)
        for k in range(ROW):
            acc[:, k] = np.bincount(Iu, weights=val[:, k].astype(F64), minlength=rows)
    out = np.zeros((rows, ROW), F32)
    for f in range(3):
        blk = acc[:, f * R.BINS:(f + 1) * R.BINS]
        s = blk.sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, f * R.BINS:(f + 1) * R.BINS] = np.where(s[:, None] != 0, blk * (100.0 / np.where(s != 0, s, 1.0))[:, None], 0.0).astype(F32)
    out[neighbor_count(rows, I) == 0] = np.nan
    return out


def pfh_counts(rows, t, tn, I, J, d2, queries=None):
    """P3-P5 on the neighbourhoods of the queries (`queries`: of those rows alone): the dict of pfh_ref.counts, its rows the queries.  (pfh_ref.counts looks
    points up by J alone; its `valid` is that of the surface points 0..rows - 1 and means nothing here, so the surface is
    padded to `rows` points for it and the entry dropped.)"""
    t, tn = np.asarray(t, F32), np.asarray(tn, F32)
    if len(t) < rows:
        pad = np.full((rows - len(t), 4), np.nan, F32)
        t, tn = np.concatenate([t.reshape(-1, 4), pad]), np.concatenate([tn.reshape(-1, 4), pad])
    C = PR.counts(t, tn, (I, J, PR.d2_bits(d2)), np.arange(rows) if queries is None else np.asarray(queries, np.int64))
    del C["valid"]
    return C


def normals_from_sets(q, t, I, J, viewpoint=(0.0, 0.0, 0.0)):
    """normals_ref.normals_from_sets for a query array: the moments of the surface points J about the query I"""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    n = len(q)
    d = t[J, :3].astype(F64) - q[I, :3].astype(F64)
    s1 = np.stack([np.bincount(I, d[:, j], minlength=n) for j in range(3)], 1)
    s2 = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            s2[:, a, b] = s2[:, b, a] = np.bincount(I, d[:, a] * d[:, b], minlength=n)
    return NR._solve(q, neighbor_count(n, I), s1, s2, viewpoint)


def normals_from_lists(q, t, k, viewpoint=(0.0, 0.0, 0.0), fma=False):
    """normals_ref.normals_from_lists on the k-NN lists of the queries in the surface"""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    idx, _ = NR.knn_brute(q, t, k, fma)
    if len(t) == 0:
        t = np.zeros((1, 4), F32)      # (nothing is listed: any row serves the lookup of the unlisted entries)
    return NR.normals_from_lists(q, idx, viewpoint, t=t)
