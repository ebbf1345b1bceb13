"""numpy reference of the FPFH descriptors (include/mvr_hip.h: mvr_cloud_fpfh, rules F1-F6).

Neighbour sets are the library's f32 rule (outlier_ref.within_r2) over candidates from a kd-tree with a widened radius -- or,
for the self-check, over all pairs.  The pair features are computed in f64 from the f32 points and normals.  The library
computes them in f32, so a pair whose f64 feature lies close to a bin edge may land in the neighbouring bin there.  Such a pair
is SLACK: it is left out of the sure counts and counted per query, and the GPU's histogram must lie between the sure counts and
the sure counts plus the slack.  A pair is slack when
  * one of its three scaled bin coordinates 11 * x lies within EDGE = 1e-3 of an integer, or
  * |v| / f4 < ILL = 1e-3: dp is nearly along n1, so v = dp x n1 is the small difference of large products, or
  * ||a1| - |a2|| < TIE = 1e-5: the swap of F3 is undecided, or
  * v is exactly 0 in f64 (no features here; f32 may find some).
A pair of coincident points (f4 == 0) gives no features on either side and is never slack.

The weighting (F6) is a function of an SPFH table and the neighbour sets; fpfh_from_spfh takes the table as an argument, so it
can be run on the library's own SPFH and pins the second pass alone."""
import numpy as np

from outlier_ref import d2_f32, within_r2

F32, F64 = np.float32, np.float64
BINS, ROW = 11, 33
EDGE, ILL, TIE = 1e-3, 1e-3, 1e-5
D_PI = F64(F32(1.0 / (2.0 * np.pi)))


def valid_mask(p, nrm):
    """F1: finite coordinates and a finite normal"""
    return np.isfinite(np.asarray(p, F32)[:, :3]).all(1) & np.isfinite(np.asarray(nrm, F32)[:, :3]).all(1)


def pairs(p, nrm, radius, fma=False, brute=False):
    """(I, J): every ordered pair of valid points with the f32 d2(i, j) <= f32(radius * radius), i == j included, sorted by
    (i, j) (F2).  brute: candidates are all pairs instead of a kd-tree's."""
    p = np.asarray(p, F32)
    ids = np.nonzero(valid_mask(p, nrm))[0]
    if len(ids) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    P = np.ascontiguousarray(p[ids, :3])
    r2 = F32(min(radius * radius, float(np.finfo(F32).max)))
    if brute:
        I, J = [a.reshape(-1) for a in np.meshgrid(np.arange(len(P)), np.arange(len(P)), indexing="ij")]
    else:
        from scipy.spatial import cKDTree
        P64 = P.astype(F64)
        cand = cKDTree(P64).query_ball_point(P64, radius * (1.0 + 1e-4) + 1e-4 + 1e-6 * float(np.abs(P64).max()), workers=-1)
        I = np.repeat(np.arange(len(P)), [len(c) for c in cand])
        J = np.concatenate([np.asarray(c, np.int64) for c in cand])
    keep = within_r2(P[I], P[J], r2, fma)
    I, J = I[keep], J[keep]
    o = np.lexsort((J, I))
    return ids[I[o]], ids[J[o]]


def _dot(a, b):
    return (a * b).sum(-1)


def pair_features(p, nrm, I, J):
    """F3 in f64 for the pairs (I, J), I != J: dict(has = the pair gives features, f = [m, 3] the features f1, f2, f3,
    coord = [m, 3] the scaled bin coordinates 11 * x of F4, bins = [m, 3] the clamped bins, slack = the pair is slack)"""
    pi, pj = np.asarray(p, F32)[I, :3].astype(F64), np.asarray(p, F32)[J, :3].astype(F64)
    ni, nj = np.asarray(nrm, F32)[I, :3].astype(F64), np.asarray(nrm, F32)[J, :3].astype(F64)
    dp = pj - pi
    f4 = np.sqrt(_dot(dp, dp))
    some = f4 > 0
    f4s = np.where(some, f4, 1.0)
    a1, a2 = _dot(ni, dp) / f4s, _dot(nj, dp) / f4s
    swap = np.abs(a1) < np.abs(a2)
    n1, n2 = np.where(swap[:, None], nj, ni), np.where(swap[:, None], ni, nj)
    dp = np.where(swap[:, None], -dp, dp)
    f3 = np.where(swap, -a2, a1)
    v = np.cross(dp, n1)
    vn = np.sqrt(_dot(v, v))
    has = some & (vn > 0)
    v = v / np.where(vn > 0, vn, 1.0)[:, None]
    w = np.cross(n1, v)
    f2 = _dot(v, n2)
    f1 = np.arctan2(_dot(w, n2), _dot(n1, n2))
    coord = BINS * np.stack([(f1 + np.pi) * D_PI, (f2 + 1.0) * 0.5, (f3 + 1.0) * 0.5], 1)
    bins = np.clip(np.floor(coord), 0, BINS - 1).astype(np.int64)
    slack = (np.abs(coord - np.rint(coord)) < EDGE).any(1) | (vn / f4s < ILL) | (np.abs(np.abs(a1) - np.abs(a2)) < TIE)
    slack &= some
    return dict(has=has & ~slack, f=np.stack([f1, f2, f3], 1), coord=coord, bins=bins, slack=slack, has_f64=has)


def spfh_counts(p, nrm, radius, fma=False, brute=False, sets=None):
    """dict(n = n_i [n], sure = [n, 3, 11] the counts of the pairs that are not slack, slack = [n] the number of slack pairs,
    full = [n, 3, 11] sure plus the slack pairs at their f64 bins, valid, I, J)"""
    p = np.asarray(p, F32)
    n = len(p)
    I, J = pairs(p, nrm, radius, fma, brute) if sets is None else sets
    cnt = np.bincount(I, minlength=n).astype(np.int64)
    o = I != J
    Io, Jo = I[o], J[o]
    sure, full = np.zeros((n, 3, BINS), np.int64), np.zeros((n, 3, BINS), np.int64)
    slack = np.zeros(n, np.int64)
    if len(Io):
        F = pair_features(p, nrm, Io, Jo)
        for f in range(3):
            np.add.at(sure[:, f, :], (Io[F["has"]], F["bins"][F["has"], f]), 1)
            both = F["has"] | (F["slack"] & F["has_f64"])
            np.add.at(full[:, f, :], (Io[both], F["bins"][both, f]), 1)
        slack = np.bincount(Io[F["slack"]], minlength=n).astype(np.int64)
    return dict(n=cnt, sure=sure, slack=slack, full=full, valid=valid_mask(p, nrm), I=I, J=J)


def spfh_from_counts(counts, n_i, valid):
    """F5: [n, 33] f32 rows from integer counts [n, 3, 11]"""
    n_i = np.asarray(n_i, np.int64)
    with np.errstate(divide="ignore"):
        scale = np.where(n_i > 1, F32(100.0) / np.maximum(n_i - 1, 1).astype(F32), F32(0.0)).astype(F32)
    out = (counts.reshape(len(counts), ROW).astype(F32) * scale[:, None]).astype(F32)
    out[~valid] = np.nan
    return out


def counts_from_spfh(spfh, n_i):
    """the integer counts [n, 3, 11] an SPFH table holds: rint(spfh * (n_i - 1) / 100) (0 for a NaN row)"""
    n_i = np.asarray(n_i, np.int64)
    with np.errstate(invalid="ignore"):
        c = np.rint(np.asarray(spfh, F32).astype(F64) * np.maximum(n_i - 1, 0)[:, None] / 100.0)
    return np.nan_to_num(c, nan=0.0).astype(np.int64).reshape(len(c), 3, BINS)


def fpfh_from_spfh(p, spfh, I, J, valid, fma=False):
    """F6 on a GIVEN SPFH table: [n, 33] f32"""
    p = np.asarray(p, F32)
    n = len(p)
    spfh = np.asarray(spfh, F32)
    acc = np.zeros((n, ROW), F64)
    if len(I):
        d2 = d2_f32(p[I, :3], p[J, :3], fma)
        with np.errstate(divide="ignore", over="ignore"):
            w = F32(1.0) / d2
        use = (d2 != 0) & np.isfinite(w)
        Iu, val = I[use], (spfh[J[use]] * w[use, None]).astype(F32)
        for k in range(ROW):
            acc[:, k] = np.bincount(Iu, weights=val[:, k].astype(F64), minlength=n)
    out = np.zeros((n, ROW), F32)
    for f in range(3):
        blk = acc[:, f * BINS:(f + 1) * BINS]
        s = blk.sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, f * BINS:(f + 1) * BINS] = np.where(s[:, None] != 0, blk * (100.0 / np.where(s != 0, s, 1.0))[:, None], 0.0).astype(F32)
    out[~valid] = np.nan
    return out


def fpfh(p, nrm, radius, fma=False, brute=False):
    """the whole reference, slack pairs at their f64 bins: (fpfh [n, 33], spfh [n, 33], the dict of spfh_counts)"""
    C = spfh_counts(p, nrm, radius, fma, brute)
    S = spfh_from_counts(C["full"], C["n"], C["valid"])
    return fpfh_from_spfh(p, S, C["I"], C["J"], C["valid"], fma), S, C
