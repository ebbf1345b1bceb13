"""numpy reference of the PFH descriptors (include/mvr_hip.h: mvr_cloud_pfh, rules P1-P8), on top of tests/fpfh_ref.py.

A neighbourhood is a list of (query i, neighbour j, f32 d2 bits): in radius mode fpfh_ref.pairs with the library's f32 distance
(P2, rule F2), in k mode the entries of a k-NN table (the library's own, or knn_lists below) whose normal is finite.  Inside a
neighbourhood the members are ordered by the key (d2 bits, index) and every pair (earlier, later) gets the features of
fpfh_ref.pair_features with the later member in the role of "i" (P3), computed in f64 from the f32 inputs.  The library
computes them in f32, so the slack method of fpfh_ref.py carries over, per PAIR.  A pair is slack when
  * one of its three scaled bin coordinates 5 * x lies within EDGE of an integer, or
  * ILL or TIE of fpfh_ref.py holds (or v is exactly 0 in f64: no features here, f32 may find some), or
  * its two keys tie in d2 and the two orders give different outcomes (the key decides by index, on the GPU as here: listed
    for completeness, the candidate set holds both orders).
A slack pair is left out of the sure counts and records the set of joint bins it may land in: both neighbouring bins of every
near-edge coordinate (their product over the three coordinates), both orders of a key tie, and every one of the 125 bins for an
ILL or TIE pair, whose features f32 cannot be held to at all.  `maybe[q, h]` counts the slack pairs of query q whose set holds
h: the GPU's c[q, h] must lie in [sure, sure + maybe], and its total in [sum sure, sum sure + slack].

naive() is a second, deliberately plain transcription of PCL's double loop (computePointPFHSignature) in pure Python floats,
for the host self-check of the vectorised code."""
import math

import numpy as np

import fpfh_ref as R
from outlier_ref import d2_f32

F32, F64 = np.float32, np.float64
SUB, DIM = 5, 125
EDGE, ILL, TIE = R.EDGE, R.ILL, R.TIE
NONE = np.uint32(0xFFFFFFFF)


def d2_bits(d2):
    return np.ascontiguousarray(d2, F32).view(np.uint32).astype(np.int64)


# ------------------------------------------------------------------ neighbourhoods (P2)

def hoods_radius(p, nrm, radius, fma=False, brute=False):
    """(I, J, bits): every valid j within the f32 radius of every valid i, i included"""
    I, J = R.pairs(p, nrm, radius, fma, brute)
    p = np.asarray(p, F32)
    return I, J, d2_bits(d2_f32(p[I, :3], p[J, :3], fma))


def knn_lists(p, k, fma=False):
    """mvr_knn of a small cloud in itself by brute force: (idx [n, k] uint32, d2 [n, k] f32), rules N1-N3"""
    p = np.asarray(p, F32)
    n = len(p)
    idx, d2 = np.full((n, k), NONE, np.uint32), np.full((n, k), np.inf, F32)
    fin = np.isfinite(p[:, :3]).all(1)
    for i in np.nonzero(fin)[0]:
        d = d2_f32(p[i, None, :3], p[:, :3], fma)
        ok = np.nonzero(fin & np.isfinite(d))[0]
        o = ok[np.lexsort((ok, d2_bits(d[ok])))][:k]
        idx[i, :len(o)], d2[i, :len(o)] = o, d[o]
    return idx, d2


def hoods_knn(p, nrm, idx, d2):
    """(I, J, bits) from a k-NN table: the listed entries whose normal is finite, for the valid queries"""
    v = R.valid_mask(p, nrm)
    n, k = idx.shape
    I = np.repeat(np.arange(n, dtype=np.int64), k)
    J, b = idx.reshape(-1).astype(np.int64), d2_bits(d2.reshape(-1))
    nf = np.isfinite(np.asarray(nrm, F32)[:, :3]).all(1)
    keep = (idx.reshape(-1) != NONE) & v[I]
    keep[keep] &= nf[J[keep]]
    return I[keep], J[keep], b[keep]


# ------------------------------------------------------------------ pairs (P3) and bins (P4)

def _ordered_pairs(I, J, bits, queries):
    """every pair of every neighbourhood of `queries`: (query position, earlier member, later member, the keys tie in d2)"""
    sel = np.isin(I, queries)
    I, J, bits = I[sel], J[sel], bits[sel]
    o = np.lexsort((J, bits, I))
    I, J, bits = I[o], J[o], bits[o]
    qpos = np.searchsorted(queries, I)
    size = np.bincount(qpos, minlength=len(queries))
    start = np.concatenate([[0], np.cumsum(size)[:-1]])
    Q, A, B = [], [], []
    for s in np.unique(size):
        if s < 2:
            continue
        g = np.nonzero(size == s)[0]
        a, b = np.triu_indices(int(s), 1)
        Q.append(np.repeat(g, len(a)))
        A.append((start[g][:, None] + a[None, :]).reshape(-1))
        B.append((start[g][:, None] + b[None, :]).reshape(-1))
    if not Q:
        z = np.zeros(0, np.int64)
        return z, z, z, np.zeros(0, bool), size
    Q, A, B = np.concatenate(Q), np.concatenate(A), np.concatenate(B)
    return Q, J[A], J[B], bits[A] == bits[B], size


def _features(p, nrm, later, earlier):
    """the features of fpfh_ref.pair_features for (i = later, j = earlier) at 5 subdivisions: dict(has, joint, coord, slack,
    wild = the slack is ILL / TIE / a zero v: no bin can be named)"""
    F = R.pair_features(p, nrm, later, earlier)
    f = F["f"]
    coord = SUB * np.stack([(f[:, 0] + np.pi) * R.D_PI, (f[:, 1] + 1.0) * 0.5, (f[:, 2] + 1.0) * 0.5], 1)
    bins = np.clip(np.floor(coord), 0, SUB - 1).astype(np.int64)
    # ILL and TIE again (pair_features folds them into its 11-bin slack)
    P, N = np.asarray(p, F32)[:, :3].astype(F64), np.asarray(nrm, F32)[:, :3].astype(F64)
    dp = P[earlier] - P[later]
    f4 = np.sqrt((dp * dp).sum(1))
    some = f4 > 0
    f4s = np.where(some, f4, 1.0)
    a1, a2 = (N[later] * dp).sum(1) / f4s, (N[earlier] * dp).sum(1) / f4s
    n1 = np.where((np.abs(a1) < np.abs(a2))[:, None], N[earlier], N[later])
    vn = np.sqrt((np.cross(dp, n1) ** 2).sum(1))
    wild = some & ((vn / f4s < ILL) | (np.abs(np.abs(a1) - np.abs(a2)) < TIE) | ~F["has_f64"])
    edge = some & (np.abs(coord - np.rint(coord)) < EDGE).any(1)
    slack = wild | edge
    return dict(has=F["has_f64"] & ~slack, has_f64=F["has_f64"], joint=bins[:, 0] + SUB * bins[:, 1] + SUB * SUB * bins[:, 2],
                coord=coord, slack=slack, wild=wild)


def _candidates(coord, wild):
    """[m, 125] the joint bins a slack pair may land in"""
    lo = np.clip(np.floor(coord - EDGE), 0, SUB - 1).astype(np.int64)
    hi = np.clip(np.floor(coord + EDGE), 0, SUB - 1).astype(np.int64)
    ar = np.arange(SUB)
    m = [(ar[None, :] == lo[:, d, None]) | (ar[None, :] == hi[:, d, None]) for d in range(3)]
    out = (m[2][:, :, None, None] & m[1][:, None, :, None] & m[0][:, None, None, :]).reshape(len(coord), DIM)
    out[wild] = True
    return out


def counts(p, nrm, hoods, queries=None):
    """P3-P5 for the neighbourhoods `hoods` = (I, J, bits): dict(queries, n = n_i, m = m_i, sure [q, 125], maybe [q, 125],
    slack [q] = slack pairs, full [q, 125] = sure plus the slack pairs at their f64 bins, feat [q] = pairs with features in f64,
    pairs = all pairs, valid [q]); rows follow `queries` (default: every point)"""
    p, nrm = np.asarray(p, F32), np.asarray(nrm, F32)
    I, J, bits = hoods
    queries = np.arange(len(p)) if queries is None else np.asarray(queries, np.int64)
    nq = len(queries)
    Q, E, L, tie, size = _ordered_pairs(I, J, bits, queries)
    sure, maybe, full = (np.zeros((nq, DIM), np.int64) for _ in range(3))
    slack, feat = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    if len(Q):
        F = _features(p, nrm, L, E)
        sl = F["slack"].copy()
        if tie.any():                                  # both orders of a key tie
            t = np.nonzero(tie)[0]
            G = _features(p, nrm, E[t], L[t])
            differ = (G["has_f64"] != F["has_f64"][t]) | (G["joint"] != F["joint"][t]) | G["slack"]
            sl[t[differ]] = True
        s = np.nonzero(sl)[0]
        cand = _candidates(F["coord"][s], F["wild"][s])
        if tie.any():
            ts = np.nonzero(tie[s])[0]
            if len(ts):
                G = _features(p, nrm, E[s[ts]], L[s[ts]])
                cand[ts] |= _candidates(G["coord"], G["wild"])
        ok = F["has_f64"] & ~sl
        np.add.at(sure, (Q[ok], F["joint"][ok]), 1)
        full += sure
        both = sl & F["has_f64"]
        np.add.at(full, (Q[both], F["joint"][both]), 1)
        for h in range(DIM):
            maybe[:, h] = np.bincount(Q[s][cand[:, h]], minlength=nq)
        slack = np.bincount(Q[s], minlength=nq).astype(np.int64)
        feat = np.bincount(Q[F["has_f64"]], minlength=nq).astype(np.int64)
    n = size.astype(np.int64)
    return dict(queries=queries, n=n, m=n * (n - 1) // 2, sure=sure, maybe=maybe, slack=slack, full=full, feat=feat,
                pairs=int(len(Q)), valid=R.valid_mask(p, nrm)[queries])


def rows_from_counts(c, n, valid):
    """P5: [q, 125] f32 rows from integer counts: (float)c * (100.0f / (float)m_i); n_i == 1: zeros; n_i == 0 or invalid: NaN"""
    n = np.asarray(n, np.uint64)
    m = n * np.maximum(n, 1) - n
    m //= 2
    with np.errstate(divide="ignore"):
        scale = np.where(m > 0, F32(100.0) / np.maximum(m, 1).astype(F32), F32(0.0)).astype(F32)
    out = (np.asarray(c).astype(F32) * scale[:, None]).astype(F32)
    out[(n == 0) | ~np.asarray(valid, bool)] = np.nan
    return out


def pfh(p, nrm, radius=None, k=None, fma=False, brute=False, queries=None):
    """the whole reference, slack pairs at their f64 bins: (rows [q, 125], the dict of counts)"""
    if k is None:
        hoods = hoods_radius(p, nrm, radius, fma, brute)
    else:
        hoods = hoods_knn(p, nrm, *knn_lists(p, k, fma))
    C = counts(p, nrm, hoods, queries)
    return rows_from_counts(C["full"], C["n"], C["valid"]), C


# ------------------------------------------------------------------ the naive transcription

def _pair_features_plain(p1, n1, p2, n2):
    """pcl::computePairFeatures(p1, n1, p2, n2) in Python floats: (f1, f2, f3, f4) or None"""
    dp = [p2[c] - p1[c] for c in range(3)]
    f4 = math.sqrt(sum(x * x for x in dp))
    if f4 == 0.0:
        return None
    a1 = sum(n1[c] * dp[c] for c in range(3)) / f4
    a2 = sum(n2[c] * dp[c] for c in range(3)) / f4
    if abs(a1) < abs(a2):                               # PCL: acos(fabs(a1)) > acos(fabs(a2))
        n1, n2 = n2, n1
        dp = [-x for x in dp]
        f3 = -a2
    else:
        f3 = a1
    v = [dp[1] * n1[2] - dp[2] * n1[1], dp[2] * n1[0] - dp[0] * n1[2], dp[0] * n1[1] - dp[1] * n1[0]]
    vn = math.sqrt(sum(x * x for x in v))
    if vn == 0.0:
        return None
    v = [x / vn for x in v]
    w = [n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0]]
    f2 = sum(v[c] * n2[c] for c in range(3))
    f1 = math.atan2(sum(w[c] * n2[c] for c in range(3)), sum(n1[c] * n2[c] for c in range(3)))
    return f1, f2, f3, f4


def naive(p, nrm, hoods, queries):
    """PCL's double loop over the sorted neighbour list of each query: [q, 125] integer counts (f64 bins, nothing slack)"""
    I, J, bits = hoods
    P = [[float(x) for x in r[:3]] for r in np.asarray(p, F32)]
    N = [[float(x) for x in r[:3]] for r in np.asarray(nrm, F32)]
    d_pi = float(F32(1.0 / (2.0 * math.pi)))
    out = np.zeros((len(queries), DIM), np.int64)
    for row, q in enumerate(queries):
        sel = np.nonzero(I == q)[0]
        idx = [int(J[s]) for s in sorted(sel, key=lambda s: (int(bits[s]), int(J[s])))]
        for i_idx in range(len(idx)):
            for j_idx in range(i_idx):
                f = _pair_features_plain(P[idx[i_idx]], N[idx[i_idx]], P[idx[j_idx]], N[idx[j_idx]])
                if f is None:
                    continue
                x = ((f[0] + math.pi) * d_pi, (f[1] + 1.0) * 0.5, (f[2] + 1.0) * 0.5)
                b = [min(max(int(math.floor(SUB * v)), 0), SUB - 1) for v in x]
                out[row, b[0] + SUB * b[1] + SUB * SUB * b[2]] += 1
    return out
