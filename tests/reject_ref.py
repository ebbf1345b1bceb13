"""numpy restatement of the rejector rules R2-R6 of include/mvr_hip.h (mvr_correspondences_rejected) on (query, match, d2)
arrays; independent of the library.  A chain is a list of tuples: ("distance", max_distance), ("median", factor),
("trimmed", ratio[, min_correspondences]), ("surface_normal", cosine), ("one_to_one",).  The order statistics are taken with
np.lexsort on (query, d2 bits): non-negative floats order as their bit patterns, and the query index breaks ties (R4, R6)."""
import math

import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32
KINDS = ("distance", "median", "trimmed", "surface_normal", "one_to_one")


def bits(d2):
    return np.ascontiguousarray(d2, F32).view(U32)


def dot_f32(n, t):
    """R5: (n.x * t.x + n.y * t.y) + n.z * t.z, every operation rounded to f32"""
    n, t = np.asarray(n, F32), np.asarray(t, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((n[:, 0] * t[:, 0]).astype(F32) + (n[:, 1] * t[:, 1]).astype(F32)).astype(F32) + (n[:, 2] * t[:, 2]).astype(F32)


def trimmed_count(value, m, min_correspondences=0):
    """R4's nv"""
    f = math.floor(float(value) * float(m))
    nv = 0xFFFFFFFF if f >= 4294967295.0 else int(f)
    return max(nv, int(min_correspondences))


def stage(q, m, d2, rej, src_normals=None, tgt_normals=None):
    """one stage on the live list -> (keep mask, threshold f32)"""
    kind, n = rej[0], len(q)
    value = float(rej[1]) if len(rej) > 1 else 0.0
    thr = F32(0.0)
    if kind == "distance":
        keep = d2.astype(F64) < value * value
    elif kind == "median":
        keep = np.ones(n, bool)
        if n:
            order = np.lexsort((q, bits(d2)))
            thr = d2[order[n // 2]]
            keep = d2.astype(F64) <= F64(thr) * value
    elif kind == "trimmed":
        keep = np.ones(n, bool)
        if n:
            nv = trimmed_count(value, n, rej[2] if len(rej) > 2 else 0)
            if nv == 0:
                keep[:] = False
            else:
                k = min(nv, n)
                order = np.lexsort((q, bits(d2)))
                keep[:] = False
                keep[order[:k]] = True
                thr = d2[order[k - 1]]
    elif kind == "surface_normal":
        with np.errstate(invalid="ignore"):
            keep = dot_f32(src_normals[q], tgt_normals[m]).astype(F64) > value
    elif kind == "one_to_one":
        keep = np.zeros(n, bool)
        if n:
            order = np.lexsort((q, bits(d2), m))
            first = np.ones(n, bool)
            first[1:] = m[order][1:] != m[order][:-1]
            keep[order[first]] = True
    else:
        raise ValueError(kind)
    return keep, F32(thr)


def apply_chain(query, match, d2, chain, src_normals=None, tgt_normals=None):
    """-> (query, match, d2, stages) in ascending query index; stages = [dict(n_in, n_out, threshold)]"""
    q, m, d = np.asarray(query, np.int32), np.asarray(match, np.int32), np.asarray(d2, F32)
    o = np.argsort(q, kind="stable")
    q, m, d = q[o], m[o], d[o]
    stages = []
    for rej in chain:
        keep, thr = stage(q, m, d, rej, src_normals, tgt_normals)
        stages.append(dict(n_in=len(q), n_out=int(keep.sum()), threshold=thr))
        q, m, d = q[keep], m[keep], d[keep]
    return q, m, d, stages


# ---- what the host test holds the reference against: plain loops

def naive_median(d2):
    return sorted(float(x) for x in d2)[len(d2) // 2]


def naive_one_to_one(q, m, d2):
    best = {}
    for i, j, d in zip(q.tolist(), m.tolist(), bits(d2).tolist()):
        if j not in best or (d, i) < best[j]:
            best[j] = (d, i)
    return sorted(i for d, i in best.values())


def naive_trimmed(q, d2, nv):
    keyed = sorted(zip(bits(d2).tolist(), q.tolist()))
    return sorted(i for _, i in keyed[:nv])


def brute_correspondences(src, tgt, max_dist, reciprocal):
    """determine(Reciprocal)Correspondences by exhaustive search in f32 ((dx dx + dy dy) + dz dz, ties to the lowest index); for
    the conditions of the cases, not for bits"""
    s, t = np.asarray(src, F32)[:, :3], np.asarray(tgt, F32)[:, :3]
    ns, nt = len(s), len(t)
    if ns == 0 or nt == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, F32)
    fwd, fd = np.empty(ns, np.int64), np.empty(ns, F32)
    rbest, rd = np.zeros(nt, np.int64), np.full(nt, np.inf, F32)
    step = max(1, (1 << 24) // nt)
    for a in range(0, ns, step):
        d = s[a:a + step, None, :] - t[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        fwd[a:a + step] = d2.argmin(1)
        fd[a:a + step] = d2[np.arange(len(d2)), fwd[a:a + step]]
        cm = d2.argmin(0)
        cd = d2[cm, np.arange(nt)]
        better = cd < rd
        rbest[better], rd[better] = cm[better] + a, cd[better]
    ok = ~(fd.astype(F64) > max_dist * max_dist)
    if reciprocal:
        ok &= rbest[fwd] == np.arange(ns)
    q = np.nonzero(ok)[0]
    return q.astype(np.int32), fwd[q].astype(np.int32), fd[q]
