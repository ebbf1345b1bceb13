"""numpy restatement of the rules B1-B5 of mvr_cloud_boundary and K9-K11 of mvr_cloud_iss_keypoints_border (include/mvr_hip.h):
neighbourhoods from normals_ref.radius_sets (the library's f32 rule), the tangent basis of B2 in f32 as the rule states it,
the f32 differences of B3, then f64 projections, numpy's arctan2 and a real sort.

Two correct implementations differ by the rounding of the projections and of the arctangent, so a flag can be compared only
where the largest gap is not at the threshold.  A point is DECIDED iff
    |max_dif - threshold| > 2 * max_j 1e-6 * (1 + |d_j| / |d_j in the tangent plane|)
over its neighbours j with an angle.  What the slack covers: an f32 dot product of three terms is within 3 * 2^-24 * |d| of
the exact one (|u|, |v| <= 1 for a unit normal), which turns the angle by at most that over the length of d in the tangent
plane -- 1.8e-7 * |d| / |d_t| -- on each of the two projections; atan2f is within 2 ulp of pi, 4.8e-7; the f32 subtraction
of two angles another 2.4e-7.  1e-6 * (1 + |d| / |d_t|) is above their sum per angle, a gap has two angles, hence the 2: a
factor of at least 2 is left over.  A neighbour straight above the point (|d_t| = 0) has no defined angle and leaves its point
undecided.

The border flags (K10) and the detector with a border (K11) are computable from ANY edge / border array, the reference's or
the GPU's own, as iss_ref.nms is from any saliency."""
import numpy as np

import iss_ref as IR
import normals_ref as NR
from outlier_ref import finite_mask

F32, F64 = np.float32, np.float64
SECTORS = 16
SECTOR_WIDTH = 2.0 * np.pi / SECTORS
MIN_ANGLE = np.pi / 4              # MVR_BOUNDARY_MIN_ANGLE
FLT_MIN = float(np.finfo(F32).tiny)


def basis(nrm):
    """B2 in f32, operation by operation: (u[n, 3], v[n, 3], ok[n]); ok is False under the rule's deviation"""
    n = np.ascontiguousarray(np.asarray(nrm, F32)[:, :3])
    m = len(n)
    with np.errstate(all="ignore"):
        a = np.abs(n)
        a = np.where(np.isnan(a), F32(-1), a)                      # (such a normal fails `ok` anyway)
        maxi = np.argmax(a, axis=1)                                # the FIRST index of the largest
        sndi = np.where(maxi == 0, 1, 0)
        r = np.arange(m)
        ns, nm = n[r, sndi], n[r, maxi]
        inv = F32(1.0) / np.sqrt(ns * ns + nm * nm, dtype=F32)
        v = np.zeros((m, 3), F32)
        v[r, maxi] = -ns * inv
        v[r, sndi] = nm * inv
        u = np.stack([n[:, 1] * v[:, 2] - n[:, 2] * v[:, 1], n[:, 2] * v[:, 0] - n[:, 0] * v[:, 2], n[:, 0] * v[:, 1] - n[:, 1] * v[:, 0]], 1)
    assert u.dtype == F32 and v.dtype == F32
    ok = np.isfinite(n).all(1) & np.isfinite(u).all(1) & np.isfinite(v).all(1)
    return u, v, ok


def boundary(p, nrm, radius, angle_threshold=np.pi / 2, min_neighbors=0, fma=False, sets=None):
    """B1-B5: dict(boundary, max_dif (f64), neighbor_count, slack, decided, valid, sets)"""
    p = np.asarray(p, F32)
    n = len(p)
    flat, offs = sets if sets is not None else NR.radius_sets(p, radius, fma)
    cnt = np.diff(offs).astype(np.int64)
    u, v, ok = basis(nrm) if n else (np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, bool))
    owner = np.repeat(np.arange(n), cnt)
    with np.errstate(all="ignore"):
        d = p[flat, :3] - p[owner, :3]                             # f32, as B3
    assert d.dtype == F32
    take = (d != 0).any(1) & ok[owner]
    o, d64 = owner[take], d[take].astype(F64)
    x, y = (u[o].astype(F64) * d64).sum(1), (v[o].astype(F64) * d64).sum(1)
    ang = np.arctan2(y, x)
    with np.errstate(divide="ignore", invalid="ignore"):
        sl = 1e-6 * (1.0 + np.linalg.norm(d64, axis=1) / np.hypot(x, y))
    slack = np.zeros(n)
    np.maximum.at(slack, o, sl)
    slack *= 2.0
    # the sorted angles of every owner, their consecutive differences and the wrap-around
    order = np.lexsort((ang, o))
    o, ang = o[order], ang[order]
    max_dif = np.full(n, FLT_MIN)
    if len(o):
        same = o[1:] == o[:-1]
        np.maximum.at(max_dif, o[1:][same], (ang[1:] - ang[:-1])[same])
        first = np.r_[True, ~same]
        last = np.r_[~same, True]
        np.maximum.at(max_dif, o[first], (2.0 * float(F32(np.pi)) - ang[last]) + ang[first])
    taken = np.bincount(o, minlength=n) > 0
    thr = float(F32(angle_threshold))
    valid = finite_mask(p) if n else np.zeros(0, bool)
    flag = valid & (cnt >= 3) & (cnt >= min_neighbors) & taken & (max_dif > thr)
    # decided: the count tests and `taken` are exact; the gap test where the gap is outside the slack of the threshold
    decided = ~(valid & (cnt >= 3) & (cnt >= min_neighbors) & taken) | (np.abs(max_dif - thr) > slack)
    return dict(boundary=flag, max_dif=np.where(taken, max_dif, 0.0), neighbor_count=cnt.astype(np.uint32), slack=slack, decided=decided,
                valid=valid, taken=taken, sets=(flat, offs))


def border_from_edges(edge, flat, offs, valid):
    """K10 from ANY edge array over the neighbour sets of the border radius"""
    n = len(edge)
    owner = np.repeat(np.arange(n), np.diff(offs))
    out = np.zeros(n, bool)
    if len(flat):
        np.logical_or.at(out, owner, np.asarray(edge, bool)[flat])
    return out & valid


def iss_with_border(ref, border):
    """K11 on a result of iss_ref.iss (left unchanged) from ANY border mask: a copy in which a border point has saliency 0 and
    both counts 0 and is never salient, with the suppression recomputed over the same neighbour sets"""
    border = np.asarray(border, bool)
    out = dict(ref)
    out["saliency"] = np.where(border, 0.0, ref["saliency"])
    out["salient"] = ref["salient"] & ~border
    out["salient_count"] = np.where(border, 0, ref["salient_count"]).astype(np.uint32)
    mn = ref["params"][2]
    out["nms_count"], out["keypoint"] = IR.nms(out["saliency"], ref["sets"][1][0], ref["sets"][1][1], mn)
    out["index"] = np.nonzero(out["keypoint"])[0].astype(np.uint32)
    out["border"] = border
    return out


def decided_with_border(ref, border):
    """iss_ref.decided of a point that is no border point; a border point is decided (its zeros are exact)"""
    return IR.decided(ref) | np.asarray(border, bool)
