"""numpy restatement of the rules K1-K5 of mvr_cloud_iss_keypoints (include/mvr_hip.h): neighbourhoods from
normals_ref.radius_sets (the library's f32 rule), the f64 scatter about the query point, numpy.linalg.eigvalsh, the saliency
test and the non-maximum suppression.

Two correct implementations differ by the order of the sums and by the rounding of the eigen-solver, so what can be compared
exactly depends on the input; `margins` measures it:
  * ratio:  the smallest |e2 / e1 - gamma_21| and |e3 / e2 - gamma_32| over the points whose salience hangs on them;
  * pair:   the smallest relative difference of two different saliencies of neighbouring salient points (a pair of EQUAL bits
            is a tie both implementations keep -- K5 is strict -- and is counted apart);
  * e3:     the smallest e3 / e1 of a salient point (the relative rounding of e3 is that of e1, about 1e-16, over this).
A point is DECIDED when no rounding can change whether it is salient: see `decided`."""
import numpy as np

import normals_ref as NR
from outlier_ref import finite_mask

F64 = np.float64
GAP = 1e-9


def scatter(p, flat, offs):
    """K3: (S[n, 3, 3], count[n]) -- the sums of (p_j - p_i)(p_j - p_i)^T in f64 from the f32 coordinates, not divided"""
    p = np.asarray(p, np.float32)
    n = len(p)
    cnt = np.diff(offs)
    owner = np.repeat(np.arange(n), cnt)
    d = p[flat, :3].astype(F64) - p[owner, :3].astype(F64)
    S = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            S[:, a, b] = S[:, b, a] = np.bincount(owner, d[:, a] * d[:, b], minlength=n)
    return S, cnt.astype(np.int64)


def salience(S, cnt, gamma_21, gamma_32, min_neighbors):
    """K4: dict(e[n, 3] descending, r21, r32, salient, saliency)"""
    w = np.linalg.eigvalsh(S)[:, ::-1]
    e1, e2, e3 = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        r21, r32 = e2 / e1, e3 / e2
        sal = (cnt >= min_neighbors) & np.isfinite(w).all(1) & (e3 >= 0) & (r21 < gamma_21) & (r32 < gamma_32) & (e3 > 0)
    return dict(e=w, r21=r21, r32=r32, salient=sal, saliency=np.where(sal, e3, 0.0))


def nms(saliency, flat, offs, min_neighbors):
    """K5 from ANY saliency array (the reference's, or the GPU's own) and neighbour sets: (nms_count, keypoint flags)"""
    n = len(saliency)
    cnt = np.diff(offs)
    owner = np.repeat(np.arange(n), cnt)
    beaten = np.zeros(n, bool)
    if len(flat):
        np.logical_or.at(beaten, owner, saliency[owner] < saliency[flat])
    salient = saliency != 0
    return np.where(salient, cnt, 0).astype(np.uint32), salient & (cnt >= min_neighbors) & ~beaten


def iss(p, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, fma=False, sets=None):
    """the whole detector; `sets` = ((flat, offs) of the salient radius, (flat, offs) of the non-max radius) when already at hand"""
    p = np.asarray(p, np.float32)
    s_sets, n_sets = sets if sets is not None else (NR.radius_sets(p, salient_radius, fma), NR.radius_sets(p, non_max_radius, fma))
    S, cnt = scatter(p, *s_sets)
    out = salience(S, cnt, gamma_21, gamma_32, min_neighbors)
    out["valid"] = finite_mask(p)
    out["salient_count"] = cnt.astype(np.uint32)
    out["nms_count"], out["keypoint"] = nms(out["saliency"], n_sets[0], n_sets[1], min_neighbors)
    out["index"] = np.nonzero(out["keypoint"])[0].astype(np.uint32)
    out["sets"] = (s_sets, n_sets)
    out["params"] = (gamma_21, gamma_32, min_neighbors)
    return out


def decided(r, gap=GAP):
    """the points whose salience no rounding of a correct implementation changes: too few neighbours or none (K1, K3); an
    all-zero scatter (exact in any order of the sums: every term is +0); or well-conditioned eigenvalues -- e3 and e2 above
    gap * e1 in magnitude -- with both ratios more than gap from their thresholds"""
    g21, g32, mn = r["params"]
    e1, e2, e3 = r["e"][:, 0], r["e"][:, 1], r["e"][:, 2]
    few = r["salient_count"] < mn
    zero = (r["e"] == 0).all(1)
    with np.errstate(invalid="ignore"):
        well = (e1 > 0) & (np.abs(e3) > gap * e1) & (np.abs(e2) > gap * e1) & (np.abs(r["r21"] - g21) > gap) & (np.abs(r["r32"] - g32) > gap)
    return few | zero | well


def margins(r):
    """dict(ratio, pair, e3, ties): the distances described at the top, over the salient points (inf where there is none)"""
    g21, g32, mn = r["params"]
    live = (r["salient_count"] >= mn) & (r["e"][:, 0] > 0)
    with np.errstate(invalid="ignore"):
        d21 = np.abs(r["r21"] - g21)[live]
        d32 = np.abs(r["r32"] - g32)[live & (r["r21"] < g21)]
    sal = r["saliency"]
    flat, offs = r["sets"][1]
    owner = np.repeat(np.arange(len(sal)), np.diff(offs))
    both = (sal[owner] > 0) & (sal[flat] > 0) & (owner != flat)
    a, b = sal[owner][both], sal[flat][both]
    rel = np.abs(a - b) / np.maximum(a, b)
    s = r["salient"]
    return dict(ratio=float(min(d21.min(initial=np.inf), d32.min(initial=np.inf))),
                pair=float(rel[rel > 0].min(initial=np.inf)), ties=int((rel == 0).sum()),
                e3=float((r["e"][s, 2] / r["e"][s, 0]).min(initial=np.inf)))
