"""numpy reference of the sample-consensus rejector (rules C1-C12 at mvr_reject_sample_consensus in include/mvr_hip.h).

The host SVD's bits cannot be reproduced in numpy, so the library's answer is not compared with a second run of the whole
algorithm: `verify` REPLAYS it from its trace, as tests/test_gpu_align.py::verify does for the coarse aligner:
  (a) the sampled pairs of every attempt are C2's, exactly;
  (b) every counted attempt's count equals the f32 evaluation of C4 / C5 on the traced T's bits, exactly;
  (c) the traced T is within ROT_TOL / TRANS_TOL of f64 Kabsch on the three pairs, for attempts whose sample covariance has a
      second singular value >= WELL of the first (a flatter sample does not determine the rotation to that accuracy); in a frame
      far from the origin (far = True), where T's translation is of the order of the distance, the displacement
      max_i |T p_i - T_k p_i| against `cast_bar`, what casting an f64 rigid motion to f32 can do;
  (d) C7's loop replayed over the traced counts gives the traced k and the result's iterations, attempts, skipped, best_attempt;
  (e) the survivors are the C5 inliers of result.T's bits; with refine, when the refit of the survivors keeps them (the stop by
      set equality), result.T is within the bars of Kabsch over them;
  (f) found = 0 returns the list untouched.
`run` is the whole algorithm with numpy's Kabsch as its own estimator: what the host test runs on the planted cases; it records
every attempt and every refine round.  `transform_f32(contracted=True)` is C4 as a build with contraction would evaluate it (wrong
on purpose); `candidates`, `find_tie` and `find_between` pick thresholds that lie ON a d2 or between its plain and fma forms."""
import math

import numpy as np

from align_ref import kabsch
from sac_ref import DBL_EPSILON, K_MARGIN, sample_positions

F32, F64, U32 = np.float32, np.float64, np.uint32
ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_parity.py:17
WELL = 1e-3
PROBABILITY = 0.99
SKIPPED, COUNTED = 0, 1


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def sort_list(q, m, d):
    """C1: the list in ascending query index"""
    q, m, d = np.asarray(q, np.int32), np.asarray(m, np.int32), np.asarray(d, F32)
    o = np.argsort(q, kind="stable")
    return q[o], m[o], d[o]


def valid_mask(src, tgt, q, m):
    if len(q) == 0:
        return np.zeros(0, bool)
    return np.isfinite(src[q, :3]).all(1) & np.isfinite(tgt[m, :3]).all(1)


def _fma(a, b, c):
    """fmaf on f32 arrays: a product of two f32 is exact in the 64-bit mantissa of a long double, the sum is rounded there and then
    once more"""
    L = np.longdouble
    return (a.astype(L) * b.astype(L) + c.astype(L)).astype(F32)


def transform_f32(T, P, contracted=False):
    """C4 on the rows of P (float32 (n, 3)) with the 4 x 4 float32 T: every operation rounded to f32, in the rule's order.
    contracted = True is WRONG on purpose: what a build with floating-point contraction makes of the same expression,
    fmaf(T02, z, fmaf(T01, y, T00 x)) + T03; the host test shows that the far-frame cases tell the two apart."""
    T = np.asarray(T, F32)
    x, y, z = (np.ascontiguousarray(P[:, k], F32) for k in range(3))
    with np.errstate(all="ignore"):
        if contracted:
            out = [_fma(np.full_like(z, T[r, 2]), z, _fma(np.full_like(y, T[r, 1]), y, T[r, 0] * x)) + T[r, 3] for r in range(3)]
        else:
            out = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
    assert all(o.dtype == F32 for o in out)
    return out


def d2_f32(T, P, Q, fma=False, contracted=False):
    """C5: float32[n]"""
    x, y, z = transform_f32(T, P, contracted)
    with np.errstate(all="ignore"):
        dx, dy, dz = x - Q[:, 0].astype(F32), y - Q[:, 1].astype(F32), z - Q[:, 2].astype(F32)
        if fma:      # a product of two f32 is exact in the 64-bit mantissa of a long double, the sum is rounded there and then once more
            L = np.longdouble
            t = dx * dx
            t = (dy.astype(L) * dy.astype(L) + t.astype(L)).astype(F32)
            t = (dz.astype(L) * dz.astype(L) + t.astype(L)).astype(F32)
        else:
            t = (dx * dx + dy * dy) + dz * dz
    assert t.dtype == F32
    return t


def inlier_mask(T, P, Q, value, fma=False, contracted=False):
    with np.errstate(all="ignore"):
        return d2_f32(T, P, Q, fma, contracted).astype(F64) < float(value) * float(value)


def kabsch_f32(p, q):
    """the reference's own estimator: f64 Kabsch, cast to f32 (None when not finite); and the singular values"""
    with np.errstate(all="ignore"):
        try:
            T, S = kabsch(p, q)
        except np.linalg.LinAlgError:
            return None, np.zeros(3)
    T32 = T.astype(F32)
    return (T32 if np.isfinite(T32).all() else None), S


def well_conditioned(S):
    return S[0] > 0 and S[1] >= WELL * S[0]


def replay_loop(status, counts, nv, max_iterations):
    """C7 over the attempts' statuses and counts: dict(k[t], iterations, attempts, skipped, best, best_count, min_margin); the
    attempts given must be exactly the ones the loop consumes"""
    log_p = math.log(1.0 - PROBABILITY)
    iterations = skipped = t = 0
    k, best_count, best, margin, ks = 1.0, -1, -1, math.inf, []
    while True:
        margin = min(margin, abs(iterations - k))
        if not (iterations < k and skipped < 10 * max_iterations):
            break
        assert t < len(status), "the loop wants attempt %d and the trace has %d" % (t, len(status))
        stop = False
        if status[t] == SKIPPED:
            skipped += 1
        else:
            if int(counts[t]) > best_count:
                best_count, best = int(counts[t]), t
                w = best_count / float(nv)
                pno = min(max(1.0 - w * w * w, DBL_EPSILON), 1.0 - DBL_EPSILON)
                k = log_p / math.log(pno)
            iterations += 1
            stop = iterations > max_iterations      # PCL's own off-by-one
        ks.append(k)
        t += 1
        if stop:
            break
    assert t == len(status), "the trace has %d attempts, the loop consumes %d" % (len(status), t)
    return dict(k=np.array(ks, F64), iterations=iterations, attempts=t, skipped=skipped, best=best, best_count=best_count, min_margin=margin)


def run(src, tgt, q, m, d, value, max_iterations=0, refine=False, seed=0, fma=False, check_margin=True):
    """the whole stage with numpy's Kabsch as the estimator -> dict(found, q, m, d (the survivors), T, ransac_T, inliers,
    ransac_inliers, iterations, attempts, skipped, best_attempt, refine_rounds, k, live, valid, well (share of the counted
    attempts that qualify for check (c)), min_margin) and, what the tests of the hardening cases read: status[t], counts[t], Ts[t]
    of every attempt consumed, rounds = [(T_r, I_r as a mask over the valid pairs)] for r = 0 .. refine_rounds, r = 0 being the
    RANSAC answer (a round that stops with the round before repeats it)"""
    max_it = int(max_iterations) or 1000
    q, m, d = sort_list(q, m, d)
    val = valid_mask(src, tgt, q, m)
    vi = np.nonzero(val)[0]
    nv = len(vi)
    P, Q = src[q[vi], :3], tgt[m[vi], :3]
    out = dict(found=False, q=q, m=m, d=d, T=np.eye(4, dtype=F32), ransac_T=np.eye(4, dtype=F32), inliers=len(q), ransac_inliers=0,
               iterations=0, attempts=0, skipped=0, best_attempt=-1, refine_rounds=0, k=1.0, live=len(q), valid=nv, well=1.0, min_margin=math.inf,
               status=[], counts=[], Ts=[], rounds=[])
    if nv < 3:
        return out
    log_p = math.log(1.0 - PROBABILITY)
    iterations = skipped = t = n_well = 0
    k, best_count, best_T, best, margin = 1.0, -1, None, -1, math.inf
    while True:
        margin = min(margin, abs(iterations - k))
        if not (iterations < k and skipped < 10 * max_it):
            break
        s = sample_positions(seed, t, nv)
        T, S = kabsch_f32(P[s].astype(F64), Q[s].astype(F64))
        stop = False
        out["status"].append(SKIPPED if T is None else COUNTED)
        out["Ts"].append(T)
        out["counts"].append(0)
        if T is None:
            skipped += 1
        else:
            n_well += bool(well_conditioned(S))
            count = out["counts"][-1] = int(inlier_mask(T, P, Q, value, fma).sum())
            if count > best_count:
                best_count, best, best_T = count, t, T
                w = best_count / float(nv)
                pno = min(max(1.0 - w * w * w, DBL_EPSILON), 1.0 - DBL_EPSILON)
                k = log_p / math.log(pno)
            iterations += 1
            stop = iterations > max_it
        t += 1
        if stop:
            break
    if check_margin:
        assert margin >= K_MARGIN, "a stop decision within %g of k" % margin
    out.update(iterations=iterations, attempts=t, skipped=skipped, k=k, well=n_well / max(iterations, 1), min_margin=margin)
    if best_count < 3:
        return out
    mask = inlier_mask(best_T, P, Q, value, fma)
    T_fin, rounds = best_T, 0
    out["rounds"].append((best_T, mask))
    if refine:      # C10
        while True:
            rounds += 1
            Tr, _ = kabsch_f32(P[mask].astype(F64), Q[mask].astype(F64))
            nxt = inlier_mask(Tr, P, Q, value, fma) if Tr is not None else None
            if Tr is None or nxt.sum() < 3:
                out["rounds"].append((T_fin, mask))
                break
            same = np.array_equal(nxt, mask)
            T_fin, mask = Tr, nxt
            out["rounds"].append((T_fin, mask))
            if same or rounds >= max_it:
                break
    keep = vi[mask]
    out.update(found=True, q=q[keep], m=m[keep], d=d[keep], T=T_fin, ransac_T=best_T, inliers=int(mask.sum()), ransac_inliers=best_count,
               best_attempt=best, refine_rounds=rounds)
    return out


def close_to(T, Tk):
    """T (float32 4 x 4) within the project's bars of Tk (f64)"""
    dr, dt = np.abs(T[:3, :3].astype(F64) - Tk[:3, :3]).max(), np.abs(T[:3, 3].astype(F64) - Tk[:3, 3]).max()
    return dr <= ROT_TOL and dt <= TRANS_TOL, dr, dt


def cast_bar(T, P):
    """what casting an f64 rigid motion T to f32 can move a point of P (rows of three) by: every rotation entry is off by at
    most 2^-24 of an entry <= 1, every translation entry by half an ulp of the largest; twice that"""
    big_p = float(np.abs(np.asarray(P, F64)).max())
    big_t = F32(np.abs(np.asarray(T, F64)[:3, 3]).max())
    return 2.0 * (3.0 * 2.0 ** -24 * big_p + float(np.spacing(big_t)) / 2.0)


def displacement(T, Tk, P):
    """max_i |T p_i - Tk p_i| (the largest coordinate) over the rows of P, in f64"""
    P, T, Tk = np.asarray(P, F64), np.asarray(T, F64), np.asarray(Tk, F64)
    return float(np.abs((P @ T[:3, :3].T + T[:3, 3]) - (P @ Tk[:3, :3].T + Tk[:3, 3])).max())


def verify(src, tgt, q, m, d, value, max_iterations, refine, seed, got, fma=False, check_c=False, far=False, check_refit=True):
    """checks (a)-(f) on got = (query, match, d2, result, trace) of Context.reject_sample_consensus; returns a dict of figures:
    counted, well (the share of counted attempts that qualify for (c)), worst_rot, worst_trans, refit_checked, worst_disp, bar.
    far = True: check (c) in a frame far from the origin, where T's translation is of the order of the distance and the entrywise
    bars say nothing: the displacement max_i |T p_i - T_k p_i| over the valid pairs' source points against cast_bar.
    check_refit = False leaves out the comparison of the refined T with Kabsch (the one part of (e) that needs a reference)."""
    gq, gm, gd, res, tr = got
    max_it = int(max_iterations) or 1000
    q, m, d = sort_list(q, m, d)
    val = valid_mask(src, tgt, q, m)
    vi = np.nonzero(val)[0]
    nv = len(vi)
    P, Q = src[q[vi], :3], tgt[m[vi], :3]
    assert (res["live"], res["valid"]) == (len(q), nv), (res["live"], res["valid"], len(q), nv)
    fig = dict(counted=0, well=1.0, worst_rot=0.0, worst_trans=0.0, refit_checked=False, worst_disp=0.0, bar=0.0)
    n_att = len(tr["status"])
    assert n_att == res["attempts"]
    if nv < 3:
        assert n_att == 0 and not res["found"] and res["k"] == 1.0
    n_well = 0
    for t in range(n_att):
        s = sample_positions(seed, t, nv)
        # (a)
        assert np.array_equal(tr["query"][t], q[vi[s]]) and np.array_equal(tr["match"][t], m[vi[s]]), ("samples", t)
        T = tr["T"][t].reshape(4, 4).T
        Tk, S = kabsch(P[s].astype(F64), Q[s].astype(F64))
        if tr["status"][t] == SKIPPED:
            assert not np.isfinite(Tk.astype(F32)).all(), ("an attempt was skipped whose Kabsch is finite", t)
            assert not T.any() and tr["inliers"][t] == 0, ("a skipped attempt's record", t)
            continue
        assert tr["status"][t] == COUNTED and np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1]), ("T", t)
        fig["counted"] += 1
        # (b)
        count = int(inlier_mask(T, P, Q, value, fma).sum())
        assert count == tr["inliers"][t], ("count", t, count, int(tr["inliers"][t]))
        # (c)
        if well_conditioned(S):
            n_well += 1
            ok, dr, dt = close_to(T, Tk)
            fig["worst_rot"], fig["worst_trans"] = max(fig["worst_rot"], dr), max(fig["worst_trans"], dt)
            if far:
                disp, bar = displacement(T, Tk, P), cast_bar(Tk, P)
                if disp / bar >= fig["worst_disp"] / max(fig["bar"], 1e-300):
                    fig["worst_disp"], fig["bar"] = disp, bar
                if check_c:
                    assert disp <= bar, ("T against Kabsch, as a displacement", t, disp, bar)
            elif check_c:
                assert ok, ("T against Kabsch", t, dr, dt)
    fig["well"] = n_well / max(fig["counted"], 1)
    # (d)
    if nv >= 3:
        lp = replay_loop(tr["status"], tr["inliers"], nv, max_it)
        assert np.allclose(tr["k"], lp["k"], rtol=1e-12, atol=0) and abs(res["k"] - lp["k"][-1]) <= 1e-12 * abs(lp["k"][-1])
        assert (res["iterations"], res["attempts"], res["skipped"]) == (lp["iterations"], lp["attempts"], lp["skipped"])
        found = lp["best_count"] >= 3
        assert res["found"] == found and res["best_attempt"] == (lp["best"] if found else -1)
    else:
        found = False
    if not found:
        # (f)
        assert np.array_equal(gq, q) and np.array_equal(gm, m) and np.array_equal(bits(gd), bits(d)), "found = 0 keeps the list"
        assert res["inliers"] == len(q) and np.array_equal(res["T"], np.eye(4, dtype=F32)) and res["refine_rounds"] == 0
        return fig
    # (e)
    T0 = tr["T"][lp["best"]].reshape(4, 4).T
    assert np.array_equal(bits(res["ransac_T"]), bits(T0)) and res["ransac_inliers"] == lp["best_count"]
    if not refine:
        assert np.array_equal(bits(res["T"]), bits(T0)) and res["refine_rounds"] == 0
    mask = inlier_mask(res["T"], P, Q, value, fma)
    keep = vi[mask]
    assert res["inliers"] == len(keep) >= 3
    assert np.array_equal(gq, q[keep]) and np.array_equal(gm, m[keep]) and np.array_equal(bits(gd), bits(d[keep])), "the survivors"
    if refine:
        assert 1 <= res["refine_rounds"] <= max_it
        Tk, _ = kabsch(P[mask].astype(F64), Q[mask].astype(F64))
        if check_refit and res["refine_rounds"] < max_it and np.array_equal(inlier_mask(Tk.astype(F32), P, Q, value, fma), mask):
            ok, dr, dt = close_to(res["T"], Tk)
            assert ok, ("the refined T against Kabsch over the final inliers", dr, dt)
            fig["refit_checked"] = True
    return fig


# ------------------------------------------------------------------ thresholds put on a d2 on purpose

def candidates(d2, lo=0.97, hi=0.995):
    """the pairs a threshold can be put on while the loop still consumes exactly two attempts: those with a share in [lo, hi] of
    the pairs strictly below them (w in that range keeps k between 1.01 and 1.89), in ascending d2"""
    d2 = np.asarray(d2, F32)
    below = np.searchsorted(np.sort(d2), d2, side="left") / float(len(d2))
    idx = np.nonzero((below >= lo) & (below <= hi) & np.isfinite(d2))[0]
    return idx[np.argsort(d2[idx], kind="stable")]


def find_tie(d2, among):
    """-> (i, value): the first pair i of `among` for which a double `value` exists with value * value == (double)d2[i] exactly,
    tried at sqrt(d2[i]) and its neighbours.  At that threshold C5's strict comparison leaves pair i out; at
    nextafter(value, inf) it counts it."""
    for i in among:
        x = float(d2[i])
        v = math.sqrt(x)
        near = [v, np.nextafter(v, 0.0), np.nextafter(v, math.inf)]
        near += [np.nextafter(near[1], 0.0), np.nextafter(near[2], math.inf)]
        for c in near:
            c = float(c)
            up = float(np.nextafter(c, math.inf))
            if c * c == x and up * up > x:
                return int(i), c
    return None


def find_between(d2_plain, d2_fma, among):
    """-> (i, value): the first pair i of `among` whose plain and fma d2 differ in bits, and a threshold between them:
    lo < value * value <= hi, so that the arithmetic with the lower d2 counts pair i and the other does not"""
    a, b = np.asarray(d2_plain, F32), np.asarray(d2_fma, F32)
    for i in among:
        if bits(a[i:i + 1])[0] == bits(b[i:i + 1])[0]:
            continue
        lo, hi = sorted((float(a[i]), float(b[i])))
        value = math.sqrt((lo + hi) / 2.0)
        if lo < value * value <= hi:
            return int(i), value
    return None
