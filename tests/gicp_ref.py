"""numpy restatement of the Generalized-ICP rules G3-G8 of include/mvr_hip.h (mvr_icp_align_gicp); independent of the library.
Points and normals are (n, 3) float64 arrays already gathered by the correspondence list: p, s = the source's, q, n = the
target's.  X is a (4, 4) float64 matrix.  The plain-loop versions at the end are what tests/test_gicp_host.py holds the
vectorised ones against."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
OK, E_NOCORR, E_SINGULAR = 0, -3, -5
DEFAULTS = dict(max_corr_dist=5.0, use_reciprocal=0, fma_dist=0, max_iterations=200, max_inner_iterations=20, transformation_epsilon=5e-4,
                rotation_epsilon=2e-3, gicp_epsilon=1e-3, inner_rot_tol=1e-6, inner_trans_tol=1e-5, inner_chunk=4)


def params(**kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def xyz(a):
    return np.asarray(a)[:, :3].astype(F64)


def side(nrm, eps):
    """G3: I - (1 - eps) n^ n^T per row; I where the normal is not finite or has no length"""
    nrm = np.asarray(nrm, F64)
    with np.errstate(invalid="ignore", over="ignore"):
        l2 = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        ok = np.isfinite(nrm).all(1) & (l2 > 0.0)
    u = np.zeros_like(nrm)
    u[ok] = nrm[ok] / np.sqrt(l2[ok])[:, None]
    return np.eye(3)[None] - (1.0 - eps) * u[:, :, None] * u[:, None, :]


def weights(s, n, eps):
    """G4: W = (A + B)^-1"""
    return np.linalg.inv(side(s, eps) + side(n, eps))


def jacobians(y):
    """G5: J = [-[y]x | I], (m, 3, 6)"""
    m = len(y)
    J = np.zeros((m, 3, 6))
    J[:, 0, 1], J[:, 0, 2] = y[:, 2], -y[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -y[:, 2], y[:, 0]
    J[:, 2, 0], J[:, 2, 1] = y[:, 1], -y[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    return J


IU = np.triu_indices(6)


def terms(p, s, q, n, X, eps):
    """(m, 29): what each correspondence adds to the 29 sums of G5"""
    X = np.asarray(X, F64)
    W = weights(s, n, eps)
    y = p @ X[:3, :3].T + X[:3, 3]
    r = y - q
    J = jacobians(y)
    WJ = np.einsum("mab,mbc->mac", W, J)
    H = np.einsum("mba,mbc->mac", J, WJ)
    Wr = np.einsum("mab,mb->ma", W, r)
    out = np.empty((len(p), 29))
    out[:, :21] = H[:, IU[0], IU[1]]
    out[:, 21:27] = np.einsum("mba,mb->ma", J, Wr)
    out[:, 27] = 1.0
    out[:, 28] = np.einsum("ma,ma->m", r, Wr)
    return out


def fsum_columns(t):
    """the exactly rounded sum of every column; a column that holds a NaN or infinities of both signs sums to NaN"""
    def one(col):
        try:
            return math.fsum(col)
        except (ValueError, OverflowError):
            return float("nan")
    return np.array([one(t[:, k]) for k in range(t.shape[1])]) if len(t) else np.zeros(t.shape[1])


def terms_ld(p, s, q, n, X, eps):
    """terms() once more with np.longdouble throughout and the closed-form inverse of G4 (cofactors over the determinant):
    the reference of the sums over the range of gicp_epsilon, where np.linalg.inv in f64 is no better than the kernel"""
    LD = np.longdouble
    assert np.finfo(LD).eps < 2e-19
    p, s, q, n, X = (np.asarray(a, F64).astype(LD) for a in (p, s, q, n, X))
    eps, one = LD(eps), LD(1)
    k = one - eps

    def unit(v):
        with np.errstate(invalid="ignore", over="ignore"):
            l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            ok = np.isfinite(v).all(1) & (l2 > 0)
        u = np.zeros_like(v)
        u[ok] = v[ok] / np.sqrt(l2[ok])[:, None]
        return u
    us, un = unit(s), unit(n)
    M = {}
    for a in range(3):
        for b in range(a, 3):
            M[a, b] = (LD(2) if a == b else LD(0)) - k * (us[:, a] * us[:, b]) - k * (un[:, a] * un[:, b])
    a, b, c, d, e, f = M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = (a * c00 + b * c01) + c * c02
    W = np.empty((len(p), 3, 3), LD)
    W[:, 0, 0], W[:, 0, 1], W[:, 0, 2] = c00 / det, c01 / det, c02 / det
    W[:, 1, 1], W[:, 1, 2], W[:, 2, 2] = c11 / det, c12 / det, c22 / det
    W[:, 1, 0], W[:, 2, 0], W[:, 2, 1] = W[:, 0, 1], W[:, 0, 2], W[:, 1, 2]
    y = np.stack([(X[r, 0] * p[:, 0] + X[r, 1] * p[:, 1]) + X[r, 2] * p[:, 2] + X[r, 3] for r in range(3)], axis=1)
    r = y - q
    J = np.zeros((len(p), 3, 6), LD)
    J[:, 0, 1], J[:, 0, 2] = y[:, 2], -y[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -y[:, 2], y[:, 0]
    J[:, 2, 0], J[:, 2, 1] = y[:, 1], -y[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = one
    WJ = (W[:, :, :, None] * J[:, None, :, :]).sum(2)                      # (m, 3, 6)
    Wr = (W * r[:, None, :]).sum(2)
    out = np.empty((len(p), 29), LD)
    t = 0
    for i in range(6):
        for j in range(i, 6):
            out[:, t] = (J[:, :, i] * WJ[:, :, j]).sum(1)
            t += 1
    for i in range(6):
        out[:, 21 + i] = (J[:, :, i] * Wr).sum(1)
    out[:, 27] = one
    out[:, 28] = (r * Wr).sum(1)
    assert out.dtype == LD
    return out


def sums_ld(p, s, q, n, X, eps):
    """(the exactly rounded column sums of terms_ld cast to f64, those of their absolute values)"""
    t = terms_ld(p, s, q, n, X, eps).astype(F64)
    return fsum_columns(t), fsum_columns(np.abs(t))


def sums(p, s, q, n, X, eps, with_abs=False):
    """the 29 sums (exactly rounded sums of the terms), and with_abs: the sums of the terms' absolute values"""
    t = terms(p, s, q, n, X, eps)
    return (fsum_columns(t), fsum_columns(np.abs(t))) if with_abs else fsum_columns(t)


def unpack(sm):
    H = np.zeros((6, 6))
    H[IU] = sm[:21]
    H = H + np.triu(H, 1).T
    return H, sm[21:27].copy()


def cholesky_solve(H, g, lam):
    """G6: (H + lam diag(H)) delta = -g; None for a pivot that is <= 0 or not finite"""
    A = H + lam * np.diag(np.diag(H))
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j] - float(L[j, :j] @ L[j, :j])
        if not (d > 0.0) or not math.isfinite(d):
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    z = np.zeros(6)
    for i in range(6):
        z[i] = (-g[i] - float(L[i, :i] @ z[:i])) / L[i, i]
    delta = np.zeros(6)
    for i in range(5, -1, -1):
        delta[i] = (z[i] - float(L[i + 1:, i] @ delta[i + 1:])) / L[i, i]
    return delta


def rodrigues(w):
    th = math.sqrt(float(w @ w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def candidate(X, delta):
    E = rodrigues(delta[:3])
    Xc = np.eye(4)
    Xc[:3, :3] = E @ X[:3, :3]
    Xc[:3, 3] = E @ X[:3, 3] + delta[3:]
    return Xc


def decided(f, fc, tot, totc):
    """whether the comparison f_c < f of G7 is beyond what the sums are held to: every term at both poses is exactly 0 (then
    f_c == f == 0 on any machine), or the two differ by more than 1e-9 of the terms' absolute values, ten times the bound
    each side's sum 28 is held to"""
    if tot == 0.0 and totc == 0.0:
        return True
    return bool(abs(fc - f) > 1e-9 * (tot + totc))


def solve(p, s, q, n, prm, log=None):
    """G7 -> (X, info dict(evaluations, accepted, lambda, f0, f1), status).  log (a list) gets one dict per evaluation after
    the first: decision "A" / "R", lam = lambda before it, f and fc = sum 28 at X and at the candidate, tot and totc = the sums
    of the absolute values of its terms there, w and v = |omega| and |v| of the step, decided, and the state after the
    decision: X, lam_after, accepted, f1.  Entry e - 2 is evaluation e; the state after evaluation 1 is (I, 1e-3, 0)."""
    eps = prm["gicp_epsilon"]
    X, lam = np.eye(4), 1e-3
    info = dict(evaluations=0, accepted=0, f0=0.0, f1=0.0)
    info["lambda"] = lam
    if len(p) < 3:
        return X, info, E_NOCORR
    sm, tot = sums(p, s, q, n, X, eps, with_abs=True)
    ev, status = 1, OK
    info["f0"] = info["f1"] = sm[28] / sm[27]
    if not math.isfinite(info["f0"]):                                      # G7: a listed point or weight that is not finite
        info["evaluations"] = 1
        return X, info, E_SINGULAR
    while ev < prm["max_inner_iterations"]:
        H, g = unpack(sm)
        delta = cholesky_solve(H, g, lam)
        if delta is None:
            status = E_SINGULAR
            break
        Xc = candidate(X, delta)
        sc, totc = sums(p, s, q, n, Xc, eps, with_abs=True)
        ev += 1
        w, v = math.sqrt(float(delta[:3] @ delta[:3])), math.sqrt(float(delta[3:] @ delta[3:]))
        entry = dict(lam=lam, f=float(sm[28]), fc=float(sc[28]), tot=float(tot[28]), totc=float(totc[28]), w=w, v=v,
                     decided=decided(float(sm[28]), float(sc[28]), float(tot[28]), float(totc[28])))
        end = False
        if sc[28] < sm[28]:
            X, sm, tot, lam = Xc, sc, totc, max(lam / 10.0, 1e-9)
            info["accepted"] += 1
            info["f1"] = sm[28] / sm[27]
            entry["decision"] = "A"
            end = w < prm["inner_rot_tol"] and v < prm["inner_trans_tol"]
        else:
            lam = 10.0 * lam
            entry["decision"] = "R"
            end = lam > 1e9
        if log is not None:
            entry.update(X=X.copy(), lam_after=lam, accepted=info["accepted"], f1=info["f1"])
            log.append(entry)
        if end:
            break
    info["evaluations"], info["lambda"] = ev, lam
    return X, info, status


def pattern(log):
    return "".join(e["decision"] for e in log)


def lambda_of(decisions):
    """G7's lambda after a string of decisions: 1e-3 * 10^(rejects - accepts), clipped below at 1e-9 where an accept meets it,
    by the very operations of G7"""
    lam = 1e-3
    for d in decisions:
        lam = max(lam / 10.0, 1e-9) if d == "A" else 10.0 * lam
    return lam


def undecided(log):
    """the evaluation numbers (2, 3, ...) whose decision is not decided"""
    return [k + 2 for k, e in enumerate(log) if not e["decided"]]


def objective(p, s, q, n, X, eps):
    return float(sums(p, s, q, n, X, eps)[28]) / len(p)


def outer_delta(new, old, prm):
    """G8: from the f32 entries, in f64"""
    d = np.abs(np.asarray(new, F32).astype(F64) - np.asarray(old, F32).astype(F64))
    return max(float(d[:3, :3].max()) / prm["rotation_epsilon"], float(d[:3, 3].max()) / prm["transformation_epsilon"])


def move_f32(pts, nrm, tr):
    """the current source under an incremental f32 transformation (R9), close to what the device's kernels make of it"""
    R, t = np.asarray(tr, F32)[:3, :3], np.asarray(tr, F32)[:3, 3]
    return (pts.astype(F32) @ R.T + t).astype(F32), (nrm.astype(F32) @ R.T).astype(F32)


def align(src, snrm, tgt, tnrm, prm, search, chain_fn=None):
    """G2, G8 with the caller's search(cur_pts (n,3) f32) -> (query, match, d2 f32) and chain_fn(q, m, d2, cur_nrm) -> the same.
    -> (fin f32 (4,4), dict(iterations, state, converged, n_corr, mse), trace)"""
    cur, cn = np.asarray(src, F32)[:, :3].copy(), np.asarray(snrm, F32)[:, :3].copy()
    T, N = xyz(tgt), xyz(tnrm)
    fin = np.eye(4, dtype=F32)
    st = dict(iterations=0, state="NOT", converged=False, n_corr=0, mse=0.0, rc=OK)
    trace = []
    while not st["converged"]:
        qi, mi, d2 = search(cur)
        n_found = len(qi)
        if chain_fn is not None:
            qi, mi, d2 = chain_fn(qi, mi, d2, cn)
        st["n_corr"] = len(qi)
        if len(qi) < 3:
            st["state"], st["rc"] = "NO_CORRESPONDENCES", E_NOCORR
            break
        X, info, status = solve(cur[qi].astype(F64), cn[qi].astype(F64), T[mi], N[mi], prm)
        st["mse"] = float(d2.astype(F64).sum()) / len(d2)
        if status != OK:
            st["state"], st["rc"] = "NO_CORRESPONDENCES", status
            break
        tr = X.astype(F32)
        new = (tr @ fin).astype(F32)
        delta = outer_delta(new, fin, prm)
        fin = new
        cur, cn = move_f32(cur, cn, tr)
        st["iterations"] += 1
        trace.append(dict(n_found=n_found, n_corr=len(qi), mse=st["mse"], tr=tr, info=info, delta=delta))
        if delta < 1.0:
            st["state"], st["converged"] = "TRANSFORM", True
        elif st["iterations"] >= prm["max_iterations"]:
            st["state"], st["converged"] = "ITERATIONS", True
    return fin, st, trace


# ---- helpers of the conditions: normals, searches, the SVD ICP the accuracy is held against

def knn_normals(pts, k=20):
    """PCL's k-neighbourhood normal in f64: the eigenvector of the smallest eigenvalue of the covariance of the k nearest points"""
    from scipy.spatial import cKDTree
    P = xyz(pts)
    _, idx = cKDTree(P).query(P, k=k)
    nb = P[idx] - P[:, None, :]
    c = nb - nb.mean(1, keepdims=True)
    cov = np.einsum("nka,nkb->nab", c, c) / k
    _, v = np.linalg.eigh(cov)
    out = np.zeros((len(P), 4), F32)
    out[:, :3] = v[:, :, 0].astype(F32)
    return out


def tree_search(tgt, max_dist, reciprocal):
    from scipy.spatial import cKDTree
    T = np.asarray(tgt, F32)[:, :3]
    tree = cKDTree(T.astype(F64))

    def search(cur):
        d, j = tree.query(cur.astype(F64))
        ok = d <= max_dist
        if reciprocal:
            _, back = cKDTree(cur.astype(F64)).query(T.astype(F64))
            ok &= back[j] == np.arange(len(cur))
        q = np.nonzero(ok)[0]
        diff = cur[q] - T[j[q]]
        return q.astype(np.int32), j[q].astype(np.int32), ((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]).astype(F32)
    return search


def kabsch(p, q):
    mp, mq = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((q - mq).T @ (p - mp))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def svd_icp(src, tgt, max_dist, iterations=50):
    """reciprocal point-to-point ICP in f64 with no stopping rule but the iteration count -> T (4,4)"""
    search = tree_search(tgt, max_dist, True)
    P, T = xyz(src), xyz(tgt)
    fin = np.eye(4)
    for _ in range(iterations):
        cur = P @ fin[:3, :3].T + fin[:3, 3]
        q, m, _ = search(cur.astype(F32))
        fin = kabsch(cur[q], T[m]) @ fin
    return fin


def rms_to(T, T_true, src):
    P = xyz(src)
    d = (P @ np.asarray(T, F64)[:3, :3].T + np.asarray(T, F64)[:3, 3]) - (P @ T_true[:3, :3].T + T_true[:3, 3])
    return float(np.sqrt((d * d).sum(1).mean()))


# ---- the same objective written once more, on PCL's parameters, for scipy

def euler_pose(v):
    """PCL's parameters of the optimisation: x, y, z, roll, pitch, yaw"""
    (ca, cb, cg), (sa, sb, sg) = np.cos(v[3:]), np.sin(v[3:])
    X = np.eye(4)
    X[:3, :3] = [[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca], [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca],
                 [-sb, cb * sa, cb * ca]]
    X[:3, 3] = v[:3]
    return X


def scipy_minimum(p, s, q, n, eps):
    """the smallest F that scipy's BFGS finds, started at identity and once more from where it stopped"""
    from scipy.optimize import minimize
    W = np.linalg.inv(side(s, eps) + side(n, eps))

    def F(v):
        X = euler_pose(v)
        r = p @ X[:3, :3].T + X[:3, 3] - q
        return float(np.einsum("ma,mab,mb->", r, W, r)) / len(p)
    res = minimize(F, np.zeros(6), method="BFGS", options=dict(gtol=1e-10))
    res = minimize(F, res.x, method="BFGS", options=dict(gtol=1e-10))
    return float(res.fun)


# ---- what the host test holds the reference against: plain loops, written independently

def naive_weight(s, n, eps):
    def cov(v):
        if not all(math.isfinite(x) for x in v) or not sum(x * x for x in v) > 0.0:
            return [[1.0 if a == b else 0.0 for b in range(3)] for a in range(3)]
        l = math.sqrt(sum(x * x for x in v))
        u = [x / l for x in v]
        return [[(1.0 if a == b else 0.0) - (1.0 - eps) * u[a] * u[b] for b in range(3)] for a in range(3)]
    A, B = cov(list(s)), cov(list(n))
    return np.linalg.inv(np.array([[A[a][b] + B[a][b] for b in range(3)] for a in range(3)]))


def naive_F(p, s, q, n, X, eps):
    """(1 / m) sum r^T W r, one correspondence at a time"""
    total = 0.0
    for k in range(len(p)):
        W = naive_weight(s[k], n[k], eps)
        r = X[:3, :3] @ p[k] + X[:3, 3] - q[k]
        total += float(r @ W @ r)
    return total / len(p)


def naive_sums(p, s, q, n, X, eps):
    out = np.zeros(29)
    for k in range(len(p)):
        W = naive_weight(s[k], n[k], eps)
        y = X[:3, :3] @ p[k] + X[:3, 3]
        r = y - q[k]
        J = np.zeros((3, 6))
        J[:, :3] = -np.array([[0.0, -y[2], y[1]], [y[2], 0.0, -y[0]], [-y[1], y[0], 0.0]])
        J[:, 3:] = np.eye(3)
        H, g = J.T @ W @ J, J.T @ W @ r
        t = 0
        for a in range(6):
            for b in range(a, 6):
                out[t] += H[a, b]
                t += 1
        out[21:27] += g
        out[27] += 1.0
        out[28] += float(r @ W @ r)
    return out
