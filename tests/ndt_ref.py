"""A numpy f64 restatement of rules N2-N9 of include/mvr_hip.h (the Normal Distributions Transform), independent of the
product: the tests of the NDT compare the library against this file, and tests/test_ndt_host.py checks this file against
central differences and closed forms.  Vectorised over (point, candidate cell); it never imports the product."""
import numpy as np

MU = 1e-4
STOPS = ("NOT", "STEP", "ITERATIONS", "FLAT", "NO_DECREASE", "NO_OVERLAP")
DEFAULTS = dict(resolution=1.0, step_size=0.1, outlier_ratio=0.55, transformation_epsilon=0.1, min_covar_eigvalue_mult=0.01,
                origin=(0.0, 0.0, 0.0), max_iterations=35, max_line_evals=10, min_points_per_voxel=6)
TRIU = np.triu_indices(6)


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        assert k in p, k
    p.update(kw)
    return p


def constants(resolution, outlier_ratio):
    """N2 -> (d1, d2, d3)"""
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / (resolution * resolution * resolution)
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return float(d1), float(d2), float(d3)


# ---- N3
def lattice(tgt, resolution):
    """the f32 voxel index of mvr_cloud_voxel_grid (rules 2-4) for a cubic leaf -> (inv f32, min_b int64[3], div int64[3])"""
    p = np.asarray(tgt, np.float32)[:, :3]
    p = p[np.isfinite(p).all(1)]
    inv = np.float32(1.0) / np.float32(resolution)
    min_b = np.floor(p.min(0) * inv).astype(np.int64)
    max_b = np.floor(p.max(0) * inv).astype(np.int64)
    return inv, min_b, max_b - min_b + 1


def voxel_of(points, lat):
    """ijk (int64, may lie outside the lattice) of f64 or f32 points, by the f32 rule"""
    inv, min_b, _ = lat
    with np.errstate(over="ignore", invalid="ignore"):      # (a finite point far beyond the int64 range: some index outside)
        f = np.floor(np.asarray(points).astype(np.float32) * inv) - min_b.astype(np.float32)
        far = ~(np.abs(f) < 2.0 ** 62)
        return np.where(far, -(2 ** 62), np.where(far, 0.0, f).astype(np.int64))


def build_cells(tgt, prm):
    res, mult = prm["resolution"], prm["min_covar_eigvalue_mult"]
    min_points = max(3, int(prm["min_points_per_voxel"]))
    t32 = np.asarray(tgt, np.float32)[:, :3]
    ok = np.isfinite(t32).all(1)
    out = dict(key=np.zeros(0, np.uint64), count=np.zeros(0, np.uint32), mean=np.zeros((0, 3)), icov=np.zeros((0, 6)), lat=None,
               eig_ratio=np.zeros(0), inflated=np.zeros(0, bool))
    if not ok.any():
        return out
    lat = lattice(t32, res)
    out["lat"] = lat
    div = lat[2]
    ijk = voxel_of(t32[ok], lat)
    key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    pts = t32[ok].astype(np.float64)
    order = np.argsort(key, kind="stable")
    key, pts = key[order], pts[order]
    uk, start, cnt = np.unique(key, return_index=True, return_counts=True)
    keys, counts, means, icovs, ratios, infl = [], [], [], [], [], []
    for k, b, n in zip(uk, start, cnt):
        if n < min_points:
            continue
        q = pts[b:b + n]
        m = q.sum(0) / n
        d = q - m
        Cm = ((n - 1.0) / n) * (1.0 / n) * (d.T @ d)
        lam, V = np.linalg.eigh(Cm)
        lmax = lam[2]
        if not (np.isfinite(lam).all() and lmax > 0.0):
            continue
        lp = np.maximum(lam, mult * lmax)
        Ci = (V / lp) @ V.T
        keys.append(k); counts.append(n); means.append(m)
        icovs.append([Ci[0, 0], Ci[0, 1], Ci[0, 2], Ci[1, 1], Ci[1, 2], Ci[2, 2]])
        ratios.append(lmax / lp.min()); infl.append(bool((lam < mult * lmax).any()))
    if keys:
        out.update(key=np.array(keys, np.uint64), count=np.array(counts, np.uint32), mean=np.array(means), icov=np.array(icovs),
                   eig_ratio=np.array(ratios), inflated=np.array(infl))
    return out


# ---- N4, N6: the matrices the host forms
def axis_rotation(ax, a, order):
    """the rotation about axis ax, differentiated `order` times: the angle shifted by order * pi / 2 (taken exactly), constant
    entries zeroed for order > 0"""
    c0, s0 = np.cos(a), np.sin(a)
    c, s = [(c0, s0), (-s0, c0), (-c0, -s0)][order]
    M = np.zeros((3, 3))
    i, j = (ax + 1) % 3, (ax + 2) % 3
    M[ax, ax] = 1.0 if order == 0 else 0.0
    M[i, i] = c; M[i, j] = -s; M[j, i] = s; M[j, j] = c
    return M


def rot(r, ox=0, oy=0, oz=0):
    return axis_rotation(0, r[0], ox) @ axis_rotation(1, r[1], oy) @ axis_rotation(2, r[2], oz)


def pose_matrix(p, origin=(0.0, 0.0, 0.0), G=None):
    """X(p) G, 4x4 f64: y = R (x - o) + o + t"""
    p, o = np.asarray(p, np.float64), np.asarray(origin, np.float64)
    X = np.eye(4)
    X[:3, :3] = rot(p[3:])
    X[:3, 3] = o + p[:3] - X[:3, :3] @ o
    return X if G is None else X @ np.asarray(G, np.float64)


OFFSETS = [(di, dj, dk) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1)]      # ascending voxel index


def sums(src, cells, prm, p=None, G=None, with_abs=False):
    """N5, N6 -> the 29 sums (and, with_abs, the sums of the terms' absolute values)"""
    out, mag = np.zeros(29), np.zeros(29)
    p = np.zeros(6) if p is None else np.asarray(p, np.float64)
    if len(cells["key"]) == 0 or len(src) == 0:
        return (out, mag) if with_abs else out
    res = prm["resolution"]
    d1, d2, _ = constants(res, prm["outlier_ratio"])
    o = np.asarray(prm["origin"], np.float64)
    x = np.asarray(src, np.float32)[:, :3].astype(np.float64)
    if G is not None:
        G = np.asarray(G, np.float64)
        x = x @ G[:3, :3].T + G[:3, 3]
    xt = x - o
    r = p[3:]
    y = xt @ rot(r).T + o + p[:3]
    ok = np.isfinite(y).all(1)
    xt, y = xt[ok], y[ok]
    D = [rot(r, 1, 0, 0), rot(r, 0, 1, 0), rot(r, 0, 0, 1)]
    DD = {(0, 0): rot(r, 2, 0, 0), (0, 1): rot(r, 1, 1, 0), (0, 2): rot(r, 1, 0, 1), (1, 1): rot(r, 0, 2, 0), (1, 2): rot(r, 0, 1, 1),
          (2, 2): rot(r, 0, 0, 2)}
    n = len(y)
    J = np.zeros((n, 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    for k in range(3):
        J[:, :, 3 + k] = xt @ D[k].T
    K = np.zeros((n, 6, 6, 3))
    for (i, j), M in DD.items():
        K[:, 3 + i, 3 + j] = K[:, 3 + j, 3 + i] = xt @ M.T
    lat = cells["lat"]
    div = lat[2]
    h = voxel_of(y, lat)
    keys = cells["key"].astype(np.int64)
    ic = cells["icov"]
    Cfull = np.stack([ic[:, [0, 1, 2]], ic[:, [1, 3, 4]], ic[:, [2, 4, 5]]], 1)
    H, Ha = np.zeros((6, 6)), np.zeros((6, 6))
    g, ga = np.zeros(6), np.zeros(6)
    cnt, s, sa = 0.0, 0.0, 0.0
    for off in OFFSETS:
        ijk = h + np.asarray(off)
        inside = ((ijk >= 0) & (ijk < div)).all(1)
        key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
        pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
        hit = inside & (keys[pos] == key)
        idx, cell = np.nonzero(hit)[0], pos[hit]
        d = y[idx] - cells["mean"][cell]
        near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= res * res
        idx, cell, d = idx[near], cell[near], d[near]
        Ci = Cfull[cell]
        v = np.einsum("nij,nj->ni", Ci, d)
        q = np.einsum("ni,ni->n", d, v)
        e = np.exp(-d2 * q / 2.0)
        w = d2 * e
        with np.errstate(invalid="ignore"):
            good = (w >= 0.0) & (w <= 1.0)
        idx, d, Ci, v, e, w = idx[good], d[good], Ci[good], v[good], e[good], w[good]
        Jn, Kn = J[idx], K[idx]
        a = np.einsum("nc,nci->ni", v, Jn)
        M = np.einsum("nci,ncd,ndj->nij", Jn, Ci, Jn)
        vK = np.einsum("nc,nijc->nij", v, Kn)
        f = d1 * w
        Ht = f[:, None, None] * (M - d2 * a[:, :, None] * a[:, None, :] + vK)
        gt = f[:, None] * a
        H += Ht.sum(0); Ha += np.abs(Ht).sum(0)
        g += gt.sum(0); ga += np.abs(gt).sum(0)
        cnt += len(idx)
        s += (-d1 * e).sum(); sa += np.abs(d1 * e).sum()
    out[:21], out[21:27], out[27], out[28] = H[TRIU], g, cnt, s
    mag[:21], mag[21:27], mag[27], mag[28] = Ha[TRIU], ga, cnt, sa
    return (out, mag) if with_abs else out


def unpack(s29):
    H = np.zeros((6, 6))
    H[TRIU] = s29[:21]
    H = H + H.T - np.diag(np.diag(H))
    return H, s29[21:27], s29[27], s29[28]


# ---- N7
def direction(s29):
    """-> delta (6) = -H^+ g, or None where N7 says FLAT on |delta|"""
    H, g, _, _ = unpack(s29)
    if not (np.isfinite(H).all() and np.isfinite(g).all()):
        return None
    lam, V = np.linalg.eigh(H)
    thr = 6.0 * 2.0 ** -52 * np.abs(lam).max()
    delta = np.zeros(6)
    for k in range(6):
        if abs(lam[k]) > thr:
            delta -= V[:, k] * ((V[:, k] @ g) / lam[k])
    return delta


# ---- N7-N9
def align(src, cells, prm, G=None, evaluate=None):
    """-> dict(stop, converged, iterations, evaluations, p, X, score, count, sums, trace, margins); margins: for every decision
    of the line search, |lhs - rhs| / |s(0)| (test_ndt_host.py asks that none is a near-tie).  evaluate(p) -> the 29 sums, in
    place of sums(src, cells, prm, p, G): the loop on a script (src and cells are then not looked at)"""
    if evaluate is None:
        evaluate = lambda q: sums(src, cells, prm, q, G)
    with np.errstate(all="ignore"):          # (a scripted score may be 0, infinite or not a number: the margins are then, too)
        return _newton(prm, G, evaluate)


def _newton(prm, G, evaluate):
    eps, step = prm["transformation_epsilon"], prm["step_size"]
    p = np.zeros(6)
    cur = np.asarray(evaluate(p.copy()), np.float64)
    evals, iters, stop, trace, margins = 1, 0, "NOT", [], []
    if not cur[27] > 0.0:
        stop = "NO_OVERLAP"
    while stop == "NOT":
        rec = dict(a=0.0, delta_norm=0.0, trials=0, reversed=False, fallback=False)
        delta = direction(cur)
        dn = float(np.sqrt(delta @ delta)) if delta is not None else float("nan")
        rec["delta_norm"] = dn
        if not (np.isfinite(dn) and dn > 0.0):
            stop = "FLAT"
        else:
            u = delta / dn
            dphi = -(cur[21:27] @ u)
            if dphi > 0.0:
                u, dphi, rec["reversed"] = -u, -dphi, True
            if not dphi < 0.0:
                stop = "FLAT"
        if stop == "NOT":
            a, taken, best = min(dn, step), None, None
            while rec["trials"] < prm["max_line_evals"]:
                tr = np.asarray(evaluate(p + a * u), np.float64)
                evals += 1; rec["trials"] += 1
                s0, sa = cur[28], tr[28]
                margins.append(abs((-s0 + MU * a * dphi) - (-sa)) / abs(s0))
                if -sa <= -s0 + MU * a * dphi:
                    taken = (a, tr)
                    break
                margins.append(abs(sa - s0) / abs(s0))
                if sa > s0 and (best is None or sa > best[1][28]):
                    if best is not None:
                        margins.append(abs(sa - best[1][28]) / abs(s0))
                    best = (a, tr)
                a *= 0.5
                if a < eps / 2.0:
                    break
            if taken is None and best is not None:
                taken, rec["fallback"] = best, True
            if taken is None:
                stop = "NO_DECREASE"
            else:
                p = p + taken[0] * u
                cur = taken[1]
                iters += 1
                rec["a"] = taken[0]
                if taken[0] < eps:
                    stop = "STEP"
                elif iters >= prm["max_iterations"]:
                    stop = "ITERATIONS"
        rec.update(stop=stop, score=cur[28], count=cur[27], p=p.copy())
        trace.append(rec)
    return dict(stop=stop, converged=stop in ("STEP", "ITERATIONS"), iterations=iters, evaluations=evals, p=p,
                X=pose_matrix(p, prm["origin"], G), score=cur[28], count=cur[27], sums=cur, trace=trace, margins=margins)
