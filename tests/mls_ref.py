"""numpy reference of the moving-least-squares smoothing (include/mvr_hip.h: mvr_cloud_mls, rules M1-M6), all in f64, by two
independent routes:

  route A  moments of the neighbours about the query point, covariance, numpy's eigh, u from the axis the normal leans on
           least, the 6 x 6 normal equations of the basis 1, b, b^2, a, ab, a^2 solved by Cholesky (a pivot that is not
           finite and positive abandons the fit) -- the arithmetic the rules describe;
  route B  the centroid in absolute coordinates, an SVD of the centred neighbour matrix for the plane, a different pair
           u, v, and the weighted least-squares problem itself (rows scaled by sqrt(w)) through the pseudo-inverse -- no
           normal equations, no covariance.

Neighbour membership is the library's f32 rule, through outlier_ref.within_r2 (candidates from a kd-tree over the finite
points with a wide margin).  Per point the reference reports the neighbour count, the relative eigen-gap (l1 - l0) / l2 of the
covariance and the condition number of the 6 x 6 system, raw (`cond`) and written in units of the radius (`cond_r`).  A point
is EXCLUDED from value comparisons when its gap is below 1e-6, when its polynomial applies and cond_r exceeds 1e10, or when the
two routes differ by more than 1e-9 radii in a coordinate or 1e-9 in a component of the unit normal (`rel_plane`, `rel_poly`).
Kept set, order and counts are never excluded.

The exclusion rules know no unit of length.  The problem is homogeneous: the cloud and the radius times a power of two give
route A's coordinates times that power, and its normals and curvature unchanged, bit for bit (tests/test_mls_host.py asserts
it).  So the yardsticks are homogeneous too: the condition number is that of D A D with D = diag(r^-deg) over the basis 1, b,
b^2, a, ab, a^2 -- the system of the offsets a / r, b / r --, route B solves its least-squares problem in those offsets (the
cut-off of the pseudo-inverse compares singular values, which in raw offsets span 1 to r^2), and the routes' distance is
taken in radii.  The raw condition number and the raw distances (`cond`, `diff_plane`, `diff_poly`, in the cloud's unit) are
still reported; nothing is decided on them.

The curvature |l0| / (l0 + l1 + l2) has a blind spot of its own: where the neighbours are coplanar -- always, with exactly 3
of them -- l0 is exactly 0 and what any implementation computes is the rounding noise of its eigen-solver, about 1e-16 l2.
The same third rule covers it: the curvature (and only the curvature) of a point is left out of value comparisons where the
two routes' curvatures (eigh of the covariance; squared singular values of the centred neighbour matrix) differ by more than
1e-9 relative (curvature_unpinned).  A component of the unit normal that is exactly 0 has the same blind spot and the same rule
(normal_unpinned)."""
import numpy as np

from outlier_ref import finite_mask, neighbor_counts, within_r2

F32, F64 = np.float32, np.float64
MIN_GAP, MAX_COND, MAX_ROUTE_DIFF = 1e-6, 1e10, 1e-9


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _dot(a, b):
    return (a * b).sum(-1)


def _chunks(p, radius, fma, rows, budget=4e6):
    """yields (row indices, q[m, 3] f64, X[m, K, 3] f64 neighbour coordinates, member[m, K] bool) over the queries `rows` of
    the cloud p: member marks the finite points j with the f32 d2(i, j) <= f32(radius * radius), i itself included (M1); a
    non-finite query has none (M2)"""
    from scipy.spatial import cKDTree
    p = np.asarray(p, F32)
    rows = np.arange(len(p)) if rows is None else np.asarray(rows, np.int64)
    if len(rows) == 0:
        return
    fin = finite_mask(p)
    P = np.ascontiguousarray(p[fin, :3])
    if len(P) == 0:
        yield rows, np.zeros((len(rows), 3)), np.zeros((len(rows), 1, 3)), np.zeros((len(rows), 1), bool)
        return
    r2 = F32(min(radius * radius, float(np.finfo(F32).max)))
    P64 = P.astype(F64)
    tree = cKDTree(P64)
    rad = radius * (1.0 + 1e-4) + 1e-6 * float(np.abs(P64).max())         # (in the cloud's own unit: no absolute length)
    qf = fin[rows]
    q32 = np.where(qf[:, None], p[rows, :3], P[0]).astype(F32)        # (a non-finite query: a finite stand-in, masked below)
    Q = q32.astype(F64)
    cnt = np.minimum(tree.query_ball_point(Q, rad, return_length=True, workers=-1), len(P))
    c0 = 0
    while c0 < len(rows):
        K, c1 = max(int(cnt[c0]), 1), c0 + 1
        while c1 < len(rows) and max(K, int(cnt[c1])) * (c1 + 1 - c0) <= budget:
            K = max(K, int(cnt[c1]))
            c1 += 1
        _, idx = tree.query(Q[c0:c1], k=K, distance_upper_bound=rad, workers=-1)
        idx = np.asarray(idx).reshape(c1 - c0, K)
        valid = idx < len(P)
        idx = np.where(valid, idx, 0)
        member = valid & qf[c0:c1, None] & within_r2(q32[c0:c1, None, :], P[idx], r2, fma)
        yield rows[c0:c1], Q[c0:c1], P64[idx], member
        c0 = c1


def counts(p, radius, fma=False, rows=None):
    """neighbour count of every query (the point itself included; 0 for a non-finite point)"""
    n = len(p) if rows is None else len(rows)
    out = np.zeros(n, np.int64)
    o = 0
    for r, q, X, member in _chunks(p, radius, fma, rows):
        out[o:o + len(r)] = member.sum(1)
        o += len(r)
    return out


def kept_index(p, radius, fma=False):
    """the original indices of the output points: at least 3 neighbours (M3).  A small cloud is counted pair by pair
    (outlier_ref.neighbor_counts: the other points within the radius, so + 1 for the point itself)"""
    p = np.asarray(p, F32)
    if len(p) == 0:
        return np.zeros(0, np.uint32)
    if len(p) <= 8192:
        cnt = np.where(finite_mask(p), neighbor_counts(p, radius, fma).astype(np.int64) + 1, 0)
    else:
        cnt = counts(p, radius, fma)
    return np.nonzero(cnt >= 3)[0].astype(np.uint32)


def membership_differs(p, radius, rows=None):
    """does the fma chain of the distance change any neighbour set?"""
    a, b = _chunks(p, radius, False, rows), _chunks(p, radius, True, rows)
    return any(not np.array_equal(x[3], y[3]) for x, y in zip(a, b))


def _cholesky_solve(A, r):
    """A c = r for stacks of 6 x 6 systems by Cholesky; ok[m] false where a pivot was not finite and positive or a
    coefficient the result uses (c0, c1, c3) is not finite (M5)"""
    m = len(A)
    L = np.zeros_like(A)
    ok = np.ones(m, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(6):
            s = A[:, j, j] - (L[:, j, :j] ** 2).sum(1)
            ok &= np.isfinite(s) & (s > 0)
            d = np.sqrt(np.where(ok, s, 1.0))
            L[:, j, j] = d
            for i in range(j + 1, 6):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)) / d
        y = np.zeros((m, 6))
        for i in range(6):
            y[:, i] = (r[:, i] - (L[:, i, :i] * y[:, :i]).sum(1)) / L[:, i, i]
        c = np.zeros((m, 6))
        for i in range(5, -1, -1):
            c[:, i] = (y[:, i] - (L[:, i + 1:, i] * c[:, i + 1:]).sum(1)) / L[:, i, i]
    ok &= np.isfinite(c[:, [0, 1, 3]]).all(1)             # (a positive pivot can be as small as a denormal)
    return c, ok


def _basis(a, b):
    return np.stack([np.ones_like(a), b, b * b, a, a * b, a * a], -1)


_DEG = np.array([0.0, 1.0, 2.0, 1.0, 2.0, 2.0])          # the degrees of the basis 1, b, b^2, a, ab, a^2


def _cond(A):
    out = np.full(len(A), np.inf)
    fin = np.isfinite(A).all(axis=(1, 2))
    if fin.any():
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            out[fin] = np.linalg.cond(A[fin])
    return out


def _route_a(q, X, member, g, radius):
    """-> dict of per-point f64 results of route A"""
    m = len(q)
    w01 = member.astype(F64)
    cnt = member.sum(1)
    c = np.maximum(cnt, 1).astype(F64)
    d = (X - q[:, None, :]) * w01[:, :, None]
    mean = d.sum(1) / c[:, None]
    C = np.einsum("mki,mkj->mij", d, d) / c[:, None, None] - mean[:, :, None] * mean[:, None, :]
    ev, V = np.linalg.eigh(C)
    n = _unit(V[:, :, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        s = ev.sum(1)
        curv = np.where(s != 0, np.abs(ev[:, 0]) / np.where(s != 0, s, 1.0), 0.0)
        gap = np.where(ev[:, 2] > 0, (ev[:, 1] - ev[:, 0]) / np.where(ev[:, 2] > 0, ev[:, 2], 1.0), 0.0)
    t = _dot(mean, n)
    plane = q + t[:, None] * n
    # u from the axis n leans on least, v = n x u
    e = np.eye(3)[np.argmin(np.abs(n), axis=1)]
    u = _unit(np.cross(e, n))
    v = np.cross(n, u)
    dd = (X - q[:, None, :]) - (t[:, None] * n)[:, None, :]
    a, b, f = _dot(dd, u[:, None, :]), _dot(dd, v[:, None, :]), _dot(dd, n[:, None, :])
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        w = np.exp(-_dot(dd, dd) / g) * w01
    Phi = _basis(a, b)
    A = np.einsum("mk,mki,mkj->mij", w, Phi, Phi)
    r = np.einsum("mk,mki->mi", w * f, Phi)
    applies = cnt >= 6
    A[~applies] = np.eye(6)
    cond = _cond(A)
    # the same system in units of the radius, for the exclusion rule alone: D A D, D = diag(radius^-deg)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        D = float(radius) ** -_DEG
        cond_r = _cond(A * D[None, :, None] * D[None, None, :])
    coef, ok = _cholesky_solve(A, r)
    ok &= applies
    # a diagonal entry of A is a sum of terms w phi^2, none negative: exactly 0 in one order of summation, it is exactly 0 in
    # every order, and its pivot is not positive -- the one abandoned fit that does not hang on a rounding
    zero_diag = applies & (np.diagonal(A, axis1=1, axis2=2) == 0).any(1)
    c0 = np.where(ok, coef[:, 0], 0.0)
    poly = plane + c0[:, None] * n
    pn = _unit(n - coef[:, 3:4] * u - coef[:, 1:2] * v)
    pn = np.where(ok[:, None], pn, n)
    return dict(count=cnt, gap=gap, cond=np.where(applies, cond, 1.0), cond_r=np.where(applies, cond_r, 1.0), curv=curv, plane=plane,
                normal=n, poly=poly, poly_normal=pn, fit=ok, zero_diag=zero_diag)


def _route_b(q, X, member, g, radius):
    w01 = member.astype(F64)
    cnt = member.sum(1)
    c = np.maximum(cnt, 1).astype(F64)
    cen = (X * w01[:, :, None]).sum(1) / c[:, None]
    Y = (X - cen[:, None, :]) * w01[:, :, None]
    if Y.shape[1] < 3:
        Y = np.concatenate([Y, np.zeros((len(Y), 3 - Y.shape[1], 3))], 1)
    _, sv, Vt = np.linalg.svd(Y, full_matrices=False)
    n = _unit(Vt[:, 2, :])
    s2 = (sv * sv).sum(1)
    curv = np.where(s2 != 0, sv[:, 2] ** 2 / np.where(s2 != 0, s2, 1.0), 0.0)
    plane = q - _dot(q - cen, n)[:, None] * n
    k = np.array([0.36, 0.48, 0.8])
    k2 = np.array([0.8, -0.6, 0.0])
    par = np.abs(n @ k) > 0.9
    u = _unit(np.cross(n, np.where(par[:, None], k2, k)))
    v = np.cross(n, u)
    dd = X - plane[:, None, :]
    a, b, f = _dot(dd, u[:, None, :]), _dot(dd, v[:, None, :]), _dot(dd, n[:, None, :])
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        sw = np.sqrt(np.exp(-_dot(dd, dd) / g)) * w01
    # the least-squares problem in units of the radius: f / r over the basis of a / r, b / r; then c0 is in radii and c1, c3 are
    # slopes, which have no unit (the other three are not used)
    ir = 1.0 / float(radius)
    M = _basis(a * ir, b * ir) * sw[:, :, None]
    M = np.where(np.isfinite(M), M, 0.0)
    fr = f * ir
    coef = np.einsum("mik,mk->mi", np.linalg.pinv(M), np.where(np.isfinite(fr), fr, 0.0) * sw) if M.shape[1] >= 6 else np.zeros((len(q), 6))
    coef[:, 0] *= float(radius)
    poly = plane + coef[:, 0:1] * n
    pn = _unit(n - coef[:, 3:4] * u - coef[:, 1:2] * v)
    return dict(plane=plane, normal=n, poly=poly, poly_normal=pn, curv=curv)


def _sign_free_diff(a, b):
    return np.minimum(np.abs(a - b).max(1), np.abs(a + b).max(1))


def fit(p, radius, sqr_gauss_param=0.0, fma=False, rows=None, second_route=True):
    """Both orders at once for the queries `rows` (default: every point) of the cloud p, per query (f64 unless said):
      count, gap, cond (raw coordinates), cond_r (in units of the radius), curv, keep (count >= 3)
      plane / normal          the order-0/1 result (M4)
      poly / poly_normal      the order-2 result (M5; the plane's where the polynomial does not apply or was abandoned)
      diff_plane / diff_poly  largest difference between the two routes, coordinates (in the cloud's unit) and normal components
                              together
      rel_plane / rel_poly    the same with the coordinates' difference in radii: what excluded() decides on
      diff_curv               relative difference between the two routes' curvatures
      normal_b / poly_normal_b  route B's normals, on route A's side (the plane's where route A abandoned the fit)
      plane_b / poly_b        route B's coordinates (its polynomial is always solved, also where route A abandoned the fit)
      fit                     the polynomial applied and its fit stood (bool)
      zero_diag               the polynomial applied and a diagonal entry of the normal equations is exactly 0: the fit is
                              abandoned whatever the order of the sums.  Any other abandoned fit hangs on the sign of a pivot
                              that is rounding noise about 0 (a positive semi-definite matrix has no negative pivot), and
                              another order of summation may well keep it (tests/test_mls_host.py shows it on the reference)
    """
    p = np.asarray(p, F32)
    n = len(p) if rows is None else len(rows)
    g = float(sqr_gauss_param) if sqr_gauss_param != 0.0 else float(radius) * float(radius)
    keys3 = ("plane", "normal", "poly", "poly_normal")
    out = {k: np.full((n, 3), np.nan) for k in keys3 + ("plane_b", "poly_b", "normal_b", "poly_normal_b")}
    for k in ("gap", "cond", "cond_r", "curv", "diff_plane", "diff_poly", "diff_curv", "rel_plane", "rel_poly"):
        out[k] = np.full(n, np.nan)
    out["count"] = np.zeros(n, np.int64)
    out["fit"] = np.zeros(n, bool)
    out["zero_diag"] = np.zeros(n, bool)
    o = 0
    for r, q, X, member in _chunks(p, radius, fma, rows):
        sl = slice(o, o + len(r))
        o += len(r)
        A = _route_a(q, X, member, g, radius)
        for k in keys3 + ("gap", "cond", "cond_r", "curv", "count", "fit", "zero_diag"):
            out[k][sl] = A[k]
        if second_route:
            B = _route_b(q, X, member, g, radius)
            out["plane_b"][sl], out["poly_b"][sl] = B["plane"], B["poly"]
            with np.errstate(invalid="ignore"):
                nb = B["normal"] * np.where(_dot(A["normal"], B["normal"]) < 0, -1.0, 1.0)[:, None]
                pb = B["poly_normal"] * np.where(_dot(A["poly_normal"], B["poly_normal"]) < 0, -1.0, 1.0)[:, None]
            out["normal_b"][sl], out["poly_normal_b"][sl] = nb, np.where(A["fit"][:, None], pb, nb)
            out["diff_plane"][sl] = np.maximum(np.abs(A["plane"] - B["plane"]).max(1), _sign_free_diff(A["normal"], B["normal"]))
            # (route B always solves the least-squares problem; it is compared where route A's fit stood)
            dp = np.maximum(np.abs(A["poly"] - B["poly"]).max(1), _sign_free_diff(A["poly_normal"], B["poly_normal"]))
            out["diff_poly"][sl] = np.where(A["fit"], dp, out["diff_plane"][sl])
            ir = 1.0 / float(radius)
            out["rel_plane"][sl] = np.maximum(np.abs(A["plane"] - B["plane"]).max(1) * ir, _sign_free_diff(A["normal"], B["normal"]))
            rp = np.maximum(np.abs(A["poly"] - B["poly"]).max(1) * ir, _sign_free_diff(A["poly_normal"], B["poly_normal"]))
            out["rel_poly"][sl] = np.where(A["fit"], rp, out["rel_plane"][sl])
            big = np.maximum(A["curv"], B["curv"])
            out["diff_curv"][sl] = np.where(big > 0, np.abs(A["curv"] - B["curv"]) / np.where(big > 0, big, 1.0), 0.0)
    out["keep"] = out["count"] >= 3
    return out


def excluded(R, order):
    """the points of fit()'s result that take no part in value comparisons at this order (dropped points are not counted)"""
    poly = (order == 2) & (R["count"] >= 6)
    diff = np.where(poly, R["rel_poly"], R["rel_plane"])
    with np.errstate(invalid="ignore"):
        bad = (R["gap"] < MIN_GAP) | (poly & (R["cond_r"] > MAX_COND)) | ~(diff <= MAX_ROUTE_DIFF)
    return bad & R["keep"]


def curvature_unpinned(R):
    """the kept points whose curvature the reference cannot pin (coplanar neighbours: l0 is rounding noise)"""
    with np.errstate(invalid="ignore"):
        return ~(R["diff_curv"] <= MAX_ROUTE_DIFF) & R["keep"]


def normal_unpinned(R, order):
    """[n, 3] bool: the components of the kept points' normals that the reference cannot pin to an f32 ulp -- the two routes
    differ by more than 1e-9 of the component itself.  That is a component that is 0 in exact arithmetic (an axis-aligned
    normal on a lattice; three neighbours that share a coordinate in a far frame, where every coordinate is a multiple of
    1 / 16): each route returns its own rounding noise, 1e-17 or an exact 0, and one f32 ulp of THAT is no bar any f64
    arithmetic can meet.  Such a component is held to the bar the routes themselves are held to, 1e-9 absolute"""
    a, b = (R["poly_normal"], R["poly_normal_b"]) if order == 2 else (R["normal"], R["normal_b"])
    with np.errstate(invalid="ignore"):
        # (two routes that both return an exact 0 agree, and pin nothing: below the routes' own bar the relative test is void)
        return (~(np.abs(a - b) <= MAX_ROUTE_DIFF * np.abs(a)) | (np.abs(a) < MAX_ROUTE_DIFF)) & R["keep"][:, None]


def flip(nf, ref):
    """the f32 orientation test: negate n where dot(ref, n) < 0 (strictly), the products and sums rounded one by one"""
    nf, ref = np.asarray(nf, F32), np.asarray(ref, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        cs = (ref[:, 0] * nf[:, 0] + ref[:, 1] * nf[:, 1]) + ref[:, 2] * nf[:, 2]
        neg = cs < 0
    out = nf.copy()
    out[neg] = -out[neg]
    return out


def result(p, R, order, viewpoint=(0.0, 0.0, 0.0), src_normals=None, rows=None):
    """what mvr_cloud_mls returns for the kept queries of R (M3, M6): dict(index = positions in `rows` of the kept queries,
    xyz f32, xyz64, normal f32 -- oriented towards the viewpoint seen from the source point, or along src_normals -- and
    curvature f32)"""
    p = np.asarray(p, F32)
    src = p if rows is None else p[np.asarray(rows, np.int64)]
    keep = R["keep"]
    xyz64 = (R["poly"] if order == 2 else R["plane"])[keep]
    nrm = (R["poly_normal"] if order == 2 else R["normal"])[keep].astype(F32)
    if src_normals is not None:
        ref = np.asarray(src_normals, F32)[:, :3]
        ref = (ref if rows is None else ref[np.asarray(rows, np.int64)])[keep]
    else:
        ref = np.asarray(viewpoint, F32)[None, :] - src[keep, :3]
    return dict(index=np.nonzero(keep)[0].astype(np.uint32), xyz=xyz64.astype(F32), xyz64=xyz64, normal=flip(nrm, ref),
                curvature=R["curv"][keep].astype(F32))


def within_one_ulp(got, ref):
    """elementwise: got is ref or one of its two f32 neighbours"""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    return (got == ref) | (got == np.nextafter(ref, F32(np.inf))) | (got == np.nextafter(ref, F32(-np.inf)))
