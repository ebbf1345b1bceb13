"""numpy reference of the two outlier filters (include/mvr_hip.h: mvr_cloud_statistical_outlier_removal,
mvr_cloud_radius_outlier_removal): the library's f32 distance, the mean of the correctly rounded f32 square roots of the
mean_k smallest d2 summed in f64 in ascending order, two-pass f64 statistics, the <= rule of the radius count; non-finite
points are outliers and nobody's neighbour.  Candidates come from a kd-tree over the f64 coordinates; every distance that
decides anything is recomputed in f32, and a row whose candidate set cannot be shown wide enough is redone by brute force."""
import numpy as np

F32, F64 = np.float32, np.float64


def finite_mask(p):
    return np.isfinite(np.asarray(p, F32)[:, :3]).all(axis=1)


def d2_f32(a, b, fma=False):
    """the library's distance between the f32 points a[..., 3] and b[..., 3]: (dx*dx + dy*dy) + dz*dz with every operation
    rounded, or (fma) fma(dz, dz, fma(dy, dy, dx*dx))"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
        if not fma:
            return (dx * dx + dy * dy) + dz * dz
        # an f32 fma is one rounding of the exact a * b + c.  The product of two f32 is exact in 48 bits; in the 64-bit mantissa
        # of the x87 long double the sum is exact unless c lies more than 16 bits below the product's last bit, and a double
        # rounding then needs a 40-bit pattern: nothing a test of a few 10^7 distances meets
        L = np.longdouble
        assert np.finfo(L).nmant >= 63, "the fma reference needs an 80-bit long double"
        t = dx * dx
        t = (dy.astype(L) * dy.astype(L) + t.astype(L)).astype(F32)
        return (dz.astype(L) * dz.astype(L) + t.astype(L)).astype(F32)


def within_r2(a, b, r2, fma=False):
    """d2_f32(a, b, fma) <= r2, elementwise.  The fma arm's 80-bit arithmetic is slow, so it is spent only where it can
    decide: both expressions start from the same rounded differences and round three times, so each lies within 3 * 2^-24 of
    the same exact sum and they differ by less than 1e-6 relative -- a plain d2 further than that from r2 settles the fma
    comparison too"""
    p = d2_f32(a, b, False)
    if not fma:
        return p <= r2
    a, b = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32))
    with np.errstate(invalid="ignore", over="ignore"):
        p64, r64 = p.astype(F64), F64(r2)
        out = p64 <= r64 * (1.0 - 1.0e-6)
        amb = ~out & (p64 <= r64 * (1.0 + 1.0e-6))
    if amb.any():
        out[amb] = d2_f32(a[amb], b[amb], True) <= r2
    return out


def _brute_smallest(P, rows, k, fma):
    """the k smallest f32 d2 from each point P[rows] to the OTHER points of P, ascending"""
    out = np.empty((len(rows), k), F32)
    for a, i in enumerate(rows):
        d = d2_f32(P[i][None, :], P, fma)
        d = np.delete(d, i)
        out[a] = np.sort(d)[:k]
    return out


def smallest_d2(P, k, fma=False, pad=None, chunk=200000):
    """[n, k] the k smallest f32 d2 of every point of the finite f32 cloud P[n, 3] to the other points, ascending
    (requires n - 1 >= k)"""
    from scipy.spatial import cKDTree
    n = len(P)
    assert n - 1 >= k
    out = np.empty((n, k), F32)
    m = min(n, k + 1 + (pad if pad is not None else max(8, k // 2)))
    P64 = P.astype(F64)
    tree = cKDTree(P64)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        dist, idx = tree.query(P64[c0:c1], k=m, workers=-1)
        dist, idx = dist.reshape(c1 - c0, m), idx.reshape(c1 - c0, m)
        d = d2_f32(P[c0:c1, None, :], P[idx], fma)
        own = idx == np.arange(c0, c1)[:, None]
        has_own = own.any(axis=1)
        d = np.where(own, F32(np.inf), d)              # the point itself is not its neighbour (its duplicates are)
        d.sort(axis=1)
        out[c0:c1] = d[:, :k]
        # wide enough: every point outside the candidate set is at least as far (f64) as the last candidate; its f32 d2 can be
        # lower by the rounding of three f32 differences and products only (a few 2^-24 relative).  The k-th f32 d2 must lie
        # strictly below that bound, and the point itself must have been among the candidates -- or the set was the whole cloud
        if m < n:
            last = dist[:, -1].astype(F64) ** 2 * (1.0 - 1.0e-6)
            bad = np.nonzero(~((d[:, k - 1].astype(F64) < last) & has_own))[0]
            if len(bad):
                assert len(bad) * n <= 4e9, "too many rows need the brute-force fallback (%d of %d)" % (len(bad), n)
                out[c0 + bad] = _brute_smallest(P, c0 + bad, k, fma)
        else:
            assert has_own.all()
    return out


def mean_dist(p, k, fma=False):
    """(mean_dist[n] f32 with NaN where a point has none, n_valid)"""
    p = np.asarray(p, F32)
    fin = finite_mask(p)
    md = np.full(len(p), np.nan, F32)
    nf = int(fin.sum())
    if nf - 1 < k:
        return md, 0
    d2 = smallest_d2(np.ascontiguousarray(p[fin, :3]), k, fma)
    with np.errstate(over="ignore"):
        sq = np.sqrt(d2)                               # f32 in, f32 out: correctly rounded
    s = np.zeros(nf, F64)
    for j in range(k):                                 # ascending, one after the other
        s += sq[:, j].astype(F64)
    md[fin] = (s / F64(k)).astype(F32)
    return md, nf


def statistics(md, n_valid, stddev_mul):
    """mean / stddev / threshold of the valid mean distances (two passes, f64)"""
    if n_valid == 0:
        return dict(mean=np.nan, stddev=np.nan, threshold=np.nan, n_valid=0)
    v = md[~np.isnan(md)].astype(F64)
    assert len(v) == n_valid
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = v.sum() / n_valid
        sd = np.sqrt(F64(((v - mean) ** 2).sum()) / F64(n_valid - 1))
    return dict(mean=float(mean), stddev=float(sd), threshold=float(mean + stddev_mul * sd), n_valid=n_valid)


def statistical(p, k, stddev_mul, negative=False, fma=False):
    """dict(mean_dist, stats, inlier[n] bool, index = indices of the output points, gap = smallest relative distance between
    a mean distance and the threshold)"""
    p = np.asarray(p, F32)
    fin = finite_mask(p)
    md, nv = mean_dist(p, k, fma)
    st = statistics(md, nv, stddev_mul)
    with np.errstate(invalid="ignore"):
        inl = fin & ~(md.astype(F64) > st["threshold"])
    gap = np.inf
    if nv and np.isfinite(st["threshold"]) and st["threshold"] != 0:
        gap = float(np.min(np.abs(md[fin].astype(F64) - st["threshold"])) / abs(st["threshold"]))
    sel = ~inl if negative else inl
    return dict(mean_dist=md, stats=st, inlier=inl, index=np.nonzero(sel)[0].astype(np.uint32), gap=gap)


def neighbor_counts(p, radius, fma=False):
    """count[i] = number of finite j != i with the f32 d2(i, j) <= f32(radius * radius); 0 for a non-finite point"""
    p = np.asarray(p, F32)
    fin = finite_mask(p)
    cnt = np.zeros(len(p), np.uint32)
    P = np.ascontiguousarray(p[fin, :3])
    if len(P) == 0:
        return cnt
    r2 = F32(radius * radius)
    out = np.zeros(len(P), np.int64)
    if len(P) <= 8192:                                 # small: the definition itself, every pair (no candidate set to trust)
        step = max(1, int(2e7) // len(P))
        for c0 in range(0, len(P), step):
            c1 = min(len(P), c0 + step)
            ok = within_r2(P[c0:c1, None, :], P[None, :, :], r2, fma)
            ok[np.arange(c1 - c0), np.arange(c0, c1)] = False
            out[c0:c1] = ok.sum(axis=1)
        cnt[fin] = out.astype(np.uint32)
        return cnt
    from scipy.spatial import cKDTree
    P64 = P.astype(F64)
    tree = cKDTree(P64)
    for c0 in range(0, len(P), 50000):
        c1 = min(len(P), c0 + 50000)
        cand = tree.query_ball_point(P64[c0:c1], radius * (1.0 + 1e-4) + 1e-4, workers=-1)
        lens = np.fromiter((len(c) for c in cand), np.int64, c1 - c0)
        flat = np.fromiter((j for c in cand for j in c), np.int64, int(lens.sum()))
        row = np.repeat(np.arange(c0, c1), lens)
        ok = within_r2(P[row], P[flat], r2, fma) & (flat != row)
        out[c0:c1] = np.bincount(row[ok] - c0, minlength=c1 - c0)
    cnt[fin] = out.astype(np.uint32)
    return cnt


def radius(p, r, min_neighbors, negative=False, fma=False):
    p = np.asarray(p, F32)
    fin = finite_mask(p)
    cnt = neighbor_counts(p, r, fma)
    inl = fin & (cnt >= min_neighbors)
    sel = ~inl if negative else inl
    return dict(count=cnt, inlier=inl, index=np.nonzero(sel)[0].astype(np.uint32))


def mean_dist_f64(p, k):
    """an anchor that does not pass through the f32 path: mean of the kd-tree's own f64 distances (finite cloud)"""
    from scipy.spatial import cKDTree
    P64 = np.asarray(p, F32)[:, :3].astype(F64)
    dist, _ = cKDTree(P64).query(P64, k=k + 1, workers=-1)
    return dist[:, 1:].sum(axis=1) / k
