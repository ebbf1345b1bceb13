"""numpy reference of the SHOT local reference frames and descriptors (include/mvr_hip.h: mvr_cloud_shot, rules L1-L6 and
H1-H8), all in f64, vectorised over the flat list of (query, neighbour) pairs of a brute-force radius search -- no grid, no
walk, no lanes.  frames() solves the eigenproblem with numpy's eigh (the library: cyclic Jacobi) and reports, per query, what a
comparison needs to know about its conditioning; sums() takes the frames it is given (the GPU's own f32 frames in the GPU tests)
and returns the fixed-point sums S of rule H7 as exact integers; rows_from_sums() is rule H8."""
import numpy as np

from outlier_ref import d2_f32

F32, F64, U64 = np.float32, np.float64, np.uint64
DIM, SHAPE, VOLUMES, MIN_NEIGHBORS = 352, 11, 32, 5
ONE = 4294967296.0                       # 2^32: one unit of an amount
# pcl/features/shot.h
RAD45, RAD90, RAD135, RAD7_8 = 0.78539816339744830961566084581988, 1.5707963267948966192313216916398, \
    2.3561944901923449288469825374596, 2.7488935718910690836548129603691


def pairs(points, queries, radius, valid, fma=False, chunk=400):
    """(qi, pj) of every pair with f32 d2 <= (float)(R * R) and valid[pj], query-major; a non-finite query has none"""
    P, Q = np.asarray(points)[:, :3], np.asarray(queries)[:, :3]
    r2 = F32(min(float(radius) * float(radius), float(np.finfo(F32).max)))
    P32, Q32 = P.astype(F32), Q.astype(F32)
    cand = np.nonzero(valid)[0]
    qi, pj = [], []
    for c0 in range(0, len(Q), chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            inside = d2_f32(Q32[c0:c0 + chunk, None, :], P32[None, cand, :], fma) <= r2
        a, b = np.nonzero(inside)
        qi.append(a + c0)
        pj.append(cand[b])
    if not qi:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(qi).astype(np.int64), np.concatenate(pj).astype(np.int64)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def frames(points, queries, radius, fma=False):
    """rules L1-L6 for every query: dict(axes [nq, 3, 3] f64 rows x, y, z -- NaN where the rules give NaN --, n [nq],
    gap [nq] = min(l1 - l0, l2 - l1) / l2, margin [nq, 2] = |2 plus - n| for x and z, near [nq, 2] = the neighbours with
    |v . a| <= 1e-9 |v|, tie_s [nq, 2] = the sum of w (v . a) that decides a tie)"""
    P, Q = np.asarray(points)[:, :3].astype(F64), np.asarray(queries)[:, :3].astype(F64)
    nq, R = len(Q), float(radius)
    valid = np.isfinite(P).all(1)
    qi, pj = pairs(points, queries, radius, valid, fma)
    away = (P[pj] != Q[qi]).any(1)                                        # L2: a surface point AT the query is skipped, as in PCL
    qi, pj = qi[away], pj[away]
    n = np.bincount(qi, minlength=nq)
    v = P[pj] - Q[qi]
    d = np.sqrt(_dot(v[:, 0], v[:, 1], v[:, 2], v[:, 0], v[:, 1], v[:, 2]))
    w = R - d
    acc = lambda x: np.bincount(qi, weights=x, minlength=nq)
    W = acc(w)
    M = np.zeros((nq, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            M[:, a, b] = M[:, b, a] = acc(w * v[:, a] * v[:, b])
    ok = (n >= MIN_NEIGHBORS) & (W != 0) & np.isfinite(W) & np.isfinite(M).all((1, 2)) & np.isfinite(Q).all(1)
    axes = np.full((nq, 3, 3), np.nan)
    gap = np.zeros(nq)
    margin, near, tie_s = np.zeros((nq, 2), np.int64), np.zeros((nq, 2), np.int64), np.zeros((nq, 2))
    if ok.any():
        lam, vec = np.linalg.eigh(M[ok] / W[ok, None, None])          # ascending
        x0, z0 = np.full((nq, 3), np.nan), np.full((nq, 3), np.nan)
        x0[ok], z0[ok] = vec[:, :, 2], vec[:, :, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap[ok] = np.minimum(lam[:, 1] - lam[:, 0], lam[:, 2] - lam[:, 1]) / lam[:, 2]
        for c, a in enumerate((x0, z0)):
            dots = _dot(v[:, 0], v[:, 1], v[:, 2], a[qi, 0], a[qi, 1], a[qi, 2])
            plus = np.bincount(qi, weights=(dots >= 0), minlength=nq).astype(np.int64)
            margin[:, c] = np.abs(2 * plus - n)
            near[:, c] = np.bincount(qi, weights=(np.abs(dots) <= 1e-9 * d), minlength=nq).astype(np.int64)
            tie_s[:, c] = acc(w * np.where(np.isfinite(dots), dots, 0.0))
            neg = (2 * plus < n) | ((2 * plus == n) & (tie_s[:, c] < 0))
            a[neg] = -a[neg]
        axes[:, 0], axes[:, 2] = x0, z0
        axes[:, 1] = np.cross(z0, x0)
    axes[~ok] = np.nan
    return dict(axes=axes, n=n, gap=gap, margin=margin, near=near, tie_s=tie_s, ok=ok)


def sector_h5(x, y):
    """the sector as rule H5 words it: s = min(7, floor((atan2(y, x) + pi) / (pi / 4))); x == y == 0: 0"""
    s = np.minimum(7, np.floor((np.arctan2(y, x) + np.pi) / (np.pi / 4))).astype(np.int64)
    return np.where((x == 0) & (y == 0), 0, s)


def sector_pcl(x, y):
    """the sector as pcl/features/impl/shot.hpp selects it (desc_index >> 2 before the husk and the half are added)"""
    bit4 = ((y > 0) | ((y == 0) & (x < 0))).astype(np.int64)
    bit3 = np.where((x > 0) | ((x == 0) & (y > 0)), 1 - bit4, bit4)
    di = ((bit4 << 3) + (bit3 << 2)) << 1
    first = (x * y > 0) | (x == 0)
    di = di + np.where(first, np.where(np.abs(x) >= np.abs(y), 0, 4), np.where(np.abs(x) > np.abs(y), 4, 0))
    return di >> 2


def fix(w):
    """H7: floor(w 2^32 + 0.5) of a non-negative amount as an exact integer; a negative rounding and a NaN give 0"""
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, np.floor(w * ONE + 0.5), 0.0).astype(U64)


def sums(points, normals, queries, frames32, radius, fma=False):
    """rules H1-H7: (S [nq, 352] uint64, n [nq], contributors [nq], on_axis [nq]) -- n the valid neighbours, contributors those
    that add amounts (d != 0, finite c), on_axis those of them with x == y == 0.  A query whose frame holds a NaN gets zeros and
    n = 0.  The rule n < 5 is the caller's (rows_from_sums)."""
    P, N = np.asarray(points)[:, :3].astype(F64), np.asarray(normals)[:, :3].astype(F64)
    Q, Fm = np.asarray(queries)[:, :3].astype(F64), np.asarray(frames32).reshape(-1, 9).astype(F64)
    nq, R = len(Q), float(radius)
    R12, R14, R34 = R / 2.0, R / 4.0, (R * 3.0) / 4.0
    valid = np.isfinite(P).all(1) & np.isfinite(N).all(1)
    qi, pj = pairs(points, queries, radius, valid, fma)
    keep = np.isfinite(Fm).all(1)[qi]
    qi, pj = qi[keep], pj[keep]
    n = np.bincount(qi, minlength=nq)
    S = np.zeros(nq * DIM, U64)
    v = P[pj] - Q[qi]
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    d = np.sqrt(_dot(vx, vy, vz, vx, vy, vz))
    f = Fm[qi]
    c = _dot(N[pj, 0], N[pj, 1], N[pj, 2], f[:, 6], f[:, 7], f[:, 8])
    live = (d != 0) & np.isfinite(c)
    c = np.clip(c, -1.0, 1.0)
    x, y, z = (_dot(vx, vy, vz, f[:, 3 * a], f[:, 3 * a + 1], f[:, 3 * a + 2]) for a in range(3))
    x, y, z = (np.where(np.abs(t) < 1e-30, 0.0, t) for t in (x, y, z))
    sector = sector_pcl(x, y)
    outer = d > R12
    vol = 4 * sector + 2 * outer + (z > 0)
    bin_ = ((1.0 + c) * 10.0) / 2.0
    step = np.floor(bin_ + 0.5).astype(np.int64)
    t = bin_ - step

    def put(mask, volume, k, w):
        m = mask & live
        slot = (SHAPE * volume + k)[m]
        assert ((slot >= 0) & (slot < DIM)).all()
        np.add.at(S, qi[m] * DIM + slot, fix(w[m]))

    with np.errstate(invalid="ignore", divide="ignore"):
        home = 1.0 - np.abs(t)                                            # (a)
        put(t > 0, vol, (step + 1) % 10, t)
        put(t < 0, vol, (step + 9) % 10, -t)
        uo, ui = (d - R34) / R12, (d - R14) / R12                         # (b)
        far, close = outer & (d > R34), ~outer & (d < R14)
        home = home + np.where(outer, np.where(far, 1.0 - uo, 1.0 + uo), np.where(close, 1.0 + ui, 1.0 - ui))
        put(outer & ~far, vol - 2, step, -uo)
        put(~outer & ~close, vol + 2, step, ui)
        inc = np.arccos(np.clip(z / d, -1.0, 1.0))                        # (c)
        lower = (inc > RAD90) | ((np.abs(inc - RAD90) < 1e-30) & (z <= 0))
        ul, uu = (inc - RAD135) / RAD90, (inc - RAD45) / RAD90
        low, high = lower & (inc > RAD135), ~lower & (inc < RAD45)
        home = home + np.where(lower, np.where(low, 1.0 - ul, 1.0 + ul), np.where(high, 1.0 + uu, 1.0 - uu))
        put(lower & ~low, vol + 1, step, -ul)
        put(~lower & ~high, vol - 1, step, uu)
        planar = (x != 0) | (y != 0)                                      # (d)
        ua = np.clip((np.arctan2(y, x) - (-RAD7_8 + RAD45 * sector)) / RAD45, -0.5, 0.5)
        home = home + np.where(planar, 1.0 - np.abs(ua), 0.0)
        put(planar & (ua > 0), (vol + 4) % VOLUMES, step, ua)
        put(planar & ~(ua > 0), (vol + 28) % VOLUMES, step, -ua)
        put(np.ones(len(qi), bool), vol, step, home)                      # (e)
    contributors = np.bincount(qi[live], minlength=nq)
    on_axis = np.bincount(qi[live & ~planar], minlength=nq)
    return S.reshape(nq, DIM), n, contributors, on_axis


def rows_from_sums(S, n, valid):
    """H8 on returned sums: the f32 rows, NaN for an invalid query, n < 5 and norm == 0; the norm adds in ascending b"""
    S64 = np.asarray(S).astype(F64)
    norm2 = np.zeros(len(S64))
    for b in range(S64.shape[1]):
        norm2 = norm2 + S64[:, b] * S64[:, b]
    norm = np.sqrt(norm2)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (S64 / norm[:, None]).astype(F32)
    out[~(np.asarray(valid, bool) & (np.asarray(n) >= MIN_NEIGHBORS) & (norm != 0))] = np.nan
    return out
