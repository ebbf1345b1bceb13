"""references for the ICP sum kernels of csrc/mvr_reduce.hip (tests/test_sum_cases_host.py, tests/test_gpu_sums.py):
  exact_*   plain integer arithmetic on integral input (asserted) -- what the f64 sums must equal bit for bit when every partial
            sum is below 2^53;
  fsum_*    for real-valued f32 points: the terms formed as the kernels define them ((double)p - o, then f64 products; the build
            uses -ffp-contract=off, so numpy's products are the kernel's terms bit for bit), every column summed by math.fsum
            (exactly rounded), with the sum of the terms' absolute values beside it;
  fake_sums a numpy model of the reduction itself -- lane accumulators in the kernels' stride order (the walk of kUn = 3 queries
            per trip adds k, k + stride, k + 2 stride in that order, as a one-at-a-time walk does), the wave sum of 4 rows of 16
            lanes, 4 waves, the partial rows, the final sum in 8 row groups -- with switchable faults.  It exists only so that
            the CPU test can show which of the sizes of tests/sum_cases.py catches which fault.

Column order of the 29 moment sums: n, sum p (3), sum q (3), sum pp (xx xy xz yy yz zz), sum qq (6), sum pq (9: p_r q_c,
row-major), sum d2.  Of the 29 point-to-plane sums: the upper triangle of sum a a^T (21, row-major), sum a d (6), the count,
sum d^2, with a = [p x n, n] and d = n.(q - p) in the kernel's operation order."""
import math
from fractions import Fraction

import numpy as np

TRI = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
KRT, KUN, GROUPS, MAX_BLOCKS = 256, 3, 8, 1024
FAULTS = ("last_lane_of_partial_wave", "third_query_at_the_end", "rows_from_8", "range_starts_one_late", "cap_is_a_miss")


def _integral(*arrays):
    for a in arrays:
        a = np.asarray(a, np.float64)
        assert np.isfinite(a).all() and np.array_equal(a, np.rint(a)), "exact_*: input is not integral"


def _i64(a):
    return np.rint(np.asarray(a, np.float64)).astype(np.int64)


def moment_terms(p, q, d2, origin):
    """(m, 29) float64: the terms moments2_kernel / accept_moments2_body add for each correspondence"""
    o = np.asarray(origin, np.float64)
    p, q = np.asarray(p, np.float32)[:, :3].astype(np.float64) - o, np.asarray(q, np.float32)[:, :3].astype(np.float64) - o
    cols = [np.ones(len(p))] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)]
    cols += [p[:, a] * p[:, b] for a, b in TRI] + [q[:, a] * q[:, b] for a, b in TRI]
    cols += [p[:, a] * q[:, b] for a in range(3) for b in range(3)] + [np.asarray(d2, np.float32).astype(np.float64)]
    return np.stack(cols, 1) if len(p) else np.zeros((0, 29))


def exact_sums(p, q, d2, origin):
    """the 29 moment sums as int64; refuses input that is not integral.  (sum_cases.int_sums adds the same columns from the
    construction's int64 arrays; the two are kept apart on purpose -- the case module must not depend on the reference it is
    checked with -- and the host test compares them on every case)"""
    _integral(np.asarray(p)[:, :3], np.asarray(q)[:, :3], d2, origin)
    o = _i64(origin)
    p, q = _i64(np.asarray(p)[:, :3]) - o, _i64(np.asarray(q)[:, :3]) - o
    out = [len(p)] + [p[:, a].sum() for a in range(3)] + [q[:, a].sum() for a in range(3)]
    out += [(p[:, a] * p[:, b]).sum() for a, b in TRI] + [(q[:, a] * q[:, b]).sum() for a, b in TRI]
    out += [(p[:, a] * q[:, b]).sum() for a in range(3) for b in range(3)] + [_i64(d2).sum()]
    return np.array([int(v) for v in out], np.int64)


def fsum_columns(terms):
    """-> (exactly rounded column sums, column sums of the absolute values)"""
    t = np.asarray(terms, np.float64)
    return (np.array([math.fsum(t[:, k]) for k in range(t.shape[1])]), np.array([math.fsum(np.abs(t[:, k])) for k in range(t.shape[1])]))


def fsum_sums(p, q, d2, origin):
    return fsum_columns(moment_terms(p, q, d2, origin))


def abs_sums(p, q, d2, origin):
    """the column sums of |terms| (for the proof that every partial sum stays below 2^53)"""
    return np.abs(moment_terms(p, q, d2, origin)).sum(0)


# ---- pass2_kernel: the 9 centred products sum (q - mq)_r (p - mp)_c about the means pass1_final_kernel leaves, float(sum) / float(n)
def means(p, q):
    """-> (mp, mq): one correctly rounded division of the exactly rounded sums (of exact integers on a lattice)"""
    p, q = np.asarray(p, np.float32)[:, :3].astype(np.float64), np.asarray(q, np.float32)[:, :3].astype(np.float64)
    n = float(len(p))
    return (np.array([math.fsum(p[:, a]) / n for a in range(3)]), np.array([math.fsum(q[:, a]) / n for a in range(3)]))


def centred_terms(p, q, mp, mq):
    p, q = np.asarray(p, np.float32)[:, :3].astype(np.float64) - mp, np.asarray(q, np.float32)[:, :3].astype(np.float64) - mq
    return np.stack([q[:, r] * p[:, c] for r in range(3) for c in range(3)], 1), p, q


def fsum_centred(p, q):
    """-> (sums[9], abs[9], mp, mq, sum |p - mp| (3), sum |q - mq| (3)) about the rounded means"""
    mp, mq = means(p, q)
    t, pc, qc = centred_terms(p, q, mp, mq)
    s, a = fsum_columns(t)
    return s, a, mp, mq, np.abs(pc).sum(0), np.abs(qc).sum(0)


def exact_centred(p, q):
    """the 9 centred sums about the EXACT means, as Fractions: sum q_r p_c - sum q_r sum p_c / n"""
    _integral(np.asarray(p)[:, :3], np.asarray(q)[:, :3])
    p, q = _i64(np.asarray(p)[:, :3]), _i64(np.asarray(q)[:, :3])
    n = len(p)
    return [Fraction(int((q[:, r] * p[:, c]).sum())) - Fraction(int(q[:, r].sum()) * int(p[:, c].sum()), n) for r in range(3) for c in range(3)]


# ---- p2plane_kernel
def plane_terms(p, q, nrm):
    p, q, n = (np.asarray(x, np.float32)[:, :3].astype(np.float64) for x in (p, q, nrm))
    sx, sy, sz, nx, ny, nz = p[:, 0], p[:, 1], p[:, 2], n[:, 0], n[:, 1], n[:, 2]
    a = [nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz]
    d = nx * q[:, 0] + ny * q[:, 1] + nz * q[:, 2] - nx * sx - ny * sy - nz * sz
    cols = [a[r] * a[c] for r in range(6) for c in range(r, 6)] + [a[r] * d for r in range(6)] + [np.ones(len(p)), d * d]
    return np.stack(cols, 1) if len(p) else np.zeros((0, 29))


def fsum_plane(p, q, nrm):
    return fsum_columns(plane_terms(p, q, nrm))


def exact_plane(p, q, nrm):
    _integral(np.asarray(p)[:, :3], np.asarray(q)[:, :3], np.asarray(nrm)[:, :3])
    p, q, n = (_i64(np.asarray(x)[:, :3]) for x in (p, q, nrm))
    a = np.concatenate([np.cross(p, n), n], 1)
    d = (n * (q - p)).sum(1)
    out = [(a[:, r] * a[:, c]).sum() for r in range(6) for c in range(r, 6)] + [(a[:, r] * d).sum() for r in range(6)] + [len(p), (d * d).sum()]
    return np.array([int(v) for v in out], np.int64)


def plane_system(sums):
    """the 29 sums -> (A^T A (6, 6), A^T b (6)) as lists of Python ints / floats"""
    A = [[0] * 6 for _ in range(6)]
    t = 0
    for r in range(6):
        for c in range(r, 6):
            A[r][c] = A[c][r] = sums[t]
            t += 1
    return A, [sums[21 + r] for r in range(6)]


def solve_rational(A, b):
    """Gauss-Jordan in Fractions -> x, or None when A is singular"""
    n = len(b)
    M = [[Fraction(int(v)) for v in row] + [Fraction(int(b[i]))] for i, row in enumerate(A)]
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c] != 0), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b_ for a, b_ in zip(M[r], M[c])]
    return [M[r][n] for r in range(n)]


def pcl_matrix(x):
    """PCL's constructTransformationMatrix(alpha, beta, gamma, tx, ty, tz) in f64"""
    al, be, ga, tx, ty, tz = (float(v) for v in x)
    sa, ca, sb, cb, sg, cg = math.sin(al), math.cos(al), math.sin(be), math.cos(be), math.sin(ga), math.cos(ga)
    return np.array([[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca, tx],
                     [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca, ty],
                     [-sb, cb * sa, cb * ca, tz], [0.0, 0.0, 0.0, 1.0]])


# ---- fitness_kernel
def exact_fitness(d2, max_range):
    """-> (sum of the d2 <= max_range, their count) in integers"""
    _integral(d2)
    d = _i64(d2)
    keep = d.astype(np.float64) <= max_range
    return int(d[keep].sum()), int(keep.sum())


def fsum_fitness(d2, max_range):
    d = np.asarray(d2, np.float32).astype(np.float64)
    keep = d <= max_range
    return math.fsum(d[keep]), int(keep.sum()), math.fsum(np.abs(d[keep]))


# ---- the fake reduction
def moments_blocks(n, n_cu, reduce_rows=0):
    cap = reduce_rows if reduce_rows > 0 else max(32, n_cu // 4)
    return max(1, min((n + KRT - 1) // KRT, MAX_BLOCKS, cap))


def reduce_blocks(n, n_cu):
    return max(1, min((n + KRT - 1) // KRT, MAX_BLOCKS, n_cu))


def wave_sum(v):
    """v: (..., 64, K) -> (..., K): an inclusive scan inside each row of 16 lanes by shifts of 1, 2, 4, 8 (lanes from outside the
    row read as 0), then lanes 15, 31, 47, 63 added in order"""
    v = v.reshape(v.shape[:-2] + (4, 16, v.shape[-1])).copy()
    for s in (1, 2, 4, 8):
        old = v.copy()
        v[..., s:, :] += old[..., :-s, :]
    r = v[..., 15, :]
    return ((r[..., 0, :] + r[..., 1, :]) + r[..., 2, :]) + r[..., 3, :]


def fake_sums(src, tgt, match, d2, rec_ok, max2, origin, q_begin, q_count, blocks, fault=None):
    """accept_moments2_kernel + moments2_final_kernel in numpy.  src, tgt: (n, >= 3) points; match[i] / d2[i]: query i's forward
    neighbour (-1: none) and its f32 squared distance; rec_ok[i] (or None): what the reverse test says of query i.  fault: one of
    FAULTS, or None."""
    assert fault is None or fault in FAULTS
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    match, d2 = np.asarray(match, np.int64), np.asarray(d2, np.float64)
    stride = blocks * KRT
    trips = max(1, -(-q_count // stride))
    k = np.arange(trips * stride)
    live = k < q_count
    if fault == "range_starts_one_late":
        live &= k != 0
    if fault == "third_query_at_the_end":                                   # u = 2 of a trip, and the last query of the range
        live &= ~(((k // stride) % KUN == 2) & (k == q_count - 1))
    i = np.minimum(q_begin + k, len(src) - 1)
    j = match[i]
    ok = live & (j >= 0) & ((d2[i] < max2) if fault == "cap_is_a_miss" else ~(d2[i] > max2))
    if rec_ok is not None:
        ok &= np.asarray(rec_ok, bool)[i]
    terms = np.zeros((trips * stride, 29))
    terms[ok] = moment_terms(src[i[ok]], tgt[j[ok]], d2[i[ok]].astype(np.float32), origin)
    acc = np.zeros((stride, 29))
    for t in range(trips):                                                  # a lane adds its queries k0, k0 + stride, ... in order
        acc += terms[t * stride:(t + 1) * stride]
    acc = acc.reshape(blocks, KRT // 64, 64, 29)
    if fault == "last_lane_of_partial_wave":
        first = (np.arange(stride) < q_count).reshape(blocks, KRT // 64, 64)  # lanes with a query in the first trip
        cnt = first.sum(2)
        for b, w in zip(*np.nonzero((cnt > 0) & (cnt < 64))):
            acc[b, w, cnt[b, w] - 1] = 0.0
    waves = wave_sum(acc)                                                    # (blocks, 4, 29)
    rows = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]         # (blocks, 29): the partial rows
    grp = np.zeros((GROUPS, 29))
    for r in range(blocks):
        if fault == "rows_from_8" and r >= GROUPS:
            break
        grp[r % GROUPS] += rows[r]
    out = grp[0].copy()
    for g in range(1, GROUPS):
        out = out + grp[g]
    return out


# ---- the point-to-plane solve from the exact sums
def ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def plane_expectation(p, q, nrm):
    """the exact normal equations of the list, solved in rationals -> (PCL's matrix in f64 rounded to f32, the allowed difference per
    entry, cond(A^T A), x).  Allowance: one f32 ulp of the entry (its rounding, and a last-place difference of the f64 value before
    it) plus 8 cond(A^T A) 2^-52 times the entry's scale: 1 for the entries of the rotation block (sines and cosines), the largest
    |translation| for the three translation entries."""
    A, b = plane_system([int(v) for v in exact_plane(p, q, nrm)])
    x = solve_rational(A, b)
    if x is None:
        return None
    cond = float(np.linalg.cond(np.array(A, np.float64)))
    M = pcl_matrix(x)
    T = M.astype(np.float32)
    scale = np.ones((4, 4))
    scale[:3, 3] = np.abs(M[:3, 3]).max()
    allow = ulp32(M) + 8.0 * cond * 2.0 ** -52 * scale
    allow[3] = 0.0
    return T, allow, cond, x


# ---- rigid fits of degenerate lists
def kabsch(p, q):
    """numpy's least-squares rotation with the determinant correction -> (R, t, residual sum |R p + t - q|^2)"""
    p, q = np.asarray(p, np.float64)[:, :3], np.asarray(q, np.float64)[:, :3]
    mp, mq = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((p - mp).T @ (q - mq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    t = mq - R @ mp
    return R, t, float((((p @ R.T + t) - q) ** 2).sum())


def check_rigid_fit(T, p, q, what=""):
    """T (4, 4) float32 from umeyama_from_moments on the list p -> q: finite, a rotation within the f32 rounding of its entries, and
    a residual no worse than Kabsch's by more than that rounding allows.  Rounding an entry to f32 moves it by at most 2^-24 of its
    size (<= 1 for R): R^T R and det R, sums of 3 and 6 products of such entries, move by at most 6 x 2^-24 and 6 x 2^-24 (+ 1e-12 for
    the f64 arithmetic before the rounding); a posed coordinate moves by at most e = 2^-24 (|px| + |py| + |pz| + |t|), so a point's
    residual vector r by a vector of length <= sqrt(3) e and its square by <= 2 |r| sqrt(3) e + 3 e^2."""
    T = np.asarray(T, np.float64)
    p, q = np.asarray(p, np.float64)[:, :3], np.asarray(q, np.float64)[:, :3]
    assert np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1]), what
    R, t = T[:3, :3], T[:3, 3]
    tol = 6 * 2.0 ** -24 + 1e-12
    assert np.abs(R.T @ R - np.eye(3)).max() <= tol and abs(np.linalg.det(R) - 1.0) <= tol, (what, R)
    r = (p @ R.T + t) - q
    got = float((r ** 2).sum())
    Rk, tk, best = kabsch(p, q)
    rk = np.linalg.norm((p @ Rk.T + tk) - q, axis=1)
    e = 2.0 ** -24 * (np.abs(p).sum(1) + np.abs(t).max())
    allow = float((2 * rk * np.sqrt(3) * e + 3 * e * e).sum()) + 1e-9 * max(best, 1e-12)
    print("%s: residual %.6g, Kabsch %.6g, allowed excess %.3g" % (what, got, best, allow))
    assert got - best <= allow, (what, got, best, allow)
    return got, best, allow
