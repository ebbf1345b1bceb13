"""shared inputs of the tests of the ICP sum kernels (tests/test_sum_cases_host.py on the CPU, tests/test_gpu_sums.py on the GPU):
lattice pairs whose accepted correspondences and whose 29 sums are known BY CONSTRUCTION, in integers.

A case is a target, a source and a search distance of MAX_DIST = 4:
  target  the points g * PITCH + frame for g in a box of `dims` (PITCH = 8), stored in a seeded random order;
  source  `plain` points: a seeded subset of the targets, each moved by an integer offset from {-2..2}^3, so d2 <= 12 against
          (8 - 2)^2 = 36 or more to any other target -- forward and reverse neighbours are unambiguous;
          `rival`: a second source point on an already matched target, at (3, 2, 1) (d2 = 14, 30 to the next target): the one-way
          filter keeps both, the reciprocal filter the nearer (plain) one;
          `equal`: on a matched target with offset off != 0, the mirrored point at -off (the same d2): the reverse search's
          lowest-index rule decides, so the reciprocal filter keeps the one stored first (case["equal_winners"]);
          `orphan`: points 1000 units and more outside the lattice: no match within MAX_DIST;
          `edge`: on the outer face g_x = 0, on a target no other source point uses, offset 4 straight outwards: d2 = 16 =
          MAX_DIST^2, accepted in both modes (the rule is !(d2 > max2)), and never between two targets;
          all stored in a seeded random order.
Every coordinate is an integer below 2^24, so it is held exactly in f32, and every term of the 29 sums about an integer origin
is an integer; the host test proves that every partial sum stays below 2^53, so the f64 sums are the integers in any order.

Frames: "near" = frame and origin (0, 0, 896); "far" = frame and origin (610000, -520000, 600896); "far0" = the far frame with
the origin (0, 0, 0), at no more than 4 097 source points (at 16 370 the sum of the absolute terms is 6.1e15 of 2^53 = 9.0e15).

Source sizes (q_count) answer to the launch shapes of csrc/mvr_reduce.hip and csrc/mvr_block_sums.h: blocks of 256 threads (four
waves of 64), at most R = max(32, n_cu / 4) partial rows for the 29-sum family (moments_blocks) and n_cu for the others
(reduce_blocks), a walk of kUn = 3 queries per lane and trip, a final sum in 8 row groups.  SIZES names them; tests/sum_ref.py's
fake reduction and tests/test_sum_cases_host.py show which injected fault each one catches."""
import numpy as np

F32 = np.float32
PITCH = 8
MAX_DIST = 4.0
N_CU = 256                                              # an MI355X; the GPU test passes the device's own count
FRAMES = {"near": ((0, 0, 896), (0, 0, 896)), "far": ((610000, -520000, 600896), (610000, -520000, 600896)),
          "far0": ((610000, -520000, 600896), (0, 0, 0))}
SMALL, MID, BIG = (6, 5, 4), (48, 48, 32), (64, 64, 64)
PLAIN, RIVAL, EQUAL, ORPHAN, EDGE = 0, 1, 2, 3, 4
FAR0_MAX = 4097
_cases = {}


def row_cap(n_cu=N_CU):
    """moments_blocks' cap on the partial rows"""
    return max(32, int(n_cu) // 4)


def sizes(n_cu=N_CU):
    """name -> q_count.  "all_rows" (the 64^3 box) fills all kMaxBlocks = 1024 rows under reduce_rows = 1024; "empty" is orphans only."""
    R = row_cap(n_cu)
    s = {str(n): n for n in (1, 2, 3, 63, 64, 65, 255, 256, 257)}
    s.update({"rowcap-1": 256 * R - 1, "rowcap": 256 * R, "rowcap+1": 256 * R + 1, "2stride+1": 2 * 256 * R + 1,
              "walk-1": 3 * 256 * R - 1, "walk+1": 3 * 256 * R + 1, "blockcap": 256 * int(n_cu) + 257, "all_rows": 1024 * 256 - 255, "empty": 65})
    return s


SMALL_NAMES = ("1", "2", "3", "63", "64", "65", "255", "256", "257")
LARGE_NAMES = ("rowcap-1", "rowcap", "rowcap+1", "2stride+1", "walk-1", "walk+1", "blockcap")
NAMES = SMALL_NAMES + LARGE_NAMES + ("all_rows", "empty")
FAR0_NAMES = ("65", "257", "4097")


def _kinds(n, orphans_only):
    if orphans_only:
        return dict(plain=0, rival=0, equal=0, orphan=n, edge=0)
    if n < 4:
        return dict(plain=1, rival=int(n == 3), equal=0, orphan=int(n >= 2), edge=0)
    assert n >= 16
    return dict(plain=n - 10, rival=3, equal=2, orphan=3, edge=2)


def build(dims, n_src, frame, origin, seed, orphans_only=False):
    rng = np.random.default_rng(seed)
    frame, origin = np.asarray(frame, np.int64), np.asarray(origin, np.int64)
    nt = int(np.prod(dims))
    g = np.stack(np.unravel_index(np.arange(nt), dims), 1).astype(np.int64)
    g = g[rng.permutation(nt)]                                             # stored order is not spatial order
    tgt = g * PITCH + frame
    k = _kinds(n_src, orphans_only)
    face = np.nonzero(g[:, 0] == 0)[0]
    edge_t = rng.choice(face, k["edge"], replace=False)
    pool = np.setdiff1d(np.arange(nt), edge_t)
    assert k["plain"] <= len(pool), (dims, n_src)
    plain_t = rng.choice(pool, k["plain"], replace=False)
    off = rng.integers(-2, 3, (k["plain"], 3))
    eq = np.arange(k["rival"], k["rival"] + k["equal"])                    # rivals sit on the first plain hosts, mirrors on the next
    off[eq[(off[eq] == 0).all(1)]] = (1, 0, -2)
    pts = [tgt[plain_t] + off, tgt[plain_t[:k["rival"]]] + (3, 2, 1), tgt[plain_t[eq]] - off[eq],
           frame + np.stack([-1000 - 16 * np.arange(k["orphan"]), np.full(k["orphan"], -1000), np.full(k["orphan"], -1000)], 1),
           tgt[edge_t] + (-4, 0, 0)]
    host = np.concatenate([plain_t, plain_t[:k["rival"]], plain_t[eq], np.full(k["orphan"], -1), edge_t]).astype(np.int64)
    kind = np.concatenate([np.full(len(p), c) for p, c in zip(pts, (PLAIN, RIVAL, EQUAL, ORPHAN, EDGE))])
    pts = np.concatenate(pts).astype(np.int64)
    assert len(pts) == n_src
    sperm = rng.permutation(n_src)                                         # stored position i holds constructed row sperm[i]
    pos = np.empty(n_src, np.int64)
    pos[sperm] = np.arange(n_src)
    src, host, kind = pts[sperm], host[sperm], kind[sperm]
    d2 = np.where(host >= 0, ((src - tgt[np.maximum(host, 0)]) ** 2).sum(1), -1)
    one_way = host >= 0
    recip = one_way & (kind != RIVAL)
    winners = []
    for j, e in enumerate(eq):                                             # the plain point and its mirror: the lower stored index wins
        a, b = int(pos[e]), int(pos[k["plain"] + k["rival"] + j])
        recip[max(a, b)] = False
        winners.append((int(plain_t[e]), min(a, b), max(a, b)))
    assert np.abs(src).max() < 2 ** 24 and np.abs(tgt).max() < 2 ** 24

    def cloud(x):
        out = np.ones((len(x), 4), F32)
        out[:, :3] = x
        assert np.array_equal(out[:, :3].astype(np.int64), x)
        return out

    c = dict(dims=dims, src=cloud(src), tgt=cloud(tgt), src_int=src, tgt_int=tgt, origin=origin.astype(np.float64), origin_int=origin,
             max_dist=MAX_DIST, kind=kind, host=host, d2_int=d2, equal_winners=winners, accepted={}, sums={})
    for rec, keep in ((False, one_way), (True, recip)):
        q = np.nonzero(keep)[0]
        c["accepted"][rec] = (q.astype(np.int32), host[q].astype(np.int32), d2[q].astype(F32))
        c["sums"][rec] = int_sums(src[q], tgt[host[q]], d2[q], origin)
    return c


def int_sums(p, q, d2, origin):
    """n, sum p (3), sum q (3), sum pp (xx xy xz yy yz zz), sum qq (6), sum pq (9, p_r q_c row-major), sum d2 -- int64, about origin.
    (independent of sum_ref.exact_sums on purpose: tests/test_sum_cases_host.py compares the two on every case)"""
    p, q = np.asarray(p, np.int64) - origin, np.asarray(q, np.int64) - origin
    tri = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    out = [len(p)] + [p[:, a].sum() for a in range(3)] + [q[:, a].sum() for a in range(3)]
    out += [(p[:, a] * p[:, b]).sum() for a, b in tri] + [(q[:, a] * q[:, b]).sum() for a, b in tri]
    out += [(p[:, a] * q[:, b]).sum() for a in range(3) for b in range(3)] + [np.asarray(d2, np.int64).sum()]
    return np.array([int(v) for v in out], np.int64)


def case(name, frame="near", n_cu=N_CU):
    key = (name, frame, int(n_cu))
    if key not in _cases:
        n = int(name) if name.isdigit() else sizes(n_cu)[name]
        assert frame != "far0" or n <= FAR0_MAX
        dims = BIG if name == "all_rows" else (SMALL if n <= 65 else MID)
        fr, org = FRAMES[frame]
        seed = 7000 + 31 * (list(NAMES).index(name) if name in NAMES else 97) + list(FRAMES).index(frame)
        _cases[key] = build(dims, n, fr, org, seed, orphans_only=(name == "empty"))
    return _cases[key]


def ring_views(n_cu=N_CU):
    """two sources (4 097 and 256 R + 1 points) on ONE lattice target (the same seed draws the same target order), the three views
    of the ring test: view 0 = the target, views 1 and 2 = the sources"""
    key = ("ring", int(n_cu))
    if key not in _cases:
        fr, org = FRAMES["near"]
        _cases[key] = tuple(build(MID, n, fr, org, 9100) for n in (4097, 256 * row_cap(n_cu) + 1))
        assert np.array_equal(_cases[key][0]["tgt_int"], _cases[key][1]["tgt_int"])
    return _cases[key]


def swapped(c, rec=True):
    """the pair (target, source): each matched target finds its nearest source point, which is the reciprocal pair read the other
    way round -- with or without the reciprocal filter (a target has at most one source point within MAX_DIST that is its nearest,
    the lower index on a tie, and that point's nearest target is the target itself).  -> (query, match, d2, sums)"""
    q, m, d = c["accepted"][True]
    o = np.argsort(m, kind="stable")
    return m[o], q[o], d[o], int_sums(c["tgt_int"][m[o]], c["src_int"][q[o]], c["d2_int"][q[o]], c["origin_int"])


def self_pair(c):
    """the pair (source, source): every point, orphans included, matches itself at d2 = 0 (no two source points coincide)"""
    n = len(c["src_int"])
    assert len(np.unique(c["src_int"], axis=0)) == n
    return np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.zeros(n, F32), int_sums(c["src_int"], c["src_int"], np.zeros(n, np.int64), c["origin_int"])


def quarter_turn(pivot):
    """(4, 4) float64: a quarter turn about z through the integer pivot, written with literal 0.0 and +-1.0"""
    px, py = float(pivot[0]), float(pivot[1])
    return np.array([[0.0, -1.0, 0.0, px + py], [1.0, 0.0, 0.0, py - px], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def translation(t):
    T = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    T[:3, 3] = t
    return T


def unposed(cloud, T):
    """the integer cloud that T (an exact pose of the two kinds above) takes onto `cloud`"""
    R, t = np.rint(T[:3, :3]).astype(np.int64), np.rint(T[:3, 3]).astype(np.int64)
    raw = (cloud[:, :3].astype(np.int64) - t) @ R                          # R^-1 = R^T, and (x - t) R = R^T (x - t) as rows
    out = np.ones((len(raw), 4), F32)
    out[:, :3] = raw
    assert np.array_equal(out[:, :3].astype(np.int64), raw) and np.array_equal(raw @ R.T + t, cloud[:, :3].astype(np.int64))
    return out


PLANE_NAMES = ("16", "65", "257", "blockcap")            # the point-to-plane sizes (3 correspondences cannot fill a 6 x 6 system: see the tests)


def axis_normals(nt):
    """unit normals +-e_x, +-e_y, +-e_z by target index: axis j % 3, sign by (j // 3) % 2"""
    j = np.arange(nt)
    out = np.zeros((nt, 4), F32)
    out[j, j % 3] = np.where((j // 3) % 2 == 0, 1.0, -1.0)
    return out


def degenerate_lists():
    """name -> (src, tgt) clouds paired index by index, for svd3's rank-1 and rank-2 branches and the reflection case of Umeyama:
    integer points in the near frame, the target an exact rigid motion of the source unless the name says otherwise"""
    T = translation((5.0, -3.0, 2.0)) @ quarter_turn((24, 16))
    gx, gy = np.meshgrid(np.arange(7) * PITCH, np.arange(5) * PITCH)
    sheet = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 896)], 1)
    row = np.stack([np.arange(9) * PITCH, np.full(9, 16), np.full(9, 900)], 1)
    same = np.tile(np.array([[8, 24, 912]]), (6, 1))
    three = np.array([[0, 0, 896], [16, 8, 904], [8, 24, 888]])
    rng = np.random.default_rng(77)
    blob = rng.integers(-20, 21, (40, 3)) + (0, 0, 896)

    def cloud(x):
        out = np.ones((len(x), 4), F32)
        out[:, :3] = x
        return out

    def moved(x):
        return x @ np.rint(T[:3, :3]).astype(np.int64).T + np.rint(T[:3, 3]).astype(np.int64)
    out = {"sheet": (cloud(sheet), cloud(moved(sheet))), "row": (cloud(row), cloud(moved(row))), "identical": (cloud(same), cloud(moved(same))),
           "three": (cloud(three), cloud(moved(three) + np.array([[1, 0, -1], [0, 2, 0], [-1, -1, 1]]))),
           "mirrored": (cloud(blob), cloud(blob * (-1, 1, 1)))}
    return out
