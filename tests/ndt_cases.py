"""The clouds and parameters the NDT tests share (tests/test_ndt_host.py, tests/test_gpu_ndt.py, tests/test_gpu_ndt_cxx.py).
Every case is a dict(src, tgt float32 (n, 4); prm: keywords of ndt_ref.params / mvr.ndt_params; G: the guess or None;
truth: where the source's points belong, or None).  Lengths are millimetres."""
import functools

import numpy as np

import ndt_ref as R
from conftest import load_golden

P_STAR = np.array([1.0, -0.6, 0.5, 0.01, -0.008, 0.012])
ALIGN_PARAMS = {"res5": dict(resolution=5.0, step_size=1.0, transformation_epsilon=0.01),
                "res10": dict(resolution=10.0, step_size=2.0, transformation_epsilon=0.01)}


def cloud(xyz):
    p = np.ones((len(xyz), 4), np.float32)
    p[:, :3] = np.asarray(xyz, np.float32)
    return p


@functools.lru_cache(maxsize=None)
def _pair():
    t = load_golden("pair_2x10000.npz")["tgt"][:, :3].astype(np.float64)
    return t, np.round(t.mean(0))


def _moved(truth, p, origin):
    """the points that X(p) (about origin) takes to `truth`"""
    X = np.linalg.inv(R.pose_matrix(p, origin))
    return truth @ X[:3, :3].T + X[:3, 3]


def centred(which="res5"):
    t, c = _pair()
    tgt = cloud(t - c)
    truth = tgt[3::5, :3].astype(np.float64)
    return dict(name="centred-" + which, tgt=tgt, src=cloud(_moved(truth, P_STAR, np.zeros(3))), prm=dict(ALIGN_PARAMS[which]), G=None, truth=truth)


FAR = np.array([-10.0, 50.0, 870.0])      # the centroid to the nearest multiple of both resolutions: the voxels cut the cloud where `centred`'s do


def far(which="res5"):
    """`centred`'s clouds back where the scanner saw them, z about 900, rotating about the point `centred` rotates about.  The
    offset is a multiple of the resolution, so the lattice cuts the cloud into the same voxels; the f32 coordinates are coarser
    out here (ulp 6e-5), so the cells and the trace follow `centred`'s closely, not bit for bit."""
    case = centred(which)
    tgt = cloud(case["tgt"][:, :3].astype(np.float64) + FAR)
    truth = tgt[3::5, :3].astype(np.float64)
    prm = dict(ALIGN_PARAMS[which], origin=tuple(FAR))
    return dict(name="far-" + which, tgt=tgt, src=cloud(_moved(truth, P_STAR, FAR)), prm=prm, G=None, truth=truth)


def far_to_centred(X):
    """a pose of the far frame, seen from the centred frame"""
    A, B = np.eye(4), np.eye(4)
    A[:3, 3], B[:3, 3] = -FAR, FAR
    return A @ X @ B


def guess(which="res5"):
    case = centred(which)
    case.update(name="guess-" + which, G=R.pose_matrix(0.5 * P_STAR))
    return case


def align_cases():
    return [centred("res5"), centred("res10"), far("res5"), far("res10"), guess("res5"), guess("res10")]


# ---- one cell, one point: the branches of N7-N9 the clouds above do not reach
def one_cell(name, r0, **prm):
    """The target is `lattice`'s first cell, the corners (+-1)^3 about (2, 2, 2): C^-1 = (8 / 7) I.  The source is the one point
    (2 + r0, 2, 2) and the rotation turns about it, so the angle columns of J vanish, H is zero outside its translation block
    and the pose moves along x only: s(r) = -d1 exp(-d2 (8 / 7) r^2 / 2) while r <= 4 and the point's home voxel is the cell's
    or a neighbour of it, else nothing is counted."""
    corners = np.array([[a, b, c] for a in (-1.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)])
    point = (2.0 + r0, 2.0, 2.0)
    prm = dict(dict(resolution=4.0, min_points_per_voxel=8, transformation_epsilon=0.01, origin=point), **prm)
    return dict(name=name, tgt=cloud(corners + 2.0), src=cloud([point]), prm=prm, G=None, truth=np.array([[2.0, 2.0, 2.0]]))


FALLBACK_STEP = 5.0 - 2.0 ** -12


def branch_cases():
    """fallback*: the point sits beyond the inflection of the cell's Gaussian (r0 = 2.5 > sqrt(7 / (8 d2))), where H is positive:
    Newton's direction points away and is reversed, and the longest step overshoots the centre to r = -2.49976, a score
    above s(0) by less than the Armijo line asks: remembered, not accepted (both decisions 1.2e-4 |s(0)| from a tie).  With a
    second trial the half step lands 1.2e-4 from the centre and is accepted.  A step from there would gain 1e-9 |s(0)|, too
    near a tie to be a test, so fallback-2 has an epsilon above the half step and stops there on STEP.  flat*: at the centre
    g = 0.  iterations: `centred` cut short."""
    cut = centred("res5")
    cut["prm"]["max_iterations"] = 3
    cut["name"] = "iterations"
    return [one_cell("fallback", 2.5, step_size=FALLBACK_STEP, max_line_evals=1, max_iterations=1),
            one_cell("fallback-35", 2.5, step_size=FALLBACK_STEP, max_line_evals=1, max_iterations=35),
            one_cell("fallback-2", 2.5, step_size=FALLBACK_STEP, max_line_evals=2, max_iterations=35, transformation_epsilon=3.0),
            one_cell("flat-0", 0.0, step_size=1.0), one_cell("flat-1", 1.0, step_size=1.0, max_iterations=35), cut]


def residual(X, case):
    """the largest distance of a source point under X from where it belongs"""
    s = case["src"][:, :3].astype(np.float64)
    return float(np.linalg.norm(s @ X[:3, :3].T + X[:3, 3] - case["truth"], axis=1).max())


def all_align_cases():
    """every case an align test runs: together they reach every stop and both values of `reversed` and of `fallback`"""
    return align_cases() + branch_cases() + [disjoint()]


def branches(runs):
    """(stops, reversed flags, fallback flags) seen in a list of (stop, trace) runs"""
    return ({stop for stop, _ in runs}, {bool(t["reversed"]) for _, tr in runs for t in tr if t["trials"] > 0},
            {bool(t["fallback"]) for _, tr in runs for t in tr if t["a"] > 0})


EVERY_BRANCH = ({"STEP", "ITERATIONS", "FLAT", "NO_DECREASE", "NO_OVERLAP"}, {False, True}, {False, True})


# ---- exact arithmetic: points on a binary lattice
def lattice():
    """Resolution 4.  Each cell is the 8 corners (+-1)^3 about a centre on the lattice of voxel centres 4 Z^3 + 2: mean = the
    centre, sum (p - m)(p - m)^T = 8 I, C = (7 / 8)(1 / 8) 8 I = (7 / 8) I, C^-1 = (8 / 7) I, no eigenvalue inflated.  The
    source point (2, 2, 2) is exactly `resolution` away from the centres of its three axis neighbours: all counted
    (distance^2 == 16).  Under the pose `beyond`, a translation by -2^-50 along x (exact in f64: the f32 source could not
    carry it), the x-neighbour's centre is 4 + 2^-50 away, one f64 ulp beyond, and is not counted; nothing else changes."""
    centres = np.array([[2.0, 2.0, 2.0], [6.0, 2.0, 2.0], [2.0, 6.0, 2.0], [2.0, 2.0, 6.0], [10.0, 6.0, 6.0]])
    corners = np.array([[a, b, c] for a in (-1.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)])
    tgt = (centres[:, None, :] + corners[None, :, :]).reshape(-1, 3)
    src = np.array([[2.0, 2.0, 2.0], [2.5, 2.25, 1.75], [6.5, 2.5, 2.0], [9.0, 5.0, 7.0], [3.0, 3.0, 3.0]])
    prm = dict(resolution=4.0, step_size=1.0, transformation_epsilon=0.01, min_points_per_voxel=8)
    beyond = np.array([-2.0 ** -50, 0.0, 0.0, 0.0, 0.0, 0.0])
    return dict(name="lattice", tgt=cloud(tgt), src=cloud(src), prm=prm, G=None, truth=None, centres=centres, beyond=beyond)


# ---- shapes
def ragged(n):
    """`centred` with a source of n points (tiled from the target, each copy shifted a little)"""
    case = centred("res5")
    t = case["tgt"][:, :3].astype(np.float64)
    reps = -(-n // len(t))
    pts = np.concatenate([t + 0.01 * k for k in range(reps)])[:n]
    case.update(name="ragged-%d" % n, src=cloud(_moved(pts, 0.5 * P_STAR, np.zeros(3))), truth=None)
    return case


def voxel_edges():
    """Resolution 8, voxels with 5, 6 and 7 points (min_points_per_voxel 6: the first is not a cell), one with 5 000, one of 9
    coincident points (dropped: lmax = 0) and a planar one (z constant: its smallest eigenvalue is inflated)."""
    rng = np.random.default_rng(71)
    parts = []
    for n, corner in ((5, (0, 0, 0)), (6, (8, 0, 0)), (7, (16, 0, 0)), (5000, (0, 8, 0))):
        parts.append(np.asarray(corner, np.float64) + 0.5 + 7.0 * rng.random((n, 3)))
    parts.append(np.tile([[20.0, 12.0, 4.0]], (9, 1)))
    plane = np.asarray((8.0, 8.0, 8.0)) + 0.5 + 7.0 * rng.random((40, 3))
    plane[:, 2] = 12.0
    parts.append(plane)
    tgt = np.concatenate(parts)
    src = tgt[rng.permutation(len(tgt))[:700]] + 0.3 * rng.standard_normal((700, 3))
    prm = dict(resolution=8.0, step_size=1.0, transformation_epsilon=0.01)
    return dict(name="voxel_edges", tgt=cloud(tgt), src=cloud(src), prm=prm, G=None, truth=None)


def nonfinite():
    """`centred` with a NaN source point and a NaN / an infinite target point; `clean`: the same clouds without them"""
    case = centred("res5")
    src, tgt = case["src"].copy(), case["tgt"].copy()
    clean = dict(case, src=np.delete(src, [7], 0), tgt=np.delete(tgt, [11, 5000], 0), name="nonfinite-clean",
                 truth=np.delete(case["truth"], [7], 0))
    src[7, 1] = np.nan
    tgt[11, 0] = np.nan
    tgt[5000, 2] = np.inf
    case.update(name="nonfinite", src=src, tgt=tgt, clean=clean)
    return case


def disjoint():
    case = centred("res5")
    src = case["src"].copy()
    src[:, 0] += 1000.0
    case.update(name="disjoint", src=src, truth=None)
    return case


def poses():
    """where the sums are checked: identity, p* / 2, p*"""
    return [np.zeros(6), 0.5 * P_STAR, P_STAR.copy()]


# ---- the edges of the kernels
def many_voxels(n_cu):
    """64 n_cu + 5 voxels of three points each, one layer in z: the wave-per-voxel loop of the cell kernel (64 n_cu waves at
    most) laps, every voxel is a cell (min_points_per_voxel 3), so there are n / 3 cells, one below the capacity n / 3 + 1,
    and every cell is planar: its smallest eigenvalue is inflated.  The source is 500 of the points, jittered."""
    rng = np.random.default_rng(23)
    nv = 64 * int(n_cu) + 5
    w = int(np.ceil(np.sqrt(nv)))
    v = np.arange(nv)
    corner = np.stack([4.0 * (v % w), 4.0 * (v // w), np.zeros(nv)], 1)
    tri = np.array([[1.0, 1.0, 1.0], [3.0, 1.0, 1.0], [1.0, 3.0, 1.0]])
    pts = corner[:, None, :] + tri[None, :, :] + np.concatenate([0.25 * (2.0 * rng.random((nv, 3, 2)) - 1.0), np.zeros((nv, 3, 1))], 2)
    tgt = pts.reshape(-1, 3)[rng.permutation(3 * nv)]
    src = tgt[rng.permutation(len(tgt))[:500]] + 0.1 * rng.standard_normal((500, 3))
    prm = dict(resolution=4.0, step_size=1.0, transformation_epsilon=0.01, min_points_per_voxel=3)
    return dict(name="many_voxels", tgt=cloud(tgt), src=cloud(src), prm=prm, G=None, truth=None, n_voxels=nv)


LINE_T = 0.5 + 0.625 * np.arange(10)          # exact in f32, inside a voxel of 8


def lane_edges():
    """Resolution 8.  Voxels of 63, 64, 65, 127, 128 and 129 points, the edges of the lane loop k += 64; a voxel of 10 points
    on its diagonal and one of 10 points along x (collinear: two eigenvalues inflated, C^-1 = (1 / l)(u u^T + 100 (I - u u^T))
    with l = (9 / 100) sum |p - m|^2 and u the line); a voxel of 6 points 1e-4 apart (a covariance of 1e-9: the Jacobi
    threshold has to be relative)."""
    rng = np.random.default_rng(29)
    parts = []
    for k, n in enumerate((63, 64, 65, 127, 128, 129)):
        parts.append(np.array([8.0 * (k % 3), 8.0 * (k // 3), 0.0]) + 0.5 + 7.0 * rng.random((n, 3)))
    parts.append(np.array([0.0, 0.0, 8.0]) + LINE_T[:, None] * np.ones(3))
    parts.append(np.array([8.0, 0.0, 8.0]) + np.stack([LINE_T, np.full(10, 4.0), np.full(10, 4.0)], 1))
    parts.append(np.array([20.0, 4.0, 12.0]) + 1e-4 * rng.standard_normal((6, 3)))
    tgt = np.concatenate(parts)
    src = tgt[rng.permutation(len(tgt))[:300]] + 0.3 * rng.standard_normal((300, 3))
    prm = dict(resolution=8.0, step_size=1.0, transformation_epsilon=0.01)
    return dict(name="lane_edges", tgt=cloud(tgt), src=cloud(src), prm=prm, G=None, truth=None,
                counts=[63, 64, 65, 127, 128, 129, 10, 10, 6], diagonal_key=0 + 0 + 1 * 3 * 2, axis_key=1 + 0 + 1 * 3 * 2)


def line_icov(points):
    """C^-1 of a voxel of collinear points in closed form: (1 / l)(u u^T + 100 (I - u u^T)), l = ((n - 1) / n^2) sum |p - m|^2"""
    q = np.asarray(points, np.float64)
    n, d = len(q), q - q.mean(0)
    u = (q[-1] - q[0]) / np.linalg.norm(q[-1] - q[0])
    M = (np.outer(u, u) + 100.0 * (np.eye(3) - np.outer(u, u))) / (((n - 1.0) / n ** 2) * (d * d).sum())
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def borders():
    """`lattice`'s target (div 3 x 2 x 2, min_b 0) with source points one voxel outside the lattice (home voxel h = -1 or
    h = div on one axis: rule N5 still looks at the lattice's rim, and each is 3 from one centre), two voxels outside (h = -2,
    h = div + 1: nothing), and two finite points whose voxel index is astronomically far out"""
    case = lattice()
    counted = [(-1.0, 2.0, 2.0), (2.0, -1.0, 2.0), (2.0, 2.0, -1.0), (13.0, 6.0, 6.0), (2.0, 9.0, 2.0), (2.0, 2.0, 9.0)]
    unseen = [(-5.0, 2.0, 2.0), (2.0, -5.0, 2.0), (2.0, 2.0, -5.0), (17.0, 6.0, 6.0), (2.0, 13.0, 2.0), (2.0, 2.0, 13.0),
              (3e38, 2.0, 2.0), (2.0, 1e30, 2.0)]
    case.update(name="borders", src=cloud(np.array(counted + unseen)), n_counted=len(counted), pairs=[9.0] * len(counted))
    del case["beyond"]
    return case


GUARD_OFFSETS = (0.0, 1e-6, 3e-6, 1e-5, 1e-4, 5e-4)
GUARD_COUNTS = (0, 0, 1, 1, 1, 1)


def weight_guard():
    """Resolution 0.002 and outlier ratio 0.99 give d2 = 1 + 6.25e-6 > 1, so w = d2 exp(-d2 q / 2) > 1 for q < 2 ln(d2) / d2:
    rule N6's guard skips the pair.  One cell (the corners (+-0.0005)^3 about 0.001, C^-1 = (8 / 7) / 2.5e-7 I) and source
    points on the x axis at GUARD_OFFSETS from its mean; the threshold is at 1.65e-6."""
    corners = np.array([[a, b, c] for a in (-1.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)])
    tgt = cloud(0.0005 * corners + 0.001)
    mean = tgt[:, :3].astype(np.float64).mean(0)
    src = np.array([mean + (o, 0.0, 0.0) for o in GUARD_OFFSETS])
    prm = dict(resolution=0.002, outlier_ratio=0.99, step_size=1e-4, transformation_epsilon=1e-6, min_points_per_voxel=8)
    return dict(name="weight_guard", tgt=tgt, src=cloud(src), prm=prm, G=None, truth=None)


def sparse_native():
    """`centred` with one more target point at (1500, 1500, 1500): no cell, but the lattice now has more than 1 << 24 voxels
    and the default context searches the kept keys.  min_b and the order of the voxels are `centred`'s."""
    case = centred("res5")
    case.update(name="sparse_native", tgt=np.concatenate([case["tgt"], cloud([[1500.0, 1500.0, 1500.0]])]))
    return case


BIG_ANGLES = [np.array([1.0, -0.6, 0.5, 1.2, -1.5, 2.8]), np.array([0.0, 0.0, 0.0, 3.1, np.pi / 2 - 1e-3, -3.1])]


def big_angles():
    """[(case, p)]: `centred` at two poses with large angles, the second 1e-3 from ry = pi / 2, each on top of a guess
    G = X(p)^-1 X(p* / 2), so that X(p) G = X(p* / 2) and the source still lies over the target"""
    out = []
    for k, p in enumerate(BIG_ANGLES):
        case = centred("res5")
        case.update(name="big_angles-%d" % k, G=np.linalg.inv(R.pose_matrix(p)) @ R.pose_matrix(0.5 * P_STAR))
        out.append((case, p))
    return out
