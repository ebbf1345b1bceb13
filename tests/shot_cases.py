"""The inputs the SHOT tests share (tests/test_gpu_shot.py compares the GPU on them, tests/test_shot_host.py checks on the
reference alone what the comparison presupposes).  A descriptor case is (points [n, 4], normals [n, 4] or None, radius); None
stands for the normals of a surface, which the GPU tests take from the library (mvr_cloud_estimate_normals at NORMAL_RADIUS) and
the host test does not need (a frame needs no normal).

A frame is compared axis by axis only where the reference says it is well conditioned: eigen-gap >= GAP and, per axis, a sign
margin |2 plus - n| above TWICE the number of neighbours whose dot product with the axis is within 1e-9 |v| of zero (see
decided(); the query's own point is not among them, rule L2 skips it).  The sign of an axis is a vote, so the frames are compared at radii of their
own, FRAME_RADIUS, with 500 to 620 neighbours: at 30 neighbours a quarter of the votes end within two of a tie.  Measured on the
reference (tests/test_shot_host.py asserts >= 90 %): view 99.0 %, box 99.1 %, skew 98.1 % of the queries fully compared."""
import numpy as np

import fpfh_cases as FC
import pfh_cases as PC
import walk_cases as W

F32, F64 = np.float32, np.float64
DIM = 352
GAP = 1.0e-3
FRAME_SHARE = 0.90
NORMAL_RADIUS = 6.0
CELL_POINTS = PC.CELL_POINTS        # the grid resolutions the walk tests sweep (tune key seq_cell_points)
ROW_SIZES = (1, 63, 64, 65, 129)    # points in one cell row: the lane and ballot edges of the cooperative walk
FRAME_CASES = ("view", "box", "skew")
FRAME_RADIUS = {"view": 40.0, "box": 8.0, "skew": 4.0}      # the descriptor cases keep smaller radii: the reference stays quick
# the bar of |S_gpu - S_ref| per slot, in amounts (units of 2^32) per neighbour of the query: 16 x the worst measured on an
# MI355X (1.45e-12, tests/test_gpu_shot.py), rounded up to a power of ten
SUMS_BAR = 1.0e-10


def decided(fr):
    """[nq, 2]: the sign vote of x and of z cannot come out differently from another starting sign of the eigenvector.  A dot
    product at zero counts as "plus" under EITHER sign of the axis (L5: >= 0), so with Z such neighbours the vote that starts
    from -a has the margin 2 Z - m where the vote from a has m: both end on the same axis iff m < 0 or m > 2 Z.  (A margin
    above Z alone leaves m = 2 with Z = 1, where the vote from -a is a tie.)  Here: |m| > 2 Z."""
    return fr["margin"] > 2 * fr["near"]


def view(mvr):
    """(a) pfh_cases.view, 5 000 points of a synthetic scan, at a radius of 25 mm (257 neighbours on average)"""
    return PC.view(mvr), None, 25.0


def box():
    """(b) fpfh_cases.box at twice its radius (240 neighbours): random unit normals, every volume and shape slot reached"""
    p, nrm, _ = FC.box()
    return p, nrm, 6.0


def skew(n=1500, seed=3):
    """(c) a density that falls off along all three axes at different rates: the sign votes of L5 are decided by the gradient"""
    rng = np.random.default_rng(seed)
    p = W.cloud(rng.exponential(1.0, (n, 3)) * [3.0, 2.5, 2.0] + [0.0, 0.0, 900.0])
    return p, FC.unit_normals(rng, n), 4.0


def with_invalid(p, nrm):
    """(d) scattered non-finite points and normals (fpfh_cases.with_invalid)"""
    return FC.with_invalid(p, nrm)


def small(n, seed=7):
    """(e) n points inside one ball of radius 1 around (1, 2, 900), random normals; radius 3: everybody is everybody's neighbour"""
    rng = np.random.default_rng(seed + n)
    v = rng.standard_normal((n, 3))
    v *= (rng.uniform(0.2, 1.0, n) / np.maximum(np.linalg.norm(v, axis=1), 1e-9))[:, None]
    return W.cloud(v + [1.0, 2.0, 900.0]), FC.unit_normals(rng, n), 3.0


def copies(n=6):
    """(f) n copies of one point: n neighbours at d == 0, which add nothing (H2): S == 0, norm == 0, a NaN row (H8)"""
    p = np.tile(np.array([1.0, 2.0, 900.0, 1.0], F32), (n, 1))
    nrm = np.tile(np.array([0.0, 0.6, 0.8, 0.0], F32), (n, 1))
    return p, nrm, 0.5


def row(n, seed=11):
    """(g) n points along x, 0.01 mm apart with a jitter of a micrometre in y and z: one cell row of the grid, all inside a ball
    of radius 3"""
    rng = np.random.default_rng(seed + n)
    xyz = np.c_[0.01 * np.arange(n), rng.uniform(-1e-3, 1e-3, n), 900.0 + rng.uniform(-1e-3, 1e-3, n)]
    return W.cloud(xyz), FC.unit_normals(rng, n), 3.0


def long_row(mvr):
    """(h) walk_cases' collinear target: 2 000 points on a line over 512 cells of the grid, at a radius of 3.5 cells"""
    t = W.get("collinear", mvr)[1]
    return t, FC.unit_normals(np.random.default_rng(23), len(t)), float(W.radii("collinear", t)["several_cells"])


def lattice():
    """(i) walk_cases' 3-D lattice (step 0.25) at a radius of two steps, for frames passed in as the identity: neighbours ON the z
    axis (acos(+-1), x == y == 0), on sector borders (|x| == |y|), on the husk border (d == R / 2 exactly) and on the equator
    (z == 0), every one of them exact in f64"""
    t = W.lattice()[1]
    return t, FC.unit_normals(np.random.default_rng(29), len(t)), 2.0 * W.LATTICE_STEP


def identity_frames(n):
    return np.tile(np.eye(3, dtype=F32).reshape(1, 9), (n, 1))


def patch(mvr):
    """(j) pfh_cases.patch: 1 500 surface points on a lattice of 1 / 16 mm, which pfh_cases.patch_moved translates exactly"""
    p = PC.patch(mvr)
    return p, None, 2.0 * PC.patch_radius(p)


def tie(m=40, seed=5):
    """(k) an _at query whose sign votes TIE and whose tie sums decide: 2 m surface points in opposite directions from the query
    -- every dot product has its mirror, so plus == m == n / 2 on every axis but for dots at zero -- at DIFFERENT distances, the
    + member of a pair, on the side of (1, 1, 1), nearer than its mirror: (surface points, normals, query cloud, radius)"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((m, 3)) * [3.0, 2.0, 1.0]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[u @ np.ones(3) < 0] *= -1.0
    c = np.array([2.0, -1.0, 900.0])
    near, far = rng.uniform(0.5, 1.0, m), rng.uniform(1.5, 2.5, m)      # (w d = (R - d) d: 3.2 against 6, the far members outweigh)
    p = W.cloud(np.r_[c + u * near[:, None], c - u * far[:, None]])
    return p, FC.unit_normals(rng, 2 * m), W.cloud(c[None, :]), 5.0


def at_indices(n, seed=13):
    """unsorted, repeated indices into a cloud of n points"""
    rng = np.random.default_rng(seed)
    return np.r_[rng.integers(0, n, 300), [0, n - 1, n - 1, 0]].astype(np.uint32)
