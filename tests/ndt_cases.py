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


def residual(X, case):
    """the largest distance of a source point under X from where it belongs"""
    s = case["src"][:, :3].astype(np.float64)
    return float(np.linalg.norm(s @ X[:3, :3].T + X[:3, 3] - case["truth"], axis=1).max())


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
