"""The inputs the boundary tests share (tests/test_gpu_boundary.py compares the GPU on them, tests/test_boundary_host.py checks
on the reference alone that the conditions of the comparison hold).  Every case is a dict(p = points [n, 4], nrm = normals
[n, 4], radius, angle_threshold, min_neighbors, exact = whether the case must show both outcomes and an undecided share of at
most UNDECIDED_CAP).  The references (tests/boundary_ref.py) are computed once per process and shared.

The normals are part of the INPUT (the rule takes them from the slot): those of the view and of the patches are the surface
normals of tests/normals_ref.py, uploaded as they are, so the GPU and the reference start from the same bits."""
import numpy as np

import boundary_ref as R
import fpfh_cases as FC
import walk_cases as W

F32, F64 = np.float32, np.float64
VIEW_N = 20000
VIEW_SPACING = 1.27                # mm: 1 / sqrt(points per mm^2) of the 20 000-point view (11.7 points in a disc of 2.46 mm)
INVALID_RADIUS = 8.0               # the 6 000-point sample of it is 3.3 times sparser
UNDECIDED_CAP = 0.005
DEFAULTS = dict(angle_threshold=np.pi / 2, min_neighbors=0)
EXACT = ("view_3", "view_4", "box", "view_invalid", "duplicates", "patch_far_1e5", "patch_far_1e6")
TINY = tuple("tiny_%d" % n for n in FC.TINY_SIZES)
NAMES = EXACT + TINY
PATCH_CELLS = 2.5                  # radius of the patches, in grid edges (their surface normals: fpfh_cases.walk_normal_radius)

_cache = {}


def view(mvr):
    if "view" not in _cache:
        p = FC.view(mvr, VIEW_N)
        _cache["view"] = (p, FC.ref_normals(p))
    return _cache["view"]


def case(name, mvr):
    if name in ("view_3", "view_4"):
        p, nrm = view(mvr)
        c = dict(p=p, nrm=nrm, radius=float(name[5:]) * VIEW_SPACING, **DEFAULTS)
    elif name == "box":
        p, nrm, r = FC.box()
        c = dict(p=p, nrm=nrm, radius=r, **DEFAULTS)
    elif name == "view_invalid":
        p, nrm = view(mvr)
        q, m, _ = FC.with_invalid(p[:6000], nrm[:6000])
        c = dict(p=q, nrm=m, radius=INVALID_RADIUS, **DEFAULTS)
    elif name == "duplicates":
        p, nrm, r = FC.duplicates()
        c = dict(p=p, nrm=nrm, radius=r, **DEFAULTS)
    elif name.startswith("patch_far_"):
        t = W.get(name, mvr)[1]
        c = dict(p=t, nrm=FC.ref_normals(t, FC.walk_normal_radius(t)), radius=float(PATCH_CELLS * W.grid_edge(t)), **DEFAULTS)
    elif name.startswith("tiny_"):
        p, nrm, r = FC.tiny(int(name[5:]))
        c = dict(p=p, nrm=nrm, radius=r, **DEFAULTS)
    else:
        raise KeyError(name)
    c["exact"] = name in EXACT
    return c


def reference(name, mvr, fma=False):
    """(case, boundary_ref.boundary of it), computed once"""
    key = (name, fma)
    if key not in _cache:
        c = case(name, mvr)
        _cache[key] = (c, R.boundary(c["p"], c["nrm"], c["radius"], c["angle_threshold"], c["min_neighbors"], fma))
    return _cache[key]


# ---- constructed cases: the answer for point 0 is known without any reference
NORMALS = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0), "xy": (1.0, 1.0, 0.0)}      # xy: |n_x| == |n_y| in f32
CENTRE = np.array([3.0, -2.0, 900.0])
RING_RADIUS, RADIUS = 1.0, 1.5


def ring(normal, degrees, copies=0, zero_normal=False):
    """(points, normals): point 0 at CENTRE, `copies` exact copies of it, then one neighbour per angle (degrees, about the
    normal, from an arbitrary direction of the plane) at RING_RADIUS; every point carries the unit normal"""
    n = np.asarray(NORMALS[normal], F64)
    n /= np.linalg.norm(n)
    e1 = np.cross(n, [0.3, -0.5, 0.81])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    a = np.radians(np.asarray(degrees, F64))
    pts = np.concatenate([np.tile(CENTRE, (1 + copies, 1)), CENTRE + RING_RADIUS * (np.cos(a)[:, None] * e1 + np.sin(a)[:, None] * e2)])
    nrm = np.zeros((len(pts), 4), F32)
    nrm[:, :3] = n.astype(F32)
    if normal == "xy":
        assert nrm[0, 0] == nrm[0, 1]
    if zero_normal:
        nrm[0, :3] = 0.0
    return W.cloud(pts), nrm


# name -> (degrees, copies, keyword arguments of Context.boundary, whether point 0 is a boundary point, its neighbour count)
CONSTRUCTED = {
    "three_at_120": ([10, 130, 250], 0, {}, True, 4),
    "eight_at_45": (list(range(5, 365, 45)), 0, {}, False, 9),
    "half_plane": (list(range(20, 201, 30)), 0, {}, True, 8),
    "one_neighbour_and_copies": ([77], 2, {}, True, 4),
    "only_copies": ([], 3, {}, False, 4),
    "two_points": ([200], 0, {}, False, 2),
    "below_min_neighbors": ([10, 130, 250], 0, dict(min_neighbors=5), False, 4),
    "at_min_neighbors": ([10, 130, 250], 0, dict(min_neighbors=4), True, 4),
    "zero_normal": ([10, 130, 250], 0, dict(zero_normal=True), False, 4),
    "smallest_threshold_boundary": ([10, 130, 250], 0, dict(angle_threshold=R.MIN_ANGLE), True, 4),
    "smallest_threshold_interior": (list(range(5, 365, 30)), 0, dict(angle_threshold=R.MIN_ANGLE), False, 13),
}
