"""The inputs the FPFH tests share (tests/test_gpu_fpfh.py compares the GPU on them, tests/test_fpfh_host.py checks on the
reference alone that the share of queries with a slack pair stays under its cap).  Every case is (points [n, 4], normals
[n, 4], radius).  The GPU tests replace the normals of the view by those mvr_cloud_estimate_normals gives for the same points;
the host test takes them from tests/normals_ref.py, the reference of that call -- and so for the surface normals of the
patches among the walk cases."""
import numpy as np

import mls_cases as K
import normals_ref as NR
import walk_cases as W

F32, F64 = np.float32, np.float64
VIEW_N, VIEW_NORMAL_RADIUS, VIEW_RADIUS = 20000, 2.5, 5.0
BOX_N, BOX_EDGE, BOX_RADIUS = 3000, 20.0, 3.0
SLACK_CAP = 0.30                   # the largest share of queries with any slack pair on the view and on the box
TINY_SIZES = (0, 1, 2, 3, 5)


def view(mvr, n=VIEW_N):
    """(a) view 0 of config 3"""
    return mvr.synth_view(mvr.synth_params(12, 3), 0, n)


def ref_normals(p, radius=VIEW_NORMAL_RADIUS):
    flat, offs = NR.radius_sets(p, radius)
    return NR.normals_from_sets(p, flat, offs)[0]


def unit_normals(rng, n):
    v = rng.standard_normal((n, 3))
    out = np.zeros((n, 4), F32)
    out[:, :3] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    return out


def box(n=BOX_N, seed=11):
    """(b) uniform in a 20 mm box at the scan's depth, random unit normals: every one of the 33 bins is filled and the swap of
    F3 is taken about half the time"""
    rng = np.random.default_rng(seed)
    p = W.cloud(rng.uniform(-BOX_EDGE / 2, BOX_EDGE / 2, (n, 3)) + [0.0, 0.0, 917.0])
    return p, unit_normals(rng, n), BOX_RADIUS


def with_invalid(p, nrm, seed=5):
    """(c) scattered non-finite points (mls_cases.with_non_finite) and a few non-finite normals on other points:
    (points, normals, indices of the invalid points)"""
    q, bad = K.with_non_finite(p, seed=seed)
    m = nrm.copy()
    rest = np.setdiff1d(np.arange(len(p)), bad)
    nb = np.random.default_rng(seed + 1).choice(rest, min(12, len(rest)), replace=False)
    for j, i in enumerate(nb):
        m[i, j % 3] = (np.nan, np.inf, -np.inf)[(j // 3) % 3]
    return q, m, np.sort(np.concatenate([bad, nb, np.nonzero(~np.isfinite(nrm[:, :3]).all(1))[0]]))


def tiny(n, seed=3):
    """(d) n points 2 mm apart in a row with random normals, radius 0.8: every point alone (n_i = 1); no grid below 4 points"""
    rng = np.random.default_rng(seed + n)
    p = W.cloud(np.c_[2.0 * np.arange(n), np.zeros(n), np.full(n, 900.0)] + rng.uniform(-0.1, 0.1, (n, 3)) if n else np.zeros((0, 3)))
    return p, unit_normals(rng, n), 0.8


def duplicates(n=1500, seed=17):
    """(e) a box cloud in which every fifth point is an exact copy of its predecessor (its own normal) and ten points are copies
    of point 0: pairs with d2 == 0"""
    rng = np.random.default_rng(seed)
    p = W.cloud(rng.uniform(-6.0, 6.0, (n, 3)) + [0.0, 0.0, 917.0])
    p[4::5] = p[3::5][:len(p[4::5])]
    p[rng.choice(np.arange(1, n), 10, replace=False)] = p[0]
    return p, unit_normals(rng, n), 2.0


DEGENERATE = ("all_identical", "collinear", "regular_grid_midpoints", "huge_coordinates")


def degenerate(name, mvr):
    """(f) the target of a degenerate set of walk_cases.py with random unit normals, at the `several cells` radius"""
    t = W.get(name, mvr)[1]
    rng = np.random.default_rng(23)
    return t, unit_normals(rng, len(t)), float(W.radii(name, t)["several_cells"])


# the walk cases (tests/walk_cases.py) the descriptor is run on: the target clouds
WALK = ("patch_at_0", "patch_far_1e5", "patch_far_1e6", "lattice_3d", "clusters_and_a_far_point", "two_far_clusters", "duplicates_41",
        "every_target_duplicated", "planar_sheet") + tuple("size_%d" % n for n in W.SIZES)
WALK_SURFACE = tuple(n + "-surface" for n in WALK[:3])      # the patches a second time, with the normals of their surface
WALK_NORMAL_CELLS = 2.5                                      # radius of those normals, in grid edges
WALK_RADIUS_MM = {"clusters_and_a_far_point": 0.5, "two_far_clusters": 0.5}      # the grid edge spans the gap between the clusters:
#                                                              a small ball in cells that hold thousands of points
WALK_RADIUS_CELLS = {"lattice_3d": 2.0}                      # at one edge every lattice point is alone


def walk_radius(name, t):
    name = name.split("-")[0]
    return float(WALK_RADIUS_MM[name]) if name in WALK_RADIUS_MM else float(WALK_RADIUS_CELLS.get(name, 1.0) * W.grid_edge(t))


def walk(name, mvr):
    """(g) the target of a walk case with random unit normals (those of degenerate()), at a radius of one grid edge but for the
    exceptions above.  For a name of WALK_SURFACE the normals are None: the caller estimates them at walk_normal_radius() --
    the GPU test with the library, the host test with ref_normals"""
    t = W.get(name.split("-")[0], mvr)[1]
    nrm = None if name.endswith("-surface") else unit_normals(np.random.default_rng(23), len(t))
    return t, nrm, walk_radius(name, t)


def walk_normal_radius(t):
    return float(WALK_NORMAL_CELLS * W.grid_edge(t))


def moved(p, nrm):
    """a rigidly moved copy of a cloud and its normals: a rotation of 0.7 rad about a skew axis through the scan and a shift,
    applied on the host in f64"""
    Rm = K.rodrigues([0.3, -0.5, 0.81], 0.7)
    c = np.array([0.0, 0.0, 917.0])
    q, m = p.copy(), nrm.copy()
    q[:, :3] = ((p[:, :3].astype(F64) - c) @ Rm.T + c + [7.0, -3.0, 11.0]).astype(F32)
    m[:, :3] = (nrm[:, :3].astype(F64) @ Rm.T).astype(F32)
    return q, m
