"""The inputs the PFH tests share (tests/test_gpu_pfh.py compares the GPU on them, tests/test_pfh_host.py checks on the reference
alone that the share of slack pairs stays under its cap).  Every radius case is (points [n, 4], normals [n, 4], radius); the
sizes and radii keep a case under about 5 M reference pairs.  Where the normals are those of a surface the GPU tests take the
library's (mvr_cloud_estimate_normals) and the host test those of tests/normals_ref.py, as in fpfh_cases.py."""
import numpy as np

import fpfh_cases as FC
import walk_cases as W

F32, F64 = np.float32, np.float64
DIM, STAGE = 125, 256              # MVR_PFH_DIM, MVR_PFH_STAGE
SLACK_CAP = 0.02                   # the largest share of slack PAIRS of a case (asserted on the reference alone)
VIEW_N, VIEW_NORMAL_RADIUS, VIEW_RADIUS = 5000, 6.0, 8.0
BLOB_N, BLOB_QUERIES = STAGE * 3 // 2, (0, 1, 191, 383)
KS = (1, 2, 16, 64)
CELL_POINTS = (4, 1, 64, 4096)     # the grid resolutions tests/test_gpu_fpfh.py sweeps (tune key seq_cell_points)
PATCH_STEP = 1.0 / 16.0            # the f32 spacing between 2^19 and 2^20: a patch on this lattice moves exactly
PATCH_FARS = (1.0e5, 1.0e6)


def view(mvr):
    """(a) view 0 of config 3, 5 000 points"""
    return mvr.synth_view(mvr.synth_params(12, 3), 0, VIEW_N)


def box():
    """(b) fpfh_cases.box: random normals, all 125 bins reachable, the swap of F3 taken half the time"""
    return FC.box()


def with_invalid(p, nrm):
    """(c)"""
    return FC.with_invalid(p, nrm)


def duplicates():
    """(d) fpfh_cases.duplicates: pairs with f4 == 0, key ties at d2 == 0"""
    return FC.duplicates()


def tiny(n):
    """(e)"""
    return FC.tiny(n)


def knn_cloud():
    """(f) the duplicates cloud for the k mode, the normal of point 0 made NaN: with k = 1 the ten copies of point 0 list point 0
    alone (the lowest index at d2 == 0) -- pushed out of their own lists, and left with n_i == 0"""
    p, nrm, _ = FC.duplicates()
    nrm = nrm.copy()
    nrm[0, 1] = np.nan
    return p, nrm


def blob(seed=29):
    """(g) 1.5 x the staging capacity in points inside one ball of radius 3 (every point is every point's neighbour at radius
    6.5), random normals: every query takes the tiled path"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((BLOB_N, 3))
    v *= (3.0 * rng.uniform(0, 1, BLOB_N) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return W.cloud(v + [0.0, 0.0, 917.0]), FC.unit_normals(rng, BLOB_N), 6.5


def patch(mvr):
    """(h) the 1 500-point surface patch of walk_cases.py, its coordinates rounded to multiples of 1 / 16"""
    p = W.get("patch_at_0", mvr)[0].copy()
    p[:, :3] = (np.rint(p[:, :3].astype(F64) / PATCH_STEP) * PATCH_STEP).astype(F32)
    return p


def patch_moved(p, far):
    """the patch `far` mm from the origin along walk_cases.FAR_DIR, the offset a multiple of 1 / 16: every f32 coordinate is the
    exact sum, so every f32 difference between two points is what it was"""
    off = np.rint(W.FAR_DIR * far / PATCH_STEP) * PATCH_STEP
    q = p.copy()
    q[:, :3] = (p[:, :3].astype(F64) + off).astype(F32)
    assert np.array_equal(q[:, :3].astype(F64) - off, p[:, :3].astype(F64))
    return q


def patch_radius(p):
    return float(1.6 * W.grid_edge(p))


def patch_normal_radius(p):
    return float(FC.WALK_NORMAL_CELLS * W.grid_edge(p))
