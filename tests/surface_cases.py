"""The surfaces and the query sets the tests of the *_at calls share (tests/test_gpu_surface.py compares the GPU on them,
tests/test_surface_host.py checks on the reference alone that the share of slack pairs of the off-surface cases stays under
pfh_cases.SLACK_CAP).  The surfaces are those of fpfh_cases.py / pfh_cases.py; a surface is (points [n, 4], normals [n, 4],
radius), the normals of the view being None: the GPU tests take the library's, the host test those of tests/normals_ref.py."""
import numpy as np

import fpfh_cases as FC
import pfh_cases as PC

F32, F64 = np.float32, np.float64
SUBSET, REPEATS, OFF_MM, FAR_MM = 300, 10, 0.4, 1.0e4
SEED = 41
K = 16
TINY = tuple("tiny%d" % n for n in FC.TINY_SIZES)
SURFACES = ("box", "duplicates", "view", "invalid", "blob") + TINY
OFF_SURFACE = SURFACES            # the off-surface (c) and degenerate (d) queries run on every surface, those without a grid included
LARGE = ("box", "duplicates", "view", "invalid", "blob")      # the surfaces whose points have neighbours at the case's radius
BLOB_STEP = 12                    # the blob's neighbourhoods hold ~73 000 pairs each: the reference takes every 12th query (and the last three)
NORMAL_RADIUS = {"view": PC.VIEW_NORMAL_RADIUS, "invalid": PC.VIEW_NORMAL_RADIUS}      # else the case's own radius


def surface(name, mvr, view_normals):
    """view_normals(points, radius) -> normals [n, 4]: how the caller estimates the normals of the view"""
    if name == "box":
        return FC.box()
    if name == "duplicates":
        return FC.duplicates()
    if name in ("view", "invalid"):
        p = PC.view(mvr)
        nrm = view_normals(p, PC.VIEW_NORMAL_RADIUS)
        if name == "invalid":
            p, nrm, _ = FC.with_invalid(p, nrm)
        return p, nrm, PC.VIEW_RADIUS
    if name == "blob":
        return PC.blob()
    return FC.tiny(int(name[4:]))


def subset_with_repeats(n, seed=SEED):
    """(a) a shuffled subset of min(300, n) points with 10 repeats appended (none of an empty cloud)"""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(n)[:SUBSET]
    rep = rng.choice(idx, REPEATS) if n else idx
    return np.concatenate([idx, rep]).astype(np.uint32)


def off_surface(p, seed=SEED):
    """(c) min(300, n) FINITE surface points, each moved by a uniform +-0.4 mm per axis"""
    rng = np.random.default_rng(seed)
    fin = np.nonzero(np.isfinite(p[:, :3]).all(1))[0]
    idx = rng.permutation(fin)[:SUBSET]
    q = p[idx].copy()
    q[:, :3] = (q[:, :3].astype(F64) + rng.uniform(-OFF_MM, OFF_MM, (len(idx), 3))).astype(F32)
    return q


def reference_rows(name, rows):
    """the rows of a query set of `rows` queries the PFH reference is computed for: all, but on the blob"""
    r = np.arange(rows)
    return r if name != "blob" else np.unique(np.concatenate([r[::BLOB_STEP], r[-3:]]))


def degenerate(p, at):
    """(d) three queries: one 1e4 mm away (an empty neighbourhood), one with a NaN coordinate, one exactly at surface point `at`"""
    q = np.zeros((3, 4), F32)
    q[:, 3] = 1.0
    c = p[at, :3] if len(p) else np.array([0.0, 0.0, 917.0], F32)
    q[0, :3] = c + F32([FAR_MM, 0.0, 0.0])
    q[1, :3] = [c[0], np.nan, c[2]]
    q[2, :3] = c
    return q
