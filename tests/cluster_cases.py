"""The case table of tests/test_gpu_cluster.py: the smallest clouds on which the Euclidean cluster extraction
(csrc/mvr_cluster.hip; rules E1-E8 in include/mvr_hip.h) can go wrong.  Answers come from tests/cluster_ref.py (all pairs, no
grid) -- and, where `expect` is set, from a hand count that tests/test_cluster_host.py holds the reference to.

A Case holds pts (n, 4) f32, the tolerance, kw = the other arguments of Context.euclidean_clusters / cluster_ref.clusters
(min_size, max_size, eps_angle, index, negative), normals (n, 4) f32 or None, and expect = None or the sorted-descending list
of cluster sizes plus (too_small, too_large)."""
import math

import numpy as np

import walk_cases as W

F32 = np.float32
NAN, INF = float("nan"), float("inf")


class Case:
    def __init__(self, name, pts, tolerance, normals=None, expect=None, **kw):
        self.name, self.pts, self.tolerance, self.kw, self.expect = name, np.ascontiguousarray(pts, F32), float(tolerance), kw, expect
        self.normals = None if normals is None else np.ascontiguousarray(normals, F32)
        assert self.pts.ndim == 2 and self.pts.shape[1] == 4


def cloud(xyz):
    return W.cloud(np.asarray(xyz, np.float64).reshape(-1, 3))


def nrm(v):
    out = np.zeros((len(v), 4), F32)
    out[:, :3] = np.asarray(v, F32)
    return out


def helix(n, chord=0.95, radius=10.0, pitch=3.0, centre=(0.0, 0.0, 900.0), phase=0.0):
    """n points along a helix, consecutive points `chord` apart (below a tolerance of 1), successive turns `pitch` apart: one
    chain that winds through many cells"""
    # the chord of an angle step a: sqrt((2 R sin(a / 2))^2 + (pitch a / (2 pi))^2) -- solved for a by bisection
    lo, hi = 0.0, 1.0
    for _ in range(80):
        a = 0.5 * (lo + hi)
        c = math.hypot(2.0 * radius * math.sin(a / 2.0), pitch * a / (2.0 * math.pi))
        lo, hi = (a, hi) if c < chord else (lo, a)
    t = phase + lo * np.arange(n)
    return np.c_[radius * np.cos(t), radius * np.sin(t), pitch * (t - phase) / (2.0 * np.pi)] + np.asarray(centre)


def snake(n=600, seed=3):
    """(cloud, position of every index along the chain): the helix in shuffled index order"""
    pos = np.random.default_rng(seed).permutation(n)          # index i sits at position pos[i]
    return cloud(helix(n)[pos]), pos


def two_snakes(n=600):
    """two helices of radius 10 and 11.01 (1.01 tolerances apart, never touching), interleaved in index"""
    a, b = helix(n), helix(n, radius=11.01)
    rng = np.random.default_rng(4)
    xyz = np.empty((2 * n, 3))
    xyz[0::2], xyz[1::2] = a[rng.permutation(n)], b[rng.permutation(n)]
    return cloud(xyz)


def lattice(pitch, dims=(9, 8, 7), origin=(-3.0, 10.0, 900.0)):
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    xyz = (g.astype(F32) * F32(pitch)).astype(F32) + np.asarray(origin, F32)
    return W.cloud(xyz)


def blobs(sizes, seed=5, spacing=10.0, sigma=0.05, shuffle=True):
    """tight blobs (every pair within 1 of each other) with centres `spacing` apart on a line through (0, 0, 900)"""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.standard_normal((s, 3)) * sigma + [spacing * k, 0.0, 900.0] for k, s in enumerate(sizes)])
    if shuffle:
        xyz = xyz[rng.permutation(len(xyz))]
    return cloud(xyz)


def dirty(seed=6):
    """320 points in blobs with every kind of non-finite value in every coordinate at the first, a middle and the last index"""
    p = blobs([100, 80, 60, 40, 40], seed)
    n = len(p)
    bad = [(0, 0, NAN), (1, 1, INF), (2, 2, -INF), (n // 2, 0, INF), (n // 2 + 1, 1, NAN), (n // 2 + 2, 2, NAN), (n - 3, 0, -INF),
           (n - 2, 1, -INF), (n - 1, 2, INF)]
    for i, k, v in bad:
        p[i, k] = v
    p[7, :3] = NAN
    return p


def sheets():
    """two interpenetrating 20 x 20 sheets of pitch 0.5 with perpendicular normals: z = 900 (normal z) and x = 5 (normal x)"""
    u = np.arange(20) * 0.5
    a = np.stack(np.meshgrid(u, u, [900.0], indexing="ij"), -1).reshape(-1, 3)
    b = np.stack(np.meshgrid([5.0], u, 900.0 - 4.75 + u, indexing="ij"), -1).reshape(-1, 3)
    n = np.concatenate([np.tile([0.0, 0.0, 1.0], (len(a), 1)), np.tile([1.0, 0.0, 0.0], (len(b), 1))])
    order = np.random.default_rng(8).permutation(len(a) + len(b))
    return cloud(np.concatenate([a, b])[order]), nrm(n[order])


def cube_faces(n=600, seed=9):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.0, 10.0, (n, 3))
    xyz[np.arange(n), rng.integers(0, 3, n)] = rng.choice([0.0, 10.0], n)          # every point on a face of the bounding box
    xyz[:8] = np.stack(np.meshgrid([0.0, 10.0], [0.0, 10.0], [0.0, 10.0]), -1).reshape(-1, 3)      # the corners
    return cloud(xyz + [0.0, 0.0, 900.0])


_cache = {}


def cases(mvr):
    """{name: Case}; mvr: the package (walk_cases takes its patches from the CPU scan generator)"""
    if "all" in _cache:
        return _cache["all"]
    out = []
    add = out.append
    one_up = float(np.nextafter(F32(0.5), F32(1)))
    add(Case("empty", np.zeros((0, 4), F32), 1.0, expect=([], 0, 0)))
    add(Case("one_point", cloud([[1.0, 2.0, 900.0]]), 1.0, expect=([1], 0, 0)))
    add(Case("pair_at_r2", cloud([[0, 0, 0], [0.5, 0, 0]]), 0.5, expect=([2], 0, 0)))                    # d2 == r2 == 0.25: linked (E2)
    add(Case("pair_one_ulp_beyond", cloud([[0, 0, 0], [one_up, 0, 0]]), 0.5, expect=([1, 1], 0, 0)))
    s, pos = snake()
    add(Case("snake", s, 1.0, expect=([600], 0, 0)))
    add(Case("two_snakes", two_snakes(), 1.0, expect=([600, 600], 0, 0)))
    add(Case("lattice_at_tolerance", lattice(0.25), 0.25, expect=([504], 0, 0)))
    add(Case("lattice_next_pitch_up", lattice(float(np.nextafter(F32(0.25), F32(1))), origin=(0.0, 0.0, 0.0)), 0.25))
    below = 0.25 * (1.0 - 1.0e-7)                                 # (float)(below * below) is an f32 under 0.0625
    assert F32(below * below) < F32(0.0625)
    add(Case("lattice_tolerance_below", lattice(0.25), below, expect=([1] * 504, 0, 0)))
    dup = cloud(np.tile([[1.0, 2.0, 900.0], [4.0, 2.0, 900.0]], (150, 1)))
    add(Case("exact_duplicates", dup, 1.0e-30, expect=([150, 150], 0, 0)))                               # r2 == 0: duplicates only
    add(Case("twelve_equal_blobs", blobs([20] * 12), 1.0, expect=([20] * 12, 0, 0)))
    sized = blobs([4, 5, 9, 10, 1])
    add(Case("sizes_min_max", sized, 1.0, min_size=5, max_size=9, expect=([9, 5], 2, 1)))
    add(Case("min_size_0", sized, 1.0, min_size=0, expect=([10, 9, 5, 4, 1], 0, 0)))
    add(Case("min_size_1", sized, 1.0, min_size=1, max_size=4, expect=([4, 1], 0, 3)))
    add(Case("min_above_max", sized, 1.0, min_size=9, max_size=5, expect=([], 3, 2)))
    add(Case("max_size_0", sized, 1.0, max_size=0, expect=([], 0, 5)))
    add(Case("non_finite", dirty(), 1.0))
    add(Case("no_finite_point", cloud([[NAN, 0, 0], [0, INF, 0], [0, 0, -INF], [NAN, NAN, NAN], [INF, -INF, NAN]]), 1.0,
             expect=([1] * 5, 0, 0)))
    add(Case("non_finite_without_a_grid", cloud([[0, 0, 0], [NAN, 0, 0], [0.5, 0, 0]]), 1.0, expect=([2, 1], 0, 0)))
    add(Case("far_frame_1e6", W.moved(blobs([100, 80, 60, 40, 40], 6), 1.0e6), 1.0))
    add(Case("far_frame_snakes", W.moved(two_snakes(), 1.0e6), 1.0))
    add(Case("bounding_box_faces", cube_faces(), 1.2))
    add(Case("tolerance_above_extent", blobs([100, 80, 60, 40, 40], 6), 1.0e4, expect=([320], 0, 0)))
    add(Case("tolerance_far_below_cell", np.concatenate([blobs([200, 100], 7, sigma=2.0), cloud([[0.0, 0.0, 900.0]] * 3)]), 1.0e-3))
    for name in W.NAMES:
        t = W.get(name, mvr)[1]
        r = W.radii(name, t)
        add(Case("walk_" + name + "_fraction", t, r["fraction_of_a_cell"], min_size=2))
        add(Case("walk_" + name + "_several", t, r["several_cells"], max_size=max(len(t) // 2, 1)))
    lat = W.get("lattice_3d", mvr)[1]
    add(Case("walk_lattice_3d_at_step", lat, W.LATTICE_STEP, expect=([len(lat)], 0, 0)))
    # normals (E3)
    sp, sn = sheets()
    add(Case("sheets_with_normals", sp, 0.6, normals=sn, eps_angle=math.pi / 4, expect=([400, 400], 0, 0)))
    add(Case("sheets_without_normals", sp, 0.6, normals=sn, expect=([800], 0, 0)))
    two = cloud([[0, 0, 0], [0.5, 0, 0]])
    add(Case("dot_exactly_0", two, 1.0, normals=nrm([[1, 0, 0], [0, 1, 0]]), eps_angle=math.pi / 2, expect=([1, 1], 0, 0)))
    add(Case("opposite_normals", two, 1.0, normals=nrm([[0, 0, 1], [0, 0, -1]]), eps_angle=math.pi, expect=([1, 1], 0, 0)))
    add(Case("equal_normals", two, 1.0, normals=nrm([[0, 0, 1], [0, 0, 1]]), eps_angle=1.0e-3, expect=([2], 0, 0)))
    line = cloud([[0, 0, 0], [0.9, 0, 0], [1.8, 0, 0]])
    add(Case("blocked_by_the_middle", line, 1.0, normals=nrm([[0, 0, 1], [1, 0, 0], [0, 0, 1]]), eps_angle=0.5, expect=([1, 1, 1], 0, 0)))
    deg = np.radians([0.0, 30.0, 60.0])
    add(Case("chained_through_the_middle", line, 1.0, normals=nrm(np.c_[np.sin(deg), 0 * deg, np.cos(deg)]), eps_angle=math.radians(40.0),
             expect=([3], 0, 0)))
    bp = blobs([60], 11)
    bn = nrm(np.tile([0.0, 0.0, 1.0], (60, 1)))
    bn[[0, 29, 59], 0] = NAN
    bn[30, :3] = [INF, 0.0, 0.0]
    add(Case("nan_normals", bp, 1.0, normals=bn, eps_angle=0.3, expect=([56, 1, 1, 1, 1], 0, 0)))
    # index subsets (E1)
    cut = int(np.nonzero(pos == 300)[0][0])                       # the index in the middle of the chain
    rest = np.delete(np.arange(600), cut)
    add(Case("snake_cut_by_the_subset", s, 1.0, index=np.concatenate([rest, rest[::7], rest[:3]]), expect=([300, 299], 0, 0)))
    add(Case("snake_cut_negative", s, 1.0, index=[cut, cut, cut], negative=True, expect=([300, 299], 0, 0)))
    add(Case("subset_of_blobs", blobs([20] * 12), 1.0, index=np.arange(0, 240, 3).repeat(2)))
    add(Case("subset_of_blobs_negative", blobs([20] * 12), 1.0, index=np.arange(0, 240, 3).repeat(2), negative=True))
    add(Case("empty_subset", sized, 1.0, index=np.zeros(0, np.uint32), expect=([], 0, 0)))
    add(Case("empty_subset_negative", sized, 1.0, index=np.zeros(0, np.uint32), negative=True, expect=([10, 9, 5, 4, 1], 0, 0)))
    _cache["all"] = {c.name: c for c in out}
    assert len(_cache["all"]) == len(out)
    return _cache["all"]


def names():
    """the case names, known without building a case (parametrisation)"""
    fixed = ["empty", "one_point", "pair_at_r2", "pair_one_ulp_beyond", "snake", "two_snakes", "lattice_at_tolerance", "lattice_next_pitch_up",
             "lattice_tolerance_below", "exact_duplicates", "twelve_equal_blobs", "sizes_min_max", "min_size_0", "min_size_1", "min_above_max",
             "max_size_0", "non_finite", "no_finite_point", "non_finite_without_a_grid", "far_frame_1e6", "far_frame_snakes", "bounding_box_faces",
             "tolerance_above_extent", "tolerance_far_below_cell"]
    walk = [("walk_%s_%s" % (n, t)) for n in W.NAMES for t in ("fraction", "several")] + ["walk_lattice_3d_at_step"]
    tail = ["sheets_with_normals", "sheets_without_normals", "dot_exactly_0", "opposite_normals", "equal_normals", "blocked_by_the_middle",
            "chained_through_the_middle", "nan_normals", "snake_cut_by_the_subset", "snake_cut_negative", "subset_of_blobs",
            "subset_of_blobs_negative", "empty_subset", "empty_subset_negative"]
    return fixed + walk + tail


_refs = {}


def reference(case, fma=False):
    """cluster_ref.clusters of a case, computed once per (case, fma) and shared"""
    import cluster_ref as R
    key = (case.name, bool(fma))
    if key not in _refs:
        _refs[key] = R.clusters(case.pts, case.tolerance, normals=case.normals, fma=fma, **case.kw)
    return _refs[key]
