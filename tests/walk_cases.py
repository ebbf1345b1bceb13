"""The case table of tests/test_gpu_walk_fuzz.py: adversarial geometry for the kernels that walk a cloud's own grid (mvr_knn,
mvr_cloud_estimate_normals, the two outlier filters), and what may be asserted on each case.  Plain numpy plus the package's
CPU scan generator: tests/test_walk_cases_host.py checks every precondition stated here on the references alone.

A case is a (query, target) pair; the target is also searched against itself.  Per case:
  kind     what a normal is on the target
             "surface"  a sheet or a patch: the eigen-gap rule (gap = (l1 - l0) / l2 >= 1e-4) may exclude at most `cap` of the
                        points with a normal from the angle comparison
             "volume"   a 3-D blob or lattice: the same rule, the cap stated per case
             "plane"    an exact plane z = const: the answer is (0, 0, -1) (towards the viewpoint at the origin), curvature 0
             "line"     collinear: no defined direction; a finite unit vector orthogonal to the line, the reference's curvature
             "point"    all points identical: a finite unit vector, curvature 0
  cap      the share of points the gap rule may exclude (k mode at k = 16 and the radius of `several cells`); 1 % for the
           patch, planar, cluster and far-frame cases
  no_sets  the mean_k at which the statistical filter's inlier SET is NOT compared, because the reference cannot keep every
           mean distance 1e-9 (relative) away from the threshold: on the two lattices every point's nearest neighbour is one
           step away, so at mean_k = 1 all mean distances are equal, the deviation is 0 and the threshold IS that value.
           Mean distances and statistics are compared all the same.  (All-identical points pass: the threshold is exactly 0
           and 0 > 0 is false on both sides.)
Measured on the references alone (tests/test_walk_cases_host.py asserts it): excluded share 0 everywhere except
clusters_and_a_far_point 0.0002 (k), duplicates_41 0.0088 (k), every_target_duplicated 0.0017 (radius), lattice_3d 0.39
(radius); smallest gap of the patch 0.018 / 0.017 / 0.016 at 0 / 1e5 / 1e6 mm, of the planar sheet 0.09.  At 1e6 mm 2.4 % of
the patch's points have an exact f32 tie between their 16th and 17th neighbour and 0.2 % an exact duplicate; at 0 and 1e5 mm
none."""
import numpy as np

F32 = np.float32
FAR_DIR = np.array([0.61, -0.52, 0.6])
KS = (1, 9, 17, 33, 63, 64)
MEAN_KS = (1, 9, 33, 64)
SIZES = (3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)
LATTICE_STEP = 0.25                      # an exact f32, and so are its multiples up to 2^22 steps


def cloud(xyz):
    p = np.ones((len(xyz), 4), F32)
    p[:, :3] = np.asarray(xyz, F32)
    return p


def fuzz_geometries():
    """the eleven geometries of tests/test_gpu_fuzz.py (its cases(), copied: same seed, same draws)"""
    rng = np.random.default_rng(7)
    out = {}
    out["all_identical"] = (cloud(np.tile([1.0, 2.0, 900.0], (700, 1))), cloud(np.tile([1.0, 2.0, 900.0], (1500, 1))))
    t = rng.standard_normal((3000, 3)) * 5 + [0, 0, 900]
    out["every_target_duplicated"] = (cloud(rng.standard_normal((900, 3)) * 5 + [0, 0, 900]), cloud(np.concatenate([t, t[::-1]])))
    s = np.linspace(0, 100, 2000)
    out["collinear"] = (cloud(np.c_[s[::3] + 0.01, 0 * s[::3], 0 * s[::3] + 900]), cloud(np.c_[s, 0 * s, 0 * s + 900]))
    g = np.stack(np.meshgrid(np.arange(40.0), np.arange(40.0), [900.0]), -1).reshape(-1, 3)
    out["regular_grid_midpoints"] = (cloud(g[:1200] + [0.5, 0.5, 0]), cloud(g))          # 4-way exact ties
    a = rng.standard_normal((2500, 3)) + [0, 0, 900]
    b = rng.standard_normal((2500, 3)) + [5000, -3000, 900]
    out["two_far_clusters"] = (cloud(np.concatenate([a[:800], b[:800]])), cloud(np.concatenate([a, b])))
    out["queries_far_from_everything"] = (cloud(rng.standard_normal((500, 3)) + [1e4, 1e4, 1e4]), cloud(a))
    out["one_target"] = (cloud(rng.standard_normal((300, 3)) * 50), cloud([[3.0, -2.0, 1.0]]))
    out["one_query"] = (cloud([[0.3, 0.2, 900.1]]), cloud(a))
    out["planar_sheet"] = (cloud(np.c_[rng.uniform(0, 60, (1500, 2)), np.full(1500, 900.0)]),
                           cloud(np.c_[rng.uniform(0, 60, (5000, 2)), np.full(5000, 900.0)]))
    out["huge_coordinates"] = (cloud(rng.standard_normal((600, 3)) * 1e5), cloud(rng.standard_normal((2200, 3)) * 1e5))
    out["exactly_257_and_1025"] = (cloud(rng.standard_normal((257, 3)) * 3 + [0, 0, 900]), cloud(rng.standard_normal((1025, 3)) * 3 + [0, 0, 900]))
    return out


def surface_patch(mvr, n_view, n_patch):
    """the n_patch points of view 0 (n_view points: 200 000 is the density of a scan) nearest to one surface point"""
    v = mvr.synth_view(mvr.synth_params(12, 2), 0, n_view)
    c = v[:, :3].astype(np.float64).mean(0)
    seed = v[np.argmin(((v[:, :3] - c) ** 2).sum(1)), :3].astype(np.float64)
    order = np.argsort(((v[:, :3].astype(np.float64) - seed) ** 2).sum(1), kind="stable")
    return np.ascontiguousarray(v[np.sort(order[:n_patch])])


def moved(p, far):
    """p kept `far` mm from the origin: D = (0.61, -0.52, 0.6) * far added in f64, rounded to f32 (tests/test_gpu_exact.py)"""
    out = p.copy()
    out[:, :3] = (p[:, :3].astype(np.float64) + FAR_DIR * far).astype(F32)
    return out


def lattice():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(15), np.arange(14), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    t = cloud(g * LATTICE_STEP + [-3.0, 10.0, 900.0])                      # 6 neighbours at one step, 26 within sqrt(3) steps
    q = cloud(g[:1500] * LATTICE_STEP + [-3.0 + LATTICE_STEP / 2, 10.0 + LATTICE_STEP / 2, 900.0 + LATTICE_STEP / 2])      # cell centres: 8-way ties
    return q, t


_cache = {}

# kind, cap, no_sets; the fuzz geometries first
TABLE = {
    "all_identical": ("point", None, ()),
    "every_target_duplicated": ("volume", 0.01, ()),
    "collinear": ("line", None, ()),
    "regular_grid_midpoints": ("plane", 0.01, (1,)),
    "two_far_clusters": ("volume", 0.01, ()),
    "queries_far_from_everything": ("volume", 0.01, ()),
    "one_target": (None, None, ()),
    "one_query": ("volume", 0.01, ()),
    "planar_sheet": ("plane", 0.01, ()),
    "huge_coordinates": ("volume", 0.01, ()),
    "exactly_257_and_1025": ("volume", 0.01, ()),
    "patch_at_0": ("surface", 0.01, ()),
    "patch_far_1e5": ("surface", 0.01, ()),
    "patch_far_1e6": ("surface", 0.01, ()),
    "lattice_3d": ("volume", 0.5, (1,)),                    # cubic symmetry: a full ball has three equal eigenvalues
    "clusters_and_a_far_point": ("volume", 0.01, ()),
    "duplicates_41": ("volume", 0.01, ()),
}
for _n in SIZES:
    TABLE["size_%d" % _n] = ("volume", 0.01, ())
NAMES = sorted(TABLE)


def get(name, mvr):
    """(query, target) of a case"""
    if name in _cache:
        return _cache[name]
    if "fuzz" not in _cache:
        _cache["fuzz"] = fuzz_geometries()
    if name in _cache["fuzz"]:
        qt = _cache["fuzz"][name]
    elif name.startswith("patch_"):
        far = {"patch_at_0": 0.0, "patch_far_1e5": 1.0e5, "patch_far_1e6": 1.0e6}[name]
        if "patch" not in _cache:
            _cache["patch"] = (surface_patch(mvr, 150000, 1500), surface_patch(mvr, 200000, 6000))
        q, t = _cache["patch"]
        qt = (moved(q, far), moved(t, far)) if far else (q, t)
    elif name == "lattice_3d":
        qt = lattice()
    elif name == "clusters_and_a_far_point":
        rng = np.random.default_rng(31)
        a = rng.standard_normal((2500, 3)) + [0, 0, 900]
        b = rng.standard_normal((2500, 3)) + [5000, 0, 900]
        t = cloud(np.concatenate([a, b, [[1.0e5, 0.0, 900.0]]]))
        qt = (cloud(np.concatenate([a[:600] + 0.01, b[:600] - 0.01, [[2500.0, 0.0, 900.0], [9.0e4, 0.0, 900.0]]])), t)
    elif name == "duplicates_41":
        rng = np.random.default_rng(41)
        t = cloud(rng.standard_normal((5000, 3)) * 4 + [0, 0, 900])
        t[rng.choice(np.arange(1, 5000), 40, replace=False)] = t[0]                  # 41 copies of point 0, scattered by index
        q = cloud(rng.standard_normal((1200, 3)) * 4 + [0, 0, 900])
        q[:5] = t[0]
        qt = (q, t)
    elif name.startswith("size_"):
        n = int(name[5:])
        rng = np.random.default_rng(1000 + n)
        nq = SIZES[(SIZES.index(n) + 1) % len(SIZES)]
        qt = (cloud(rng.standard_normal((nq, 3)) * 3 + [0, 0, 900]), cloud(rng.standard_normal((n, 3)) * 3 + [0, 0, 900]))
    else:
        raise KeyError(name)
    _cache[name] = qt
    return qt


def grid_edge(p, cell_points=4):
    """the edge model_grid_size (csrc/mvr_grid_size.h) gives a finite cloud before any enlargement -- the unit of the radii"""
    P = p[:, :3].astype(np.float64)
    ext = np.maximum(1e-6, P.max(0) - P.min(0))
    area = ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]
    return max(np.sqrt(cell_points * area / max(len(p), 1)), ext.max() / 512.0)


def radii(name, p):
    """{tag: radius}: a fraction of a cell, several cells, larger than the whole cloud, one whose f32 square is 0 (exact
    duplicates only) -- and on the lattices one that IS a lattice distance (d2 == r2 must count)"""
    h = grid_edge(p)
    P = p[:, :3].astype(np.float64)
    diag = float(np.linalg.norm(P.max(0) - P.min(0)))
    out = {"fraction_of_a_cell": 0.3 * h, "several_cells": 3.5 * h, "whole_cloud": 2.0 * diag + 1.0, "zero_r2": 1.0e-30}
    assert F32(out["zero_r2"] * out["zero_r2"]) == 0
    if name == "lattice_3d":
        out["lattice_distance"] = LATTICE_STEP
        out["lattice_diagonal"] = float(np.sqrt(2.0) * LATTICE_STEP)          # (float)(r * r) rounds to 0.125 exactly
        assert F32(out["lattice_diagonal"] ** 2) == F32(0.125)
    if name == "regular_grid_midpoints":
        out["lattice_distance"] = 1.0
    return out


def boundary_case(h_target=0.3, n_fill=3000):
    """A target whose nearest point to the query lies in an UNVISITED cell, nearer than the cell's boundary: the f32 cell
    assignment floorf((x - lo) * inv_h) rounds a product just below the integer c up to c, so the point P sits in cell c while
    its f64 position, in cells of the same f32 inv_h, is c - delta (delta up to half an ulp of c, 1.5e-5 cells at c = 500).
    The query lies in cell c - 1 and a second point A of that cell is a hair farther than P.  After the first shell the k = 1
    list holds A, and the gap to the unvisited cell c is LARGER than the distance to P: a stopping bound without the margin for
    the cell assignment's rounding (the 1e-6 * mag term of knn_unvisited_bound) ends the walk there and returns
    A.  Everything lies on a line of 513 cells, so the grid is 513 x 1 x 1 with lo = 0 and an edge of L / 512.
    Returns (query cloud, target cloud, dict of the construction's figures)."""
    L = 512.0 * h_target
    fill_x = np.linspace(0.0, L, n_fill).astype(F32)          # lo = 0 and hi = L exactly; fillers on the line, removed near the action below
    h64 = float(F32(L)) / 512.0                                # model_grid_size: the longest extent / 512 (the area term is smaller, asserted below)
    inv_h = F32(1.0 / h64)
    ih = float(inv_h)
    best = None
    for c in range(505, 300, -1):
        x = F32(c * h64)
        for _ in range(40):                                    # f32 neighbours of the boundary, from above downwards
            u32 = np.floor(F32(x * inv_h))                     # the kernel's cell (f32 product, then floorf)
            u64 = float(x) * ih                                # the bound's position (f64)
            if u32 == c and c - 1.45e-5 < u64 < c - 0.9e-5:
                best = (c, x, c - u64)
                break
            x = np.nextafter(x, F32(0))
        if best:
            break
    assert best, "no f32 coordinate rounds across a cell boundary far enough"
    c, xP, delta = best
    xq = F32((c - 0.5) * h64)                                  # the query, in the middle of cell c - 1
    uq = float(xq) * ih
    assert np.floor(F32(xq * inv_h)) == c - 1
    gap = c - uq                                               # cells between the query and the unvisited cell c
    dP = float(xP) - float(xq)
    b_plain = gap / ih - 1.0e-6 / ih                           # the bound WITHOUT the 1e-6 * mag term
    lo_d2, hi_d2 = dP * dP * (1.0 + 1.0e-6), b_plain * b_plain * (1.0 - 1.0e-5) * (1.0 - 1.0e-6)
    assert lo_d2 < hi_d2, (delta, gap)
    dA = np.sqrt(0.5 * (lo_d2 + hi_d2))                        # A: between P and the bound
    xA = F32((c - 0.8) * h64)                                  # in cell c - 1, on the other side of the query
    assert np.floor(F32(xA * inv_h)) == c - 1
    dxA = float(xq) - float(xA)
    yA = F32(np.sqrt(dA * dA - dxA * dxA))
    keep = np.abs(fill_x.astype(np.float64) - float(xq)) > 2.5 * h64       # no filler within two cells of the query
    keep[0] = keep[-1] = True
    pts = [[float(v), 0.0, 0.0] for v in fill_x[keep]] + [[float(xA), float(yA), 0.0], [float(xP), 0.0, 0.0]]
    t = cloud(pts)
    q = cloud([[float(xq), 0.0, 0.0]])
    info = dict(c=c, delta=delta, gap=gap, inv_h=inv_h, h64=h64, iA=len(t) - 2, iP=len(t) - 1, b_plain=b_plain)
    return q, t, info
