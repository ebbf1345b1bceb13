"""The inputs the moving-least-squares tests share (tests/test_gpu_mls.py compares the GPU on them, tests/test_mls_host.py
checks on the reference alone that none of their points is excluded from value comparisons): synthetic views with their analytic
normals and noise-free twins, a view with scattered non-finite points, and the twelve views merged under their true poses; and
the case table of tests/test_gpu_mls_cases.py: the walk cases of tests/walk_cases.py at their radii, with the caps on the share the
reference may exclude, the sampled rows, the scales of the unit-of-length test and its preconditions."""
import numpy as np

F32, F64 = np.float32, np.float64


def synth(mvr, view, n, config=3):
    """(points, analytic normals, noise-free twins) of one synthetic view: the generator draws its noise after it has accepted a
    sample, so the same seed with noise_sigma = 0 gives the twin of every point"""
    sp = mvr.synth_params(12, config)
    p, nr = mvr.synth_view(sp, view, n, normals=True)
    sp0 = mvr.synth_params(12, config)
    sp0.noise_sigma = 0.0
    return p, nr, mvr.synth_view(sp0, view, n)


def with_non_finite(p, count=60, seed=5):
    """`count` scattered points get NaN, +inf or -inf in one coordinate, some in two, one in all three: (points, their indices)"""
    p = p.copy()
    rng = np.random.default_rng(seed)
    bad = rng.choice(len(p), min(count, len(p)), replace=False)
    vals = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(bad):
        p[i, j % 3] = vals[(j // 3) % 3]
    p[bad[0], :3] = np.nan
    if len(bad) > 1:
        p[bad[1], :3] = (np.inf, -np.inf, np.nan)
    return p, bad


NON_FINITE_RUNS = ((1.0, False), (2.5, True))          # (radius, fma) of the runs on the view with non-finite points


def sample_rows(n, seed, count=3000):
    return np.sort(np.random.default_rng(seed).choice(n, count, replace=False))


VIEW_SEED, MERGED_SEED = 1, 2                          # the sampled queries of the ground-truth tests


def rodrigues(axis, ang):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def surface_residual(x, pivot):
    """|p| - r(p / |p|) of the generator's object (csrc/synth.c), p taken about the pivot"""
    d = x - pivot
    r = np.linalg.norm(d, axis=1)
    a, b, c = (d / r[:, None]).T
    return r - (80.0 + 12.0 * (a ** 3 - 3 * a * b * b) + 6.0 * (2 * c ** 3 - c) + 5.0 * a * c + 4.0 * b)


def merged_object(mvr, n=200000):
    """the twelve views at n points each, posed into view 0's frame on the host in f64 under their TRUE poses:
    (points f32, analytic normals f32, noise-free twins f64)"""
    sp = mvr.synth_params(12, 3)
    pivot, axis = np.array(list(sp.pivot)), np.array(list(sp.axis))
    P, N, Cl = [], [], []
    for v in range(12):
        p, nr, clean = synth(mvr, v, n)
        Rm = rodrigues(axis, -v * 2.0 * np.pi / 12.0)
        q = np.ones_like(p)
        q[:, :3] = ((p[:, :3].astype(F64) - pivot) @ Rm.T + pivot).astype(F32)
        m = np.zeros_like(nr)
        m[:, :3] = (nr[:, :3].astype(F64) @ Rm.T).astype(F32)
        P.append(q); N.append(m); Cl.append((clean[:, :3].astype(F64) - pivot) @ Rm.T + pivot)
    P, N, Cl = np.concatenate(P), np.concatenate(N), np.concatenate(Cl)
    assert np.abs(surface_residual(Cl, pivot)).max() < 1e-3          # (the twins are f32: 6e-5 mm of rounding at |z| = 917)
    return P, N, Cl


# ------------------------------------------------------------------ the case table of tests/test_gpu_mls_cases.py
#
# Rows are (walk case, radius tag of walk_cases.radii) on the TARGET cloud of the case; zero_r2 is left out, and whole_cloud is
# taken for clouds of at most 1 100 points.  Per row and order the CAP on the share of kept points the reference may exclude
# from value comparisons (mls_ref.excluded, the unit-free rules).  A cap is a condition, set by rule from the share measured on
# the reference alone (tests/test_mls_host.py asserts it, the GPU test asserts it again before it compares anything):
#   share <= 0.0063      cap 1 %
#   above that           the share rounded up to the next 0.05
#   above 0.7            None: no value is compared, the row gets the reference-free checks only
# Every row not named below has (1 %, 1 %).  Measured (share at order 1 / order 2):
#   all_identical, collinear            1 / 1 at both radii: no plane is defined (gap 0)
#   every_target_duplicated             fraction_of_a_cell 0.81 / 1: most kept points are two or three distinct points, doubled
#   duplicates_41, fraction_of_a_cell   0.061 / 0.061 (the 41 copies: gap 0), cap 0.10 -- values ARE compared here
#   lattice_3d (cubic symmetry: the gap rule fires)
#                                       several_cells 0.393 / 0.393, lattice_distance 0.65 / 0.951, lattice_diagonal 0.65 / 0.65
#   two_far_clusters and clusters_and_a_far_point, several_cells
#                                       0 / 1: a cluster of sigma 1 mm in a ball of 385 / 684 mm.  In units of the radius the
#                                       offsets are 1e-2 and the 6 x 6 system's condition number is 2.3e10 / 2.2e11, over the bar
#                                       of 1e10; in millimetres (the rules before they were unit-free) it was under it and the
#                                       share 0.  The bar and the unit are the rule, so order 2 compares no values on these two
#                                       rows; order 1 does, and test_unit_of_length holds order 2 on one of them to exact
#                                       homogeneity.
#   huge_coordinates                    0 / 0 at both radii (1 / 1 at several_cells under the millimetre-bound rules)
# Largest share of the 1 % rows: every_target_duplicated several_cells 0.0017 / 0.0063 in full (its sample: see below),
# patch_far_1e6 fraction_of_a_cell 0.0053 / 0.0057.
CAPS = {
    ("all_identical", "fraction_of_a_cell"): (None, None),
    ("all_identical", "several_cells"): (None, None),
    ("collinear", "fraction_of_a_cell"): (None, None),
    ("collinear", "several_cells"): (None, None),
    ("every_target_duplicated", "fraction_of_a_cell"): (None, None),
    ("duplicates_41", "fraction_of_a_cell"): (0.10, 0.10),
    ("lattice_3d", "several_cells"): (0.40, 0.40),
    ("lattice_3d", "lattice_distance"): (0.65, None),
    ("lattice_3d", "lattice_diagonal"): (0.65, 0.65),
    ("two_far_clusters", "several_cells"): (0.01, None),
    ("clusters_and_a_far_point", "several_cells"): (0.01, None),
}
# The rows whose reference costs 10-16 s in full: values are compared at a seeded sample of at most SAMPLE query rows, which
# holds every point with 5, 6 or 7 neighbours; the kept set is compared in full.  The share of a sampled row is the share of
# its sample.  Forcing the sparse points in raises it: every_target_duplicated several_cells has 20 points with exactly 6
# neighbours -- three distinct points, doubled: a singular system -- and all 20 are in the sample of 400, so its order-2 share
# is 0.05 where the full row has 0.0063.
SAMPLE = 400
SAMPLED = {("two_far_clusters", "fraction_of_a_cell"), ("two_far_clusters", "several_cells"),
           ("clusters_and_a_far_point", "fraction_of_a_cell"), ("clusters_and_a_far_point", "several_cells"),
           ("duplicates_41", "several_cells"), ("every_target_duplicated", "several_cells"), ("one_query", "several_cells"),
           ("queries_far_from_everything", "several_cells")}
CAPS[("every_target_duplicated", "several_cells")] = (0.01, 0.05)
WHOLE_CLOUD_MAX = 1100
UNIT_SCALES = (2.0 ** -30, 2.0 ** -10, 2.0 ** 10, 2.0 ** 30)
UNIT_CLOUDS = ("patch_at_0", "patch_far_1e5", "size_257", "clusters_and_a_far_point")      # at several_cells
# the scales at which the box of each of these clouds falls under the 1e-6 that model_grid_size lifts an extent to: the grid is
# then not the unscaled cloud's, and the f64 sums run in another order (tests/test_mls_host.py asserts which scales these are)
GRID_MOVES = (2.0 ** -30,)


def case_rows():
    """[(walk case, radius tag)], sorted"""
    import walk_cases as W
    out = []
    for name in W.NAMES:
        tags = ["fraction_of_a_cell", "several_cells", "whole_cloud"]
        tags += {"lattice_3d": ["lattice_distance", "lattice_diagonal"], "regular_grid_midpoints": ["lattice_distance"]}.get(name, [])
        out += [(name, tag) for tag in tags]
    return out


def caps(name, tag):
    return CAPS.get((name, tag), (0.01, 0.01))


_inputs = {}


def case_input(mvr, name, tag):
    """(target cloud, radius, sampled query rows or None) of a row, or None where the row does not exist (whole_cloud on a
    cloud of more than WHOLE_CLOUD_MAX points)"""
    import mls_ref as R
    import walk_cases as W
    if (name, tag) in _inputs:
        return _inputs[name, tag]
    t = W.get(name, mvr)[1]
    r = W.radii(name, t)[tag]
    if tag == "whole_cloud" and len(t) > WHOLE_CLOUD_MAX:
        out = None
    else:
        rows = None
        if (name, tag) in SAMPLED:
            cnt = R.counts(t, r)
            must = np.nonzero((cnt >= 5) & (cnt <= 7))[0]
            rest = np.setdiff1d(np.arange(len(t)), must)
            seed = 7000 + case_rows().index((name, tag))
            pick = np.random.default_rng(seed).choice(rest, max(0, min(SAMPLE - len(must), len(rest))), replace=False)
            rows = np.sort(np.concatenate([must, pick]))
            assert len(rows) <= SAMPLE and np.isin(must, rows).all()
        out = (t, r, rows)
    _inputs[name, tag] = out
    return out


def scaled(p, s):
    """the cloud times a power of two: exact in f32 while nothing leaves the normal range (asserted)"""
    q = p.copy()
    q[:, :3] = p[:, :3] * F32(s)
    fin = np.isfinite(p[:, :3])
    back = q[:, :3].astype(F64) / s
    assert np.array_equal(back[fin], p[:, :3].astype(F64)[fin]) and np.isfinite(q[:, :3][fin]).all()
    return q


# The two widths of the weight on patch_at_0 at several_cells: sqr_gauss_param = r^2 * factor.  The narrow one sends all weights
# but the nearest few to 0 or to denormals.  Caps by the rule above, measured: see tests/test_mls_host.py.
WIDTHS = {"narrow": 1.0 / 4096.0, "wide": 4096.0}
WIDTH_CAPS = {"narrow": (0.01, None), "wide": (0.01, 0.01)}


def unit_preconditions(p, radius, s, cell_points=4):
    """what the unit-of-length test states about the cloud p and the radius, both times s, before it compares a bit:
      box_ok   every extent of the scaled box is >= 1e-6 and the cell edge lies in [1e-30, 1e30] -- the two absolute constants
               of model_grid_size (csrc/mvr_grid_size.h); away from them the grid, the walk order and so every f64 sum are those
               of the unscaled cloud
      d2_ok    no f32 square of a coordinate difference and no f32 d2 of a neighbour pair is denormal or infinite at that
               scale (a zero is neither): the f32 distance is then the unscaled one times s^2, exactly
    -> dict(box_ok, d2_ok, ext = the smallest scaled extent, edge = the scaled cell edge)"""
    import walk_cases as W
    P = p[np.isfinite(p[:, :3]).all(1), :3]
    ext = (P.max(0).astype(F64) - P.min(0).astype(F64)) * s
    edge = W.grid_edge(scaled(p, s), cell_points) if ext.min() >= 1e-6 else float("nan")
    box_ok = bool(ext.min() >= 1e-6 and 1e-30 <= edge <= 1e30)
    tiny, r2 = float(np.finfo(F32).tiny), F32(min((radius * s) ** 2, float(np.finfo(F32).max)))
    Ps = scaled(p, s)[np.isfinite(p[:, :3]).all(1), :3]
    d2_ok = bool(np.isfinite(r2) and r2 >= tiny)
    with np.errstate(over="ignore", under="ignore"):
        for c0 in range(0, len(Ps), 512):
            d = Ps[c0:c0 + 512, None, :] - Ps[None, :, :]
            sq = d * d
            d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
            near = d2 <= r2
            part = sq[near]
            d2_ok &= bool(((part == 0) | (part >= tiny)).all() and np.isfinite(d2[near]).all() and ((d2[near] == 0) | (d2[near] >= tiny)).all())
    return dict(box_ok=box_ok, d2_ok=d2_ok, ext=float(ext.min()), edge=edge)
