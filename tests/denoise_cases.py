"""The case table of tests/test_gpu_denoise_cases.py: adversarial clouds for mvr_cloud_denoise (csrc/mvr_denoise.hip), whose
answers come from tests/denoise_ref.py (brute force, no grid) or from a closed form.  tests/test_denoise_cases_host.py proves
on the references alone what is stated here.

A Case holds
  pts         (n, 4) f32
  radii       {tag: triangle_length}
  thresholds  the segment_thresholds run at every radius; `extra` lists (tag, threshold) calls on top (0 and -3: keep all)
  ties        the tags at which some pair lies at d == r, or one ulp of r away, ON PURPOSE (no margin is asked there)
  finite      every x, y, z is finite: oracle.denoise may referee too (it is never handed another cloud)
  kind        walk_cases' kind of the geometry, or None
  closed      {tag: (n_components, {threshold: kept indices})} where the answer is known without any search
  brute       False for the 20 000-point chains: 2e8 pairs each; the closed form is the expectation
  twice       run every call twice on a fresh upload: the union order is racy, the answer must not be

Sections (the letters of DESIGN.md 24):
  a  the target of every name of walk_cases.NAMES at every radius of walk_cases.radii (a fraction of a cell, several cells,
     beyond the whole cloud, one whose square underflows: exact duplicates only), plus `partial` where none of those leaves
     0 < kept < n with two kept components (PARTIAL_R)
  b  knife edges, each at r and at nextafter(r, 0): the cell edge is r * 1.000001, so a lattice drifts against the cells and
     pairs at exactly r straddle faces, edges and corners
  c  union-find shapes with closed-form answers
  d  grid edges
  e  non-finite input, by the rule alone"""
import numpy as np

import walk_cases as W

F32 = np.float32
INF = float("inf")


class Case:
    def __init__(self, name, section, pts, radii, thresholds=None, extra=(), ties=(), kind=None, closed=None, brute=True, twice=False):
        self.name, self.section, self.pts = name, section, np.ascontiguousarray(pts, F32)
        n = len(self.pts)
        self.radii = dict(radii)
        self.thresholds = tuple(thresholds) if thresholds is not None else (1, 2, 4, 10, n, n + 1)
        self.extra, self.ties, self.kind = tuple(extra), frozenset(ties), kind
        self.closed, self.brute, self.twice = closed or {}, brute, twice
        self.finite = bool(np.isfinite(self.pts[:, :3]).all())

    def calls(self):
        """every (tag, radius, threshold) of the case"""
        out = [(tag, r, thr) for tag, r in self.radii.items() for thr in self.thresholds]
        return out + [(tag, self.radii[tag], thr) for tag, thr in self.extra]


def below(r):
    return float(np.nextafter(np.float64(r), 0.0))


def edge(r):
    return {"at": float(r), "below": below(r)}


# Section a: one more radius for the cases where no radius of walk_cases.radii keeps a proper subset in two or more components:
# between the second and third smallest pair distance of size_5 (components of 2, 2 and 1 points), about the median distance
# to the nearest neighbour in two_far_clusters (2 400 components of mixed size); the same radius on clusters_and_a_far_point,
# whose other radii are multiples of extent / 512 (here extent / r = 5.6e5: cells 540 times the radius).  NO_PARTIAL: the cases where no radius and
# threshold can (the host test asserts each reason).
PARTIAL_R = {"size_5": 5.66, "two_far_clusters": 0.18, "clusters_and_a_far_point": 0.18}
NO_PARTIAL = {
    "lattice_3d": "every point has a neighbour at one step: singletons below the step, one component from it on",
    "size_3": "n < 5: two kept components and a dropped point need sizes (2, 2, 1) at least",
    "size_4": "n < 5: two kept components and a dropped point need sizes (2, 2, 1) at least",
}


def walk_case(name, mvr):
    t = W.get(name, mvr)[1]
    radii = W.radii(name, t)
    ties = [tag for tag in radii if tag.startswith("lattice_")]
    if name in PARTIAL_R:
        radii["partial"] = PARTIAL_R[name]
    first = next(iter(radii))
    return Case(name, "a", t, radii, extra=((first, 0), (first, -3)), ties=ties, kind=W.TABLE[name][0])


def unit_lattice():
    """the 16 x 15 x 14 lattice of walk_cases.lattice() in steps of 1, as integers"""
    return np.stack(np.meshgrid(np.arange(16), np.arange(15), np.arange(14), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)


def knife_edges(mvr):
    lat = W.get("lattice_3d", mvr)[1]
    g = unit_lattice()
    half = lat[(g.sum(1) % 2) == 0]                      # face-centred: nearest distance sqrt(2) steps, d^2 = 0.125 exactly
    far = W.moved(W.cloud(g), 1.0e6)                     # FAR_DIR * 1e6 is a vector of integers: every coordinate stays an integer below 2^24
    n, nh = len(lat), len(half)

    def one_or_all(m):
        return {"at": closed_from_groups(m, [np.arange(m)]), "below": closed_from_groups(m, [[i] for i in range(m)])}
    return [
        Case("lattice_3d_edge", "b", lat, edge(W.LATTICE_STEP), ties=("at", "below"), closed=one_or_all(n)),
        Case("lattice_fcc_half", "b", half, edge(np.sqrt(0.125)), ties=("at", "below"), closed=one_or_all(nh)),
        Case("grid_midpoints_edge", "b", W.get("regular_grid_midpoints", mvr)[1], edge(1.0), ties=("at", "below"), closed=one_or_all(1600)),
        Case("lattice_far_1e6", "b", far, edge(1.0), ties=("at", "below"), closed=one_or_all(n)),
    ]


CHAIN_N = 20000
CHAIN_ORDERS = ("ascending", "descending", "permuted", "bit_reversed", "evens_then_odds")


def chain_order(order, n):
    """position on the line of the point with index i"""
    k = np.arange(n)
    if order == "ascending":
        return k
    if order == "descending":
        return k[::-1].copy()
    if order == "permuted":
        return np.random.default_rng(51).permutation(n)
    if order == "bit_reversed":                             # the positions sorted by their bit-reversed value: neighbours far apart by index
        bits = int(n - 1).bit_length()
        rev = np.zeros(n, np.int64)
        for b in range(bits):
            rev |= ((k >> b) & 1) << (bits - 1 - b)
        return np.argsort(rev, kind="stable")
    if order == "evens_then_odds":
        return np.concatenate([k[::2], k[1::2]])
    raise KeyError(order)


def closed_from_groups(n, groups):
    """(n_components, {threshold: keep}) of a cloud whose components are the index sets `groups`"""
    groups = sorted((np.sort(np.asarray(g)) for g in groups), key=lambda g: g[0])
    sizes = sorted({len(g) for g in groups})
    thr = {1, n + 1} | set(sizes) | {s + 1 for s in sizes}
    return len(groups), {t: np.concatenate([g for g in groups if len(g) >= t] + [np.arange(0)]).astype(np.int64) for t in sorted(thr)}


def chain(order, n=CHAIN_N, cut=None):
    """n points at spacing 1 on a line, r = 1; with `cut` the point at that position is left out (two components)"""
    pos = chain_order(order, n)
    if cut is not None:
        pos = pos[pos != cut]
    m = len(pos)
    pts = W.cloud(np.c_[pos.astype(np.float64), np.zeros(m), np.full(m, 900.0)])
    idx = np.arange(m)
    groups = [idx] if cut is None else [idx[pos < cut], idx[pos > cut]]
    ncomp, keeps = closed_from_groups(m, groups)
    name = "chain_%s%s_%d" % (order, "" if cut is None else "_cut", n)
    return Case(name, "c", pts, {"at": 1.0}, thresholds=sorted(keeps), ties=("at",), closed={"at": (ncomp, keeps)}, brute=n <= 6001, twice=True)


def shapes(mvr):
    out = []
    for order in CHAIN_ORDERS:
        out += [chain(order), chain(order, cut=CHAIN_N // 3)]
    rng = np.random.default_rng(52)
    # star: 4 097 points within r / 2 of a centre that has the highest index -- every pair is linked, every thread hooks the same root
    d = rng.standard_normal((4097, 3))
    d *= (rng.uniform(0.05, 0.49, 4097) / np.linalg.norm(d, axis=1))[:, None]
    star = W.cloud(np.concatenate([d + [3.0, -2.0, 900.0], [[3.0, -2.0, 900.0]]]))
    out.append(Case("star_4097", "c", star, {"r1": 1.0}, closed={"r1": closed_from_groups(4098, [np.arange(4098)])}, twice=True))
    # bridge: two 10 x 10 x 20 blobs (step 0.5, jittered by 0.05; r = 1), 1.8 apart, joined only through the last point
    b = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(20), indexing="ij"), -1).reshape(-1, 3) * 0.5
    a = b + rng.uniform(-0.05, 0.05, b.shape)
    c = b + rng.uniform(-0.05, 0.05, b.shape) + [4.5 + 1.9, 0.0, 0.0]                  # nearest faces: 1.9 - 0.1 apart at least
    perm = rng.permutation(4000)
    xyz = np.concatenate([a, c])[perm] + [0.0, 0.0, 900.0]
    in_a = np.flatnonzero(perm < 2000)
    in_c = np.flatnonzero(perm >= 2000)
    mid = [[4.5 + 0.95, 2.0, 905.0]]                                                     # 0.95 + 0.05 from a lattice point of either blob at most
    out.append(Case("bridge_with", "c", W.cloud(np.concatenate([xyz, mid])), {"r1": 1.0}, thresholds=(1, 2000, 2001, 4001, 4002),
                    closed={"r1": closed_from_groups(4001, [np.arange(4001)])}, twice=True))
    out.append(Case("bridge_without", "c", W.cloud(xyz), {"r1": 1.0}, thresholds=(1, 2000, 2001, 4000, 4001),
                    closed={"r1": closed_from_groups(4000, [in_a, in_c])}, twice=True))
    # 3 000 two-point components, centres on a lattice of pitch 10, indices permuted; the order comes from the reference
    centres = np.stack(np.meshgrid(np.arange(15), np.arange(15), np.arange(14), indexing="ij"), -1).reshape(-1, 3)[:3000] * 10.0
    o = rng.standard_normal((3000, 3))
    o *= (rng.uniform(0.1, 0.45, 3000) / np.linalg.norm(o, axis=1))[:, None]
    pairs = np.concatenate([centres - o, centres + o])[rng.permutation(6000)] + [0.0, 0.0, 900.0]
    out.append(Case("pairs_3000", "c", W.cloud(pairs), {"r1": 1.0}, thresholds=(1, 2, 3), twice=True))
    # a 64 x 64 sheet, step 1 = r, indices permuted
    s = np.stack(np.meshgrid(np.arange(64.0), np.arange(64.0), [900.0], indexing="ij"), -1).reshape(-1, 3)[rng.permutation(4096)]
    out.append(Case("sheet_64x64_permuted", "c", W.cloud(s), edge(1.0), ties=("at", "below"), twice=True,
                    closed={"at": closed_from_groups(4096, [np.arange(4096)]), "below": closed_from_groups(4096, [[i] for i in range(4096)])}))
    # sizes 1 and 2 (63 ... 1 025 are the size_* cases of section a): the head of size_3's target
    t3 = W.get("size_3", mvr)[1]
    for n in (1, 2):
        out.append(Case("size_%d" % n, "c", t3[:n], W.radii("size_%d" % n, t3[:n]), extra=(("whole_cloud", 0), ("whole_cloud", -3)), twice=True))
    return out


def bbox_corners(L):
    """a point on each corner of [0, L]^3 and a neighbour exactly 1 inside it, along x, y or z in turn"""
    xyz = []
    for c in range(8):
        p = np.array([(c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1], np.float64) * L
        q = p.copy()
        q[c % 3] += 1.0 if p[c % 3] == 0 else -1.0
        xyz += [p, q]
    return W.cloud(np.array(xyz))


def grid_edges(mvr):
    out = []
    for L in (100.0, 4096.0):                                 # cells of r * 1.000001, and extent / r > 1023: cells of 4.004 r
        groups = [[2 * c, 2 * c + 1] for c in range(8)]
        out.append(Case("bbox_corners_%d" % L, "d", bbox_corners(L), edge(1.0), thresholds=(1, 2, 3), ties=("at", "below"),
                        closed={"at": closed_from_groups(16, groups), "below": closed_from_groups(16, [[i] for i in range(16)])}))
    t = W.get("every_target_duplicated", mvr)[1]               # t[i] == t[5999 - i]
    out.append(Case("duplicated_r_zero", "d", t, {"zero": 0.0}, thresholds=(1, 2, 3, 6000), ties=("zero",),
                    closed={"zero": closed_from_groups(6000, [[i, 5999 - i] for i in range(3000)])}))
    for name in ("patch_at_0", "lattice_3d", "huge_coordinates"):      # one cell holds the cloud: the union pass is all pairs
        t = W.get(name, mvr)[1]
        radii = {"inf": INF} if len(t) > 4000 else {"inf": INF, "f64_max": 1.7e308}
        out.append(Case(name + "_r_inf", "d", t, radii, closed={"inf": closed_from_groups(len(t), [np.arange(len(t))])}))
    return out


def sprinkle(p, mode, seed):
    """NaN, +inf and -inf in turn over 1 % of the points: in one coordinate (`one`) or in all three (`all`)"""
    rng = np.random.default_rng(seed)
    out = p.copy()
    which = rng.choice(len(p), max(3, len(p) // 100), replace=False)
    vals = np.array([np.nan, np.inf, -np.inf], F32)
    for k, i in enumerate(which):
        if mode == "one":
            out[i, rng.integers(3)] = vals[k % 3]
        else:
            out[i, :3] = vals[k % 3]
    return out


def non_finite(mvr):
    out = []
    patch, lat = W.get("patch_at_0", mvr)[1], W.get("lattice_3d", mvr)[1]
    pr = W.radii("patch_at_0", patch)
    patch_r = {"fraction_of_a_cell": pr["fraction_of_a_cell"], "several_cells": pr["several_cells"], "whole_cloud": pr["whole_cloud"], "inf": INF}
    lat_r = {"at": W.LATTICE_STEP, "below": below(W.LATTICE_STEP), "whole_cloud": W.radii("lattice_3d", lat)["whole_cloud"], "inf": INF}
    if "patch_at_0" in PARTIAL_R:
        patch_r["partial"] = PARTIAL_R["patch_at_0"]
    for k, mode in enumerate(("one", "all")):
        out.append(Case("patch_sprinkled_" + mode, "e", sprinkle(patch, mode, 60 + k), patch_r, kind="surface"))
        out.append(Case("lattice_sprinkled_" + mode, "e", sprinkle(lat, mode, 62 + k), lat_r, ties=("at", "below")))
    # two blobs 1.4 apart (r = 1) in the cells 0 and 1 of the grid: a NaN coordinate falls into cell 0 and a NaN distance is not
    # > r, so without the rule the NaN points link both blobs (and the third, 1.4 further on, through cell 1)
    rng = np.random.default_rng(64)
    blob = rng.uniform(0.0, 0.1, (3, 50, 3)) + np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [3.0, 0.0, 0.0]])[:, None, :]
    glue = W.cloud(np.concatenate([blob[0], [[np.nan, 0.05, 0.05]], blob[1], [[np.nan] * 3], blob[2], [[0.8, np.nan, 0.05], [np.inf, 0.05, 0.05]]]))
    out.append(Case("nan_between_components", "e", glue, {"r1": 1.0, "inf": INF}, thresholds=(1, 2, 50, 51, 150, 151)))
    nan = np.full((300, 3), np.nan)
    out.append(Case("all_nan", "e", W.cloud(nan), {"r1": 1.0, "zero": 0.0, "inf": INF}, thresholds=(1, 2, 300)))
    nan[137] = [1.0, 2.0, 900.0]
    out.append(Case("one_finite_among_nan", "e", W.cloud(nan), {"r1": 1.0, "zero": 0.0, "inf": INF}, thresholds=(1, 2, 300)))
    two = np.concatenate([blob[0], [[np.inf] * 3, [np.inf] * 3, [-np.inf, np.inf, 0.0], [-np.inf, np.inf, 0.0]]])
    out.append(Case("equal_inf_points", "e", W.cloud(two), {"r1": 1.0, "zero": 0.0, "inf": INF}, thresholds=(1, 2, 50, 51)))
    w = patch.copy()                                           # a non-finite w alone is NOT a non-finite point
    w[::7, 3] = np.nan
    w[3::11, 3] = np.inf
    out.append(Case("patch_non_finite_w", "e", w, {t: pr[t] for t in ("fraction_of_a_cell", "several_cells")}, kind="surface"))
    return out


_cache = {}

# every case by name, known without building one (the tests are parametrised over it; all_cases() asserts it is the table)
NAMES = list(W.NAMES) + ["lattice_3d_edge", "lattice_fcc_half", "grid_midpoints_edge", "lattice_far_1e6"] \
    + ["chain_%s%s_%d" % (o, c, CHAIN_N) for o in CHAIN_ORDERS for c in ("", "_cut")] \
    + ["star_4097", "bridge_with", "bridge_without", "pairs_3000", "sheet_64x64_permuted", "size_1", "size_2"] \
    + ["bbox_corners_100", "bbox_corners_4096", "duplicated_r_zero"] \
    + [n + "_r_inf" for n in ("patch_at_0", "lattice_3d", "huge_coordinates")] \
    + ["patch_sprinkled_one", "lattice_sprinkled_one", "patch_sprinkled_all", "lattice_sprinkled_all", "nan_between_components", "all_nan",
       "one_finite_among_nan", "equal_inf_points", "patch_non_finite_w"]


def all_cases(mvr):
    if "cases" not in _cache:
        cs = [walk_case(name, mvr) for name in W.NAMES] + knife_edges(mvr) + shapes(mvr) + grid_edges(mvr) + non_finite(mvr)
        assert [c.name for c in cs] == NAMES
        _cache["cases"] = {c.name: c for c in cs}
    return _cache["cases"]


def reference(case, margins=False):
    """{tag: (label, n_components, margin)} by brute force, computed once per case and shared"""
    import denoise_ref as R
    key = ("ref", case.name, margins)
    if key not in _cache:
        got = R.components(case.pts, list(case.radii.values()), margins=margins)
        _cache[key] = {tag: got[float(r)] for tag, r in case.radii.items()}
    return _cache[key]
