"""The inputs the ISS keypoint tests share (tests/test_gpu_iss.py compares the GPU on them, tests/test_iss_host.py checks on the
reference alone that the conditions of an exact comparison hold).  Every case is a dict(p = points [n, 4], salient_radius,
non_max_radius, gamma_21, gamma_32, min_neighbors, exact = whether keypoints and saliency flags are compared with the
reference's exactly).  The references (tests/iss_ref.py) are computed once per process and shared."""
import numpy as np

import fpfh_cases as FC
import iss_ref as R
import mls_cases as K
import walk_cases as W

VIEW_N, VIEW_SALIENT, VIEW_NON_MAX = 20000, 4.0, 2.5
# a second parameter set on the view at which BOTH thresholds reject a visible share of the points (at PCL's defaults e3 / e2
# never exceeds 0.09 on a scanned surface, so gamma_32 never rejects): chosen on the reference alone -- gamma_21 rejects 4 233
# points, gamma_32 another 1 504, 14 263 stay salient and 1 734 are keypoints; the closest ratio is 2.8e-6 from its threshold
VIEW_TIGHT = dict(gamma_21=0.8, gamma_32=0.015)
DEFAULTS = dict(gamma_21=0.975, gamma_32=0.975, min_neighbors=5)

EXACT = ("view", "view_tight", "box", "non_finite")
# the targets of the walk cases (fpfh_cases.WALK): salient radius `several cells`, non-maximum radius 0.6 of it; the two cluster
# cases 1.0 / 0.5 mm (their grid edge spans the gap between the clusters).  None is compared exactly: tests/test_iss_host.py
# records what the reference decides on each
WALK = FC.WALK
WALK_NON_MAX = 0.6
WALK_RADII_MM = {"clusters_and_a_far_point": (1.0, 0.5), "two_far_clusters": (1.0, 0.5)}
# every_target_duplicated at `several cells` (3.5 edges) has 20 balls of 6 points that are 3 distinct ones twice: a scatter of
# rank 2, whose e3 is rounding, and the reference calls 8 of them salient on that rounding alone.  At 5 edges the smallest ball
# holds 10 points and every point is decided (tests/test_iss_host.py)
WALK_RADII_CELLS = {"every_target_duplicated": 5.0}
NAMES = EXACT + tuple("tiny_%d" % n for n in FC.TINY_SIZES) + ("duplicates",) + FC.DEGENERATE + WALK
FMA_CASES = ("box", "non_finite", "duplicates")           # run a second time with the fma distance

_cache = {}


def case(name, mvr):
    if name in ("view", "view_tight"):
        c = dict(p=FC.view(mvr, VIEW_N), salient_radius=VIEW_SALIENT, non_max_radius=VIEW_NON_MAX, **DEFAULTS)
        if name == "view_tight":
            c.update(VIEW_TIGHT)
    elif name == "box":
        p, _, r = FC.box()                               # 3000 points in a 20 mm box: about 37 in a ball of 3 mm
        c = dict(p=p, salient_radius=r, non_max_radius=2.0, **DEFAULTS)
    elif name == "non_finite":
        p = K.with_non_finite(FC.view(mvr, 6000))[0]
        c = dict(p=p, salient_radius=8.0, non_max_radius=5.0, **DEFAULTS)
    elif name.startswith("tiny_"):
        p, _, r = FC.tiny(int(name[5:]))                 # every point alone: counts of 1
        c = dict(p=p, salient_radius=r, non_max_radius=r, **DEFAULTS)
    elif name == "duplicates":
        p, _, r = FC.duplicates()
        c = dict(p=p, salient_radius=r, non_max_radius=0.75 * r, **DEFAULTS)
    elif name in FC.DEGENERATE:
        p, _, r = FC.degenerate(name, mvr)
        c = dict(p=p, salient_radius=r, non_max_radius=r, **DEFAULTS)
    elif name in WALK:
        p = W.get(name, mvr)[1]
        cells = float(WALK_RADII_CELLS[name] * W.grid_edge(p)) if name in WALK_RADII_CELLS else float(W.radii(name, p)["several_cells"])
        r, m = WALK_RADII_MM.get(name) or (cells,) * 2
        c = dict(p=p, salient_radius=r, non_max_radius=m if name in WALK_RADII_MM else WALK_NON_MAX * r, **DEFAULTS)
    else:
        raise KeyError(name)
    c["exact"] = name in EXACT
    return c


def params(c):
    return dict(salient_radius=c["salient_radius"], non_max_radius=c["non_max_radius"], gamma_21=c["gamma_21"], gamma_32=c["gamma_32"],
                min_neighbors=c["min_neighbors"])


def reference(name, mvr, fma=False):
    """(case, iss_ref.iss of it), computed once; the two parameter sets of the view share their neighbour sets"""
    key = (name, fma)
    if key not in _cache:
        c = case(name, mvr)
        sets = _cache[("view", fma)][1]["sets"] if name == "view_tight" and ("view", fma) in _cache else None
        _cache[key] = (c, R.iss(c["p"], fma=fma, sets=sets, **params(c)))
    return _cache[key]
