"""shared inputs of the plane segmentation tests (tests/test_sac_host.py on the CPU, tests/test_gpu_sac.py on the GPU) and a cache
of the reference's answers (tests/sac_ref.py).  Sizes are chosen for the launch shapes of csrc/mvr_sac.hip: a thread of the
counting kernel keeps 4 points and a block 1024, so 6001 is five full tiles and a tail, 65 and 257 are a wave / a block plus
one, and 4097 = 4 x 256 x 4 + 1 is four full tiles and a single point.  The cases keep `iterations` at least 0.01 away from k at
every stop decision (the reference asserts it), so libm's log against numpy's cannot change where a loop stops."""
import math

import numpy as np

import sac_ref as R

F32 = np.float32
PPT = 4                      # points per thread of ransac_count_kernel (kRansacPpt, csrc/mvr_ransac.h)
TILE_PLUS_ONE = 4 * 256 * PPT + 1


def _pack(xyz, rng=None):
    p = np.ones((len(xyz), 4), F32)
    p[:, :3] = np.asarray(xyz, np.float64).astype(F32)
    if rng is not None:
        p = p[rng.permutation(len(p))]
    return np.ascontiguousarray(p)


def _shell(rng, n, radius=30.0, centre=(0.0, 0.0, 42.0)):
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (radius + 0.05 * rng.standard_normal((n, 1))) + np.asarray(centre)


def _disc(rng, n, radius, normal, centre=(0.0, 0.0, 0.0), noise=0.1):
    normal = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    u = np.cross(normal, [1.0, 0.0, 0.0] if abs(normal[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(normal, u)
    r, a = radius * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
    return np.asarray(centre) + np.outer(r * np.cos(a), u) + np.outer(r * np.sin(a), v) + np.outer(noise * rng.standard_normal(n), normal)


TILT = (0.05, -0.03, 1.0)


def _platter(n_obj, n_disc, seed):
    rng = np.random.default_rng(seed)
    return _pack(np.concatenate([_shell(rng, n_obj), _disc(rng, n_disc, 70.0, TILT)]), rng)


def _lattice():
    rng = np.random.default_rng(21)
    gx, gy = np.meshgrid(np.arange(-7, 7), np.arange(-7, 7))                         # 196 points with z = 0
    plane = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1)
    off = np.stack([rng.integers(-7, 7, 61), rng.integers(-7, 7, 61), rng.integers(1, 9, 61) * rng.choice([-1, 1], 61)], 1)
    return _pack(np.concatenate([plane, off]), rng)                                  # 257


def _two_planes(n, share, seed, normal_b=(1.0, 0.2, 0.1), centre_b=(0.0, 0.0, 30.0)):
    rng = np.random.default_rng(seed)
    na = int(round(share * n))
    return _pack(np.concatenate([_disc(rng, na, 60.0, (0.0, 0.0, 1.0)), _disc(rng, n - na, 60.0, normal_b, centre_b)]), rng)


def _with_invalid(p, seed, share=0.1):
    rng = np.random.default_rng(seed)
    p = p.copy()
    bad = rng.choice(len(p), int(share * len(p)), replace=False)
    p[bad, rng.integers(0, 3, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad)).astype(F32)
    return p


def _collinear():
    k = np.arange(-25, 25, dtype=np.float64)
    return _pack(np.outer(k, [1.0, 2.0, 3.0]) + [5.0, 5.0, 5.0])                     # integers: every cross product is exactly 0


def _duplicates():
    rng = np.random.default_rng(33)
    base = np.concatenate([_disc(rng, 40, 20.0, (0.0, 0.0, 1.0), noise=0.05), _shell(rng, 20, 8.0, (0.0, 0.0, 12.0))])
    return _pack(np.repeat(base, 4, axis=0), rng)                                    # 240: every point four times


def _tiny(n):
    return _pack(np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.0, 10.0, 0.0]])[:n])


# name -> (points, keyword arguments of the call)
CASES = {
    "platter": (_platter(3000, 3001, 1), dict(threshold=0.5)),
    "mostly_object": (_platter(5000, 1001, 2), dict(threshold=0.5)),
    "mostly_object_50": (_platter(5000, 1001, 2), dict(threshold=0.5, max_iterations=50)),
    "far": (_platter(3000, 3001, 1) + np.array([1.0e4, 1.0e4, 1.0e4, 0.0], F32), dict(threshold=0.5)),
    "far_tight": (_platter(3000, 3001, 1) + np.array([1.0e4, 1.0e4, 1.0e4, 0.0], F32), dict(threshold=0.1)),
    "small": (_platter(40, 25, 3), dict(threshold=0.5)),
    "lattice": (_lattice(), dict(threshold=0.5)),
    "two_planes": (_two_planes(TILE_PLUS_ONE, 0.6, 4), dict(threshold=0.4)),
    "right_angle": (_two_planes(1500, 0.6, 5, (1.0, 0.0, 0.0), (0.0, 0.0, 40.0))[:, [2, 1, 0, 3]].copy(), dict(threshold=0.4)),
    "perpendicular": (_two_planes(1500, 0.6, 5, (1.0, 0.0, 0.0), (0.0, 0.0, 40.0))[:, [2, 1, 0, 3]].copy(),
                      dict(threshold=0.4, model=R.PERPENDICULAR, axis=(0.0, 0.0, 1.0), eps_angle=0.1)),
    "collinear": (_collinear(), dict(threshold=0.5, max_iterations=10)),
    "duplicates": (_duplicates(), dict(threshold=0.3)),
    "invalid_mixed": (_with_invalid(_platter(300, 400, 6), 7), dict(threshold=0.5)),
    "all_invalid": (np.full((40, 4), np.nan, F32), dict(threshold=0.5)),
    "n0": (np.zeros((0, 4), F32), dict(threshold=0.5)),
    "n1": (_tiny(1), dict(threshold=0.5)),
    "n2": (_tiny(2), dict(threshold=0.5)),
    "n3": (_tiny(3), dict(threshold=0.5)),
}
# right_angle / perpendicular: after the swap of x and z the larger plane (60 %) has the normal x, so it stands upright along
# the axis z, and the smaller one (40 %) has the normal z: it is the plane perpendicular to the axis
SEEDS = {"platter": (1, 2, 3)}                  # the other cases run with seed 1
FOUND = ("platter", "mostly_object", "mostly_object_50", "far", "far_tight", "small", "lattice", "two_planes", "right_angle", "perpendicular",
         "duplicates", "invalid_mixed", "n3")
REFINED = tuple(n for n in FOUND if n != "n3")   # the cases whose refinement enters the measured bar (n3: three points, a zero eigenvalue)
# far_tight: the far frame at a threshold of one sigma of the disc's noise, so that many points lie near the bound: there the fma
# chain of P5 gives other counts AND another inlier set of the best plane than the plain chain (tests/test_sac_host.py asserts it)
FMA_CASE = "far_tight"
RUNS = [(name, seed) for name in CASES for seed in SEEDS.get(name, (1,))]
IDS = ["%s-%d" % r for r in RUNS]

_ref = {}


def reference(name, seed=1, fma=False, optimize=True):
    key = (name, seed, fma, optimize)
    if key not in _ref:
        p, kw = CASES[name]
        _ref[key] = (p, kw, R.segment(p, seed=seed, fma=fma, optimize=optimize, **kw))
    return _ref[key]


def plane_of(name):
    """the constructed planes of a case: unit normals"""
    t = np.asarray(TILT) / np.linalg.norm(TILT)
    return {"platter": t, "mostly_object": t, "far": t, "small": t, "lattice": np.array([0.0, 0.0, 1.0]),
            "two_planes": np.array([0.0, 0.0, 1.0]), "right_angle": np.array([1.0, 0.0, 0.0]), "perpendicular": np.array([0.0, 0.0, 1.0])}[name]
