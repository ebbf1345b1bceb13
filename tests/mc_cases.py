"""the small clouds the marching-cubes tests share (tests/test_mc_host.py, tests/test_gpu_mc.py, tests/test_gpu_mc_cxx.py): each
the smallest input at which the mistake it is after shows; (points f32[n, 3], normals f32[n, 3])"""
import numpy as np

import mc_ref as R

F32 = np.float32


def sphere(n=2000, radius=50.0, centre=(3.0, -7.0, 900.0), seed=5):
    """points on a sphere with their analytic outward normals"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return (u * radius + np.asarray(centre)).astype(F32), u.astype(F32)


def plane_patch(n=200, seed=11):
    """a tilted plane patch: no axis of the lattice is special, and the three extents differ"""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.3, -0.5, 0.81])
    nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    uv = rng.uniform(-1.0, 1.0, (n, 2)) * [40.0, 25.0]
    p = uv[:, :1] * a + uv[:, 1:] * b + [10.0, 20.0, 500.0]
    return p.astype(F32), np.tile(nrm.astype(F32), (n, 1))


def one_cell(targets, limit=200000):
    """for res (2, 2, 2): eight random points with random unit normals per wanted cube index -- seeds are tried in order until the
    reference's one cell has that index; {cube: (points, normals)}"""
    found = {}
    for seed in range(limit):
        rng = np.random.default_rng(seed)
        p = rng.uniform(0.0, 1.0, (8, 3)).astype(F32)
        n = rng.standard_normal((8, 3))
        n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F32)
        grid = R.values(p, n, (2, 2, 2))[0]
        cube = int(sum((grid[tuple(o)] < 0) << i for i, o in enumerate(R.OFF)))
        if cube in targets and cube not in found:
            found[cube] = (p, n)
            if len(found) == len(targets):
                return found
    raise AssertionError("no seed below %d gives the cubes %s" % (limit, sorted(set(targets) - set(found))))


def flat(n=300, seed=3):
    """all z equal (rule M15): a wavy line's worth of normals in the x-y plane"""
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3))
    p[:, :2] = rng.uniform(-20.0, 20.0, (n, 2))
    p[:, 2] = 7.5
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    return p.astype(F32), np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1).astype(F32)


def read_ply(path):
    """an independent reader of the files io::savePLYFile writes: (vertices f32[n, 3], faces list of lists)"""
    lines = open(path).read().split("\n")
    end = lines.index("end_header")
    nv = int([ln for ln in lines[:end] if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in lines[:end] if ln.startswith("element face")][0].split()[2])
    body = lines[end + 1:]
    v = np.array([[F32(x) for x in ln.split()] for ln in body[:nv]], F32).reshape(nv, 3)
    f = [[int(x) for x in ln.split()][1:] for ln in body[nv:nv + nf]]
    return v, f
