"""The inputs the moving-least-squares tests share (tests/test_gpu_mls.py compares the GPU on them, tests/test_mls_host.py
checks on the reference alone that none of their points is excluded from value comparisons): synthetic views with their analytic
normals and noise-free twins, a view with scattered non-finite points, and the twelve views merged under their true poses."""
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
