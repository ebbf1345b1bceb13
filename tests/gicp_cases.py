"""shared inputs of the Generalized-ICP tests (tests/test_gicp_host.py on the CPU, tests/test_gpu_gicp.py on the GPU).  Sizes answer
to the launch shapes of csrc/mvr_gicp.hip: gicp_sums_kernel runs blocks of 256 threads (four waves of 64), one block per 256
entries of the match table up to one block per compute unit, and strides beyond that; gicp_step_kernel is one block that adds the
partial rows in 8 groups.  So 3 is the smallest list the optimiser takes, 64 / 65 a wave and a wave plus one, 257 a block plus
one (two partial rows), 6 001 is 24 rows, and big_list(CU count) = CU count x 256 + 257 entries is where a block strides twice.

ALIGN cases: the synthetic turntable scans of config 1, view 1 under the mis-calibrated prior against view 0, as
reject_cases._synth_pair makes them; normals are 20-NN normals, estimated on the GPU in the GPU test and by numpy in the host
test.  CONDITIONS, asserted by the host test on the reference with a kd-tree search: every case ends by TRANSFORM before
max_iterations; for synth_6001 the rms distance to the true pose ends at no more than half of what it starts at and at no more
than what the reference's reciprocal SVD ICP (50 iterations, the same max_dist) ends with.

LIST cases (for the sums and the solve): a source cloud from reject_cases._rand_pair, a target that is the source moved by a
small rigid motion plus noise, random unit normals, and a correspondence list in shuffled order."""
import numpy as np

import reject_cases as RC

F32 = np.float32
K_NORMALS = 20
ALIGN = {"synth_6001": dict(ns=6001, nt=6001, max_dist=4.0), "synth_2003": dict(ns=2003, nt=6001, max_dist=4.0)}
LIST_SIZES = (3, 64, 65, 257, 6001)
LIST_NAMES = tuple("rand_%d" % n for n in LIST_SIZES) + ("palette", "half")
_align, _lists = {}, {}


def align_case(mvr, name):
    """dict(src, tgt, max_dist, T_true): T_true takes the source (view 1 under the prior) onto view 0"""
    if name not in _align:
        a = ALIGN[name]
        c = dict(RC._synth_pair(mvr, a["ns"], a["nt"], config=1), max_dist=a["max_dist"])
        sp = mvr.synth_params(12, 1)
        piv, ax = mvr.synth_prior(sp)
        ang = mvr.turntable_angle(1, sp.n_views)
        true_axis = np.array(sp.axis) / np.linalg.norm(np.array(sp.axis))
        c["T_true"] = mvr.axis_rotation(np.array(sp.pivot), true_axis, ang) @ np.linalg.inv(mvr.axis_rotation(piv, ax, ang))
        _align[name] = c
    return _align[name]


def small_motion(rng, angle=0.02, shift=0.5, centre=(0.0, 0.0, 900.0)):
    w = rng.standard_normal(3)
    w *= angle / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(centre) - R @ np.asarray(centre) + rng.standard_normal(3) * shift
    return T


def unit_normals(rng, n):
    v = rng.standard_normal((n, 3))
    out = np.zeros((n, 4), F32)
    out[:, :3] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    return out


def moved_pair(seed, n, noise=0.05):
    """src, tgt = src moved + noise in shuffled order, normals, and the list that pairs them up"""
    rng = np.random.default_rng(seed)
    src = RC._rand_pair(seed, n, 1)["src"]
    T = small_motion(rng)
    perm = rng.permutation(n)
    tgt = np.ones((n, 4), F32)
    moved = src[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.standard_normal((n, 3)) * noise
    tgt[perm, :3] = moved.astype(F32)
    order = rng.permutation(n)
    return dict(src=src, tgt=tgt, snrm=unit_normals(rng, n), tnrm=unit_normals(rng, n), query=order.astype(np.int32),
                match=perm[order].astype(np.int32))


def palette_case(seed=21, n=257):
    """normals that are NaN, zero, of length 0.5 and 3, and the same on both sides (A + B then has the eigenvalue 2 eps)"""
    c = moved_pair(seed, n)
    rng = np.random.default_rng(seed + 1)
    kind_s, kind_t = rng.integers(0, 6, n), rng.integers(0, 6, n)
    for nrm, kind in ((c["snrm"], kind_s), (c["tnrm"], kind_t)):
        nrm[kind == 1, 0] = np.nan
        nrm[kind == 2, :3] = 0.0
        nrm[kind == 3, :3] *= F32(0.5)
        nrm[kind == 4, :3] *= F32(3.0)
    par = np.nonzero(rng.integers(0, 4, n) == 0)[0]                # parallel pairs: the target's normal = the source's, or its opposite
    q, m = c["query"], c["match"]
    sign = np.where(rng.integers(0, 2, len(par)) == 0, F32(1.0), F32(-1.0))[:, None]
    c["tnrm"][m[par], :3] = c["snrm"][q[par], :3] * sign
    c["kinds"] = (kind_s, kind_t, par)
    return c


def half_case(seed=22, n=514):
    """every other source point is in the list: half the entries of the device's match table are -1"""
    c = moved_pair(seed, n)
    keep = c["query"] % 2 == 1
    c["query"], c["match"] = c["query"][keep], c["match"][keep]
    return c


def list_case(name):
    if name not in _lists:
        if name == "palette":
            _lists[name] = palette_case()
        elif name == "half":
            _lists[name] = half_case()
        else:
            n = int(name.split("_")[1])
            _lists[name] = moved_pair(30 + LIST_SIZES.index(n), n)
    return _lists[name]


def big_list(n_cu):
    n = int(n_cu) * 256 + 257
    if ("big", n) not in _lists:
        _lists[("big", n)] = moved_pair(40, n)
    return _lists[("big", n)]


def gathered(c):
    """(p, s, q, n) float64 (m, 3): the list's points and normals"""
    q, m = c["query"], c["match"]
    return (c["src"][q, :3].astype(np.float64), c["snrm"][q, :3].astype(np.float64), c["tgt"][m, :3].astype(np.float64),
            c["tnrm"][m, :3].astype(np.float64))


def sums_pose(seed=50):
    """a non-trivial X for the sums: a rotation of 0.3 rad about the clouds' centre and a shift of a few units"""
    return small_motion(np.random.default_rng(seed), angle=0.3, shift=3.0)
