"""shared inputs of the Generalized-ICP tests (tests/test_gicp_host.py on the CPU, tests/test_gpu_gicp.py and
tests/test_gpu_gicp_cases.py on the GPU).  Sizes answer
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


# ------------------------------------------------------------------ the branch cases (tests/test_gpu_gicp_cases.py)
#
# The list cases above all take one path through G7: accepts only, ended by the step tolerance.  Each branch case is the source,
# the normals and the list of a list case (rand_257 unless the name says otherwise) with a target of its own, rounded to f32
# before anything sees it, built so that the reference takes another path.  What each is for is stated in BRANCH and asserted
# on the reference alone by tests/test_gicp_host.py:
#   pattern   a regular expression the string of decisions (A accept, R reject) matches in full
#   end       "tol" (an accepted step below both tolerances), "cap" (max_inner_iterations), "lambda" (> 1e9), "singular"
#   evals     the evaluation count, where it is a fixed number
#   rejects   the number of rejects
#   undecided the evaluations whose decision MAY be undecided (gicp_ref.decided); every other one is decided.  "last": the last
#             one.  No case's first decision (evaluation 2) is among them.
#   small_arm the last accepted step has |w| < 1e-8: the candidate comes from the small-angle arm of G6's Rodrigues matrix
FAR_DIR = (0.61, -0.52, 0.6)
BRANCH = {
    "exact_fit": dict(pattern="R{13}", end="lambda", evals=14, rejects=13, undecided=()),
    "exact_shift": dict(pattern="A{6}", end="tol", evals=7, rejects=0, undecided=(), small_arm=True),
    "turn_0.1": dict(pattern="AARA+", end="tol", evals=10, rejects=1, undecided=("last",)),
    "turn_0.3": dict(pattern="(AR){9}A", end="cap", evals=20, rejects=9, undecided=()),
    "turn_0.3_long": dict(pattern="(AR){11}A(AR){2}A{6}", end="tol", evals=34, rejects=13, undecided=("last",), max_inner=60),
    "turn_0.3_65": dict(pattern="(AR){3}A(AR){6}", end="cap", evals=20, rejects=9, undecided=()),
    "turn_0.3_6001": dict(pattern="(AR){9}A", end="cap", evals=20, rejects=9, undecided=()),
    "far_1e4": dict(pattern="A{8}RRA", end="tol", evals=12, rejects=2, undecided=(9, 10, 11, 12)),
    "far_1e5": dict(pattern="A{5}(RA){7}", end="cap", evals=20, rejects=7, undecided=()),
    "three_targets": dict(pattern="(AR){9}A", end="cap", evals=20, rejects=9, undecided=()),
    "coplanar": dict(pattern="A+", end="tol", rejects=0, undecided=()),
    "collinear": dict(pattern="A+", end="tol", rejects=0, undecided=()),
    "collinear_origin": dict(pattern="", end="singular", evals=1, rejects=0, undecided=()),
    "all_equal_away": dict(pattern="AAA", end="tol", evals=4, rejects=0, undecided=()),
    "nan_point": dict(pattern="", end="singular", evals=1, rejects=0, undecided=()),
    "inf_target": dict(pattern="", end="singular", evals=1, rejects=0, undecided=()),
}
BRANCH_NAMES = tuple(BRANCH)
FAR_FRAMES = ("far_1e4", "far_1e5")                       # only TRANS_TOL on the displacement applies to these
# turn_0.3_long is turn_0.3 with max_inner_iterations = 60: the run then ends by the tolerance, after 34 evaluations
# the old list cases: all accepts, ended by the tolerance; at most their last LIST_UNDECIDED_TAIL decisions are undecided
LIST_UNDECIDED_TAIL = 2


def _base(name):
    base = {"turn_0.3_65": "rand_65", "turn_0.3_6001": "rand_6001"}.get(name, "rand_257")
    c = list_case(base)
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _set_target(c, pts):
    """the target whose point match[k] is pts[query[k]] (pts: one per SOURCE point, f64), rounded to f32"""
    perm = np.empty(len(c["src"]), np.int64)
    perm[c["query"]] = c["match"]
    tgt = np.ones((len(c["tgt"]), 4), F32)
    tgt[perm, :3] = np.asarray(pts, np.float64).astype(F32)
    c["tgt"] = tgt
    return c


def _moved(P, T):
    return P @ T[:3, :3].T + T[:3, 3]


def _turn(name, angle):
    c = _base(name)
    P = c["src"][:, :3].astype(np.float64)
    c["T"] = small_motion(np.random.default_rng(5), angle=angle, shift=1.0, centre=P.mean(0))
    return _set_target(c, _moved(P, c["T"]))


def _far(c, dist):
    """the pair moved by dist * FAR_DIR, each side rounded to f32"""
    off = dist * np.array(FAR_DIR)
    for key in ("src", "tgt"):
        c[key][:, :3] = (c[key][:, :3].astype(np.float64) + off).astype(F32)
    return c


def _flat(name):
    c = _base(name)
    P = c["src"][:, :3].astype(np.float64)
    # coplanar is fragile: its smallest decided margin is 1.32e-9 against the 1e-9 of gicp_ref.decided (the last decision, at
    # f = 6.5e-10).  A change to the reference's arithmetic can tip it to undecided; tests/test_gicp_host.py then fails, loudly.
    if name == "coplanar":                                # flattened to its own mean z: still some 900 units off the origin
        P[:, 2] = P[:, 2].mean()
    elif name == "collinear":                              # projected on the line through its own mean along x
        P[:, 1:] = P[:, 1:].mean(0)
    else:                                                  # collinear_origin: on the x axis, so that H[0][0] is exactly 0
        P = np.stack([P[:, 0], np.zeros(len(P)), np.zeros(len(P))], axis=1)
    c["src"][:, :3] = P.astype(F32)
    return _set_target(c, _moved(c["src"][:, :3].astype(np.float64), small_motion(np.random.default_rng(4))))


def branch_case(name):
    if ("branch", name) in _lists:
        return _lists["branch", name]
    if name == "turn_0.3_long":
        c = branch_case("turn_0.3")
    elif name.startswith("turn_"):
        c = _turn(name, float(name.split("_")[1]))
    elif name in ("coplanar", "collinear", "collinear_origin"):
        c = _flat(name)
    else:
        c = _base(name)
        P = c["src"][:, :3].astype(np.float64)
        if name == "exact_fit":
            _set_target(c, P)
        elif name == "exact_shift":
            _set_target(c, P + np.array([0.25, -0.5, 1.0]))
        elif name.startswith("far_"):
            _far(c, float(name.split("_")[1]))
        elif name == "three_targets":
            c["match"] = (np.arange(len(c["query"])) % 3).astype(np.int32)
        elif name == "all_equal_away":
            c["src"][:, :3] = c["src"][0, :3]
            _set_target(c, c["src"][:, :3].astype(np.float64) + 0.5)
        elif name == "nan_point":
            c["src"][c["query"][7], 1] = np.nan
        elif name == "inf_target":
            c["tgt"][c["match"][7], 1] = np.inf
        else:
            raise KeyError(name)
    _lists["branch", name] = c
    return c


def unlisted_nan():
    """`half` with a NaN in source points the list does not name: (the case, the same with the NaNs)"""
    c = list_case("half")
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    free = np.setdiff1d(np.arange(len(c["src"])), c["query"])
    assert len(free) >= 100
    d["src"][free[3], 1] = np.nan
    d["src"][free[40], :3] = np.nan
    d["src"][free[41], 0] = np.inf
    return c, d


UNIT_SCALES = (2.0 ** -30, 2.0 ** -10, 2.0 ** 10, 2.0 ** 30)
UNIT_CASES = ("rand_257", "turn_0.3")


def branch_params(name, **kw):
    """the keyword arguments of the case's run: the defaults, but for turn_0.3_long"""
    if "max_inner" in BRANCH[name]:
        kw.setdefault("max_inner_iterations", BRANCH[name]["max_inner"])
    return kw


_runs = {}


def reference_run(name, eps=1e-3):
    """(X, info, status, log) of gicp_ref.solve on a branch or a list case, at the case's parameters; computed once, not to be
    written to"""
    import gicp_ref as G
    if (name, eps) not in _runs:
        kw = branch_params(name, gicp_epsilon=eps) if name in BRANCH else dict(gicp_epsilon=eps)
        log = []
        X, info, status = G.solve(*gathered(any_case(name)), G.params(**kw), log=log)
        _runs[name, eps] = (X, info, status, log)
    return _runs[name, eps]


def state_after(log, k):
    """the reference's state after k evaluations -> (X, lambda, accepted)"""
    if k == 1:
        return np.eye(4), 1e-3, 0
    e = log[k - 2]
    return e["X"], e["lam_after"], e["accepted"]


def decided_prefix(log):
    """the number of evaluations up to which every decision is decided (1: not even the first decision is)"""
    k = 1
    for e in log:
        if not e["decided"]:
            break
        k += 1
    return k


def any_case(name):
    return branch_case(name) if name in BRANCH else list_case(name)


def in_unit(c, s):
    """the case with both clouds times s, a power of two (mls_cases.scaled asserts that this is exact in f32)"""
    import mls_cases as MC
    d = dict(c)
    d["src"], d["tgt"] = MC.scaled(c["src"], s), MC.scaled(c["tgt"], s)
    return d


def gathered(c):
    """(p, s, q, n) float64 (m, 3): the list's points and normals"""
    q, m = c["query"], c["match"]
    return (c["src"][q, :3].astype(np.float64), c["snrm"][q, :3].astype(np.float64), c["tgt"][m, :3].astype(np.float64),
            c["tnrm"][m, :3].astype(np.float64))


def sums_pose(seed=50):
    """a non-trivial X for the sums: a rotation of 0.3 rad about the clouds' centre and a shift of a few units"""
    return small_motion(np.random.default_rng(seed), angle=0.3, shift=3.0)
