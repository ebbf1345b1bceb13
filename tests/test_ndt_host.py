"""CPU tests of the Normal Distributions Transform (rules N1-N12 in include/mvr_hip.h): the numpy reference tests/ndt_ref.py
against central differences and closed forms, the conditions the align cases of tests/ndt_cases.py have to meet for the GPU
tests to be decidable, and the host side of the C-ABI (constants, direction, argument errors).  No GPU here."""
import ctypes as C

import numpy as np
import pytest

import ndt_cases as NC
import ndt_ref as R


def test_constants_of_rule_n2(mvr):
    """the figures the issue's prototype measured at resolution 10, outlier ratio 0.55; the library's are the reference's"""
    d1, d2, d3 = R.constants(10.0, 0.55)
    assert d1 == -9.009791891267726 and d2 == 0.11417034083046575
    got = mvr.ndt_constants(mvr.ndt_params(resolution=10.0))
    assert np.allclose(got, (d1, d2, d3), rtol=1e-14, atol=0)
    for res, ratio in ((1.0, 0.55), (5.0, 0.3), (0.002, 0.9)):
        assert np.allclose(mvr.ndt_constants(mvr.ndt_params(resolution=res, outlier_ratio=ratio)), R.constants(res, ratio), rtol=1e-13, atol=0)


def test_default_params_are_pcls(mvr):
    p = mvr.ndt_params()
    assert (p.resolution, p.step_size, p.outlier_ratio, p.transformation_epsilon, p.max_iterations) == (1.0, 0.1, 0.55, 0.1, 35)
    assert (p.min_covar_eigvalue_mult, p.max_line_evals, p.min_points_per_voxel, tuple(p.origin)) == (0.01, 10, 6, (0.0, 0.0, 0.0))
    assert {k: (tuple(v) if k == "origin" else v) for k, v in R.DEFAULTS.items()} == \
        {f[0]: (tuple(getattr(p, f[0])) if f[0] == "origin" else getattr(p, f[0])) for f in mvr.NdtParams._fields_}


@pytest.fixture(scope="module")
def fd_case():
    case = NC.centred("res5")
    prm = R.params(**case["prm"])
    return case["src"][:300], R.build_cells(case["tgt"], prm), prm


@pytest.mark.parametrize("where", ["identity", "half", "guess"])
def test_reference_gradient_and_hessian_against_central_differences(fd_case, where):
    """g = ds/dp and H = dg/dp by central differences at h = 1e-6 on 300 points of `centred`: 1e-5 of the largest entry.  (The
    issue's prototype saw 6e-8 for g and 1.5e-7 for H; the score is smooth wherever no pair sits on the radius or on a voxel
    face within h, which the count checks.)"""
    src, cells, prm = fd_case
    p0 = {"identity": np.zeros(6), "half": 0.5 * NC.P_STAR, "guess": 0.3 * NC.P_STAR}[where]
    G = R.pose_matrix(0.5 * NC.P_STAR) if where == "guess" else None
    s0 = R.sums(src, cells, prm, p0, G)
    H, g, cnt, _ = R.unpack(s0)
    assert cnt > 300
    h = 1e-6
    g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
    for i in range(6):
        e = np.zeros(6); e[i] = h
        sp, sm = R.sums(src, cells, prm, p0 + e, G), R.sums(src, cells, prm, p0 - e, G)
        assert sp[27] == cnt and sm[27] == cnt
        g_fd[i] = (sp[28] - sm[28]) / (2 * h)
        H_fd[:, i] = (sp[21:27] - sm[21:27]) / (2 * h)
    eg, eh = np.abs(g - g_fd).max() / np.abs(g).max(), np.abs(H - H_fd).max() / np.abs(H).max()
    print("%s: g within %.2g, H within %.2g of the largest entry" % (where, eg, eh))
    assert eg <= 1e-5 and eh <= 1e-5


def test_lattice_closed_forms():
    case = NC.lattice()
    prm = R.params(**case["prm"])
    cells = R.build_cells(case["tgt"], prm)
    order = np.lexsort((case["centres"][:, 0], case["centres"][:, 1], case["centres"][:, 2]))
    assert np.array_equal(cells["mean"], case["centres"][order]) and np.array_equal(cells["count"], [8] * 5)
    assert np.abs(cells["icov"] - np.array([8 / 7, 0, 0, 8 / 7, 0, 8 / 7])).max() <= 4e-16 and not cells["inflated"].any()
    assert list(cells["key"]) == [0, 1, 3, 6, 11]              # the lattice is 3 x 2 x 2
    # the squared distances of the counted pairs, point by point (the others lie beyond the radius or outside the 27 voxels)
    pairs = [0.0, 16.0, 16.0, 16.0,          # (2, 2, 2): its own cell and three centres at exactly the resolution
             0.375, 12.375, 14.375,          # (2.5, 2.25, 1.75): (2, 2, 6) is 18.375 away
             0.5,                            # (6.5, 2.5, 2)
             3.0,                            # (9, 5, 7)
             3.0, 11.0, 11.0, 11.0]          # (3, 3, 3)
    at, beyond = R.sums(case["src"], cells, prm), R.sums(case["src"], cells, prm, case["beyond"])
    assert at[27] == len(pairs) == 13 and beyond[27] == 12
    # the score of a pair at distance r from an isotropic cell: -d1 exp(-d2 (8 / 7) r^2 / 2)
    d1, d2, _ = R.constants(4.0, 0.55)
    term = lambda q: -d1 * np.exp(-d2 * (8 / 7) * q / 2)
    want = sum(term(q) for q in pairs)
    assert abs(at[28] - want) <= 1e-13 * want and abs(beyond[28] - (want - term(16.0))) <= 1e-13 * want
    # at a cell's centre the gradient of that pair vanishes and its Hessian is d1 d2 C^-1: the point (9, 5, 7) is alone with one cell
    one = R.sums(case["src"][3:4], cells, prm)
    H, g, cnt, _ = R.unpack(one)
    dvec = np.array([-1.0, -1.0, 1.0])
    e = np.exp(-d2 * (8 / 7) * 3.0 / 2)
    assert cnt == 1 and np.abs(g[:3] - d1 * d2 * e * (8 / 7) * dvec).max() <= 1e-14
    assert np.abs(H[:3, :3] - d1 * d2 * e * ((8 / 7) * np.eye(3) - d2 * (8 / 7) ** 2 * np.outer(dvec, dvec))).max() <= 1e-14


@pytest.mark.parametrize("which", [0, 1])
def test_reference_derivatives_at_large_angles(fd_case, which):
    """the same central differences, same bar, at the two poses of NC.big_angles (angles of radians; ry 1e-3 from pi / 2): the
    reference's D and DD matrices are right there before the kernel is held to them.  The guess keeps the source over the
    target: the count is at least half of `centred`'s at p* / 2"""
    src, cells, prm = fd_case
    case, p0 = NC.big_angles()[which]
    G = case["G"]
    s0 = R.sums(src, cells, prm, p0, G)
    H, g, cnt, _ = R.unpack(s0)
    assert 2 * cnt >= R.sums(src, cells, prm, 0.5 * NC.P_STAR)[27] > 300
    h = 1e-6
    g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
    for i in range(6):
        e = np.zeros(6); e[i] = h
        sp, sm = R.sums(src, cells, prm, p0 + e, G), R.sums(src, cells, prm, p0 - e, G)
        assert sp[27] == cnt and sm[27] == cnt
        g_fd[i] = (sp[28] - sm[28]) / (2 * h)
        H_fd[:, i] = (sp[21:27] - sm[21:27]) / (2 * h)
    eg, eh = np.abs(g - g_fd).max() / np.abs(g).max(), np.abs(H - H_fd).max() / np.abs(H).max()
    print("big_angles-%d: g within %.2g, H within %.2g of the largest entry" % (which, eg, eh))
    assert eg <= 1e-5 and eh <= 1e-5


def test_edge_cases_meet_their_conditions():
    """what the kernel-edge cases of tests/ndt_cases.py promise, on the reference"""
    # many_voxels (here for 4 compute units): every voxel a cell, n / 3 of them, all planar, one layer in z
    case = NC.many_voxels(4)
    cells = R.build_cells(case["tgt"], R.params(**case["prm"]))
    n = len(case["tgt"])
    assert case["n_voxels"] == 64 * 4 + 5 == len(cells["key"]) == n // 3 and (cells["count"] == 3).all() and cells["inflated"].all()
    assert cells["lat"][2][2] == 1 and R.sums(case["src"], cells, R.params(**case["prm"]))[27] >= 500
    # lane_edges: the populations, the two lines against the closed form, the tiny voxel kept
    case = NC.lane_edges()
    cells = R.build_cells(case["tgt"], R.params(**case["prm"]))
    assert sorted(cells["count"]) == sorted(case["counts"]) and cells["inflated"].sum() == 2
    t = case["tgt"][:, :3].astype(np.float64)
    for key, rows in ((case["diagonal_key"], slice(576, 586)), (case["axis_key"], slice(586, 596))):
        k = list(cells["key"]).index(key)
        want = NC.line_icov(t[rows])
        assert cells["count"][k] == 10 and cells["inflated"][k] and abs(cells["eig_ratio"][k] - 100.0) <= 1e-11
        assert np.abs(cells["icov"][k] - want).max() <= 1e-12 * np.abs(want).max()
    tiny = list(cells["count"]).index(6)
    assert 1e8 < np.abs(cells["icov"][tiny]).max() < 1e11 and not cells["inflated"][tiny]
    # borders: six pairs at squared distance 9, one per point one voxel outside; nothing from two voxels outside or from afar
    case = NC.borders()
    prm = R.params(**case["prm"])
    cells = R.build_cells(case["tgt"], prm)
    assert list(cells["lat"][2]) == [3, 2, 2] and list(cells["lat"][1]) == [0, 0, 0]
    h = R.voxel_of(case["src"][:, :3], cells["lat"])
    assert [tuple(r) for r in h[:12]] == [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (3, 1, 1), (0, 2, 0), (0, 0, 2),
                                          (-2, 0, 0), (0, -2, 0), (0, 0, -2), (4, 1, 1), (0, 3, 0), (0, 0, 3)]
    d1, d2, _ = R.constants(4.0, 0.55)
    term = -d1 * np.exp(-d2 * (8 / 7) * 9.0 / 2)
    per_point = [R.sums(case["src"][k:k + 1], cells, prm) for k in range(len(case["src"]))]
    assert [s[27] for s in per_point] == [1.0] * 6 + [0.0] * 8 and all(abs(s[28] - term) <= 1e-13 * term for s in per_point[:6])
    assert not np.array(per_point[6:]).any() and case["pairs"] == [9.0] * 6
    whole = R.sums(case["src"], cells, prm)
    assert whole[27] == 6 and abs(whole[28] - 6 * term) <= 1e-13 * whole[28]
    # sparse_native: the lattice is beyond the dense table's default, the lone point is no cell, the cells are `centred`'s
    case, base = NC.sparse_native(), NC.centred("res5")
    cells, want = R.build_cells(case["tgt"], R.params(**case["prm"])), R.build_cells(base["tgt"], R.params(**base["prm"]))
    div = cells["lat"][2]
    assert int(div[0]) * int(div[1]) * int(div[2]) > 1 << 24 and np.array_equal(cells["lat"][1], want["lat"][1])
    assert all(np.array_equal(cells[k], want[k]) for k in ("count", "mean", "icov"))
    for pose in NC.poses():
        assert np.array_equal(R.sums(case["src"], cells, R.params(**case["prm"]), pose), R.sums(base["src"], want, R.params(**base["prm"]), pose))


def test_weight_guard_case(mvr):
    """d2 > 1: w = d2 exp(-d2 q / 2) > 1 below q = 2 ln(d2) / d2, an offset of 1.65e-6 from the mean.  The library's d2 is within
    1e-13 of the reference's; d2 - 1 = 6.25e-6, so the two thresholds differ by a relative 1e-8 and no point lies between."""
    case = NC.weight_guard()
    prm = R.params(**case["prm"])
    d1, d2, _ = R.constants(prm["resolution"], prm["outlier_ratio"])
    assert d2 == 1.0000062512396983
    mine = mvr.ndt_constants(mvr.ndt_params(**case["prm"]))[1]
    assert abs(mine - d2) <= 1e-13 * d2
    cells = R.build_cells(case["tgt"], prm)
    assert len(cells["key"]) == 1 and np.abs(cells["icov"][0] - (8 / 7) / 2.5e-7 * np.array([1, 0, 0, 1, 0, 1])).max() <= 1e-6 * (8 / 7) / 2.5e-7
    thr = [np.sqrt(2 * np.log(v) / v / cells["icov"][0][0]) for v in (d2 * (1 - 1e-13), d2, d2 * (1 + 1e-13))]
    assert 1.6e-6 < thr[0] < thr[2] < 1.7e-6 and (thr[2] - thr[0]) < 1e-7 * thr[1]
    off = case["src"][:, 0].astype(np.float64) - cells["mean"][0][0]
    assert not ((off > 0.9 * thr[0]) & (off < 1.1 * thr[2])).any() and [bool(o > thr[1]) for o in off] == [bool(c) for c in NC.GUARD_COUNTS]
    for k, want in enumerate(NC.GUARD_COUNTS):
        s = R.sums(case["src"][k:k + 1], cells, prm)
        assert s[27] == want and s.any() == bool(want)


@pytest.fixture(scope="module")
def ref_runs():
    out = {}
    for case in NC.all_align_cases():
        prm = R.params(**case["prm"])
        out[case["name"]] = (case, R.align(case["src"], R.build_cells(case["tgt"], prm), prm, case["G"]))
    return out


def test_reference_reproduces_the_prototype(ref_runs):
    """what the prototype written with the issue measured on `centred`"""
    case, r5 = ref_runs["centred-res5"]
    assert (r5["stop"], r5["iterations"], r5["evaluations"]) == ("STEP", 8, 10) and abs(NC.residual(r5["X"], case) - 0.05) < 0.005
    case, r10 = ref_runs["centred-res10"]
    assert (r10["stop"], r10["iterations"], r10["evaluations"]) == ("NO_DECREASE", 5, 9) and abs(NC.residual(r10["X"], case) - 0.35) < 0.005


def test_every_line_search_decision_of_the_cases_has_a_margin(ref_runs):
    """a condition on the cases: no decision of the line search (Armijo, `better than s(0)`, `better than the remembered one`)
    is nearer to a tie than 1e-6 |s(0)| -- the GPU's sums differ from the reference's by far less, so it decides alike"""
    for name, (case, run) in ref_runs.items():
        margin = min(run["margins"], default=np.inf)          # (flat-0 and disjoint stop before any trial)
        print("%s: stop %s after %d iterations, %d evaluations; smallest margin %.3g |s(0)|; residual %.4f"
              % (name, run["stop"], run["iterations"], run["evaluations"], margin, NC.residual(run["X"], case) if case["truth"] is not None else np.nan))
        assert margin >= 1e-6, name
        for t in run["trace"]:
            assert not np.isclose(t["a"], case["prm"]["transformation_epsilon"], rtol=1e-6)       # nor the STEP stop


def trace_of(run):
    return [(t["trials"], t["reversed"], t["fallback"], t["stop"]) for t in run["trace"]]


def test_the_branch_cases_take_their_branches(ref_runs):
    """what each one-cell case is there for, on the reference; and the union of all align cases reaches every stop and both
    values of both flags (tests/test_gpu_ndt.py asserts the same of the GPU's runs)"""
    run = ref_runs["fallback"][1]
    assert (run["stop"], run["converged"], run["iterations"], run["evaluations"]) == ("ITERATIONS", True, 1, 2)
    assert trace_of(run) == [(1, True, True, "ITERATIONS")] and run["trace"][0]["a"] == NC.FALLBACK_STEP
    assert 1.1e-4 < min(run["margins"]) < 1.3e-4 and run["score"] > -R.constants(4.0, 0.55)[0] * np.exp(-R.constants(4.0, 0.55)[1] * (8 / 7) * 6.25 / 2)
    run = ref_runs["fallback-35"][1]
    assert (run["stop"], run["converged"], run["iterations"], run["evaluations"]) == ("NO_DECREASE", False, 1, 3)
    assert trace_of(run) == [(1, True, True, "NOT"), (1, True, False, "NO_DECREASE")] and np.array_equal(run["p"], [-NC.FALLBACK_STEP, 0, 0, 0, 0, 0])
    run = ref_runs["fallback-2"][1]
    assert (run["stop"], run["iterations"], run["evaluations"]) == ("STEP", 1, 3)
    assert trace_of(run) == [(2, True, False, "STEP")] and run["trace"][0]["a"] == NC.FALLBACK_STEP / 2
    run = ref_runs["flat-0"][1]
    assert (run["stop"], run["converged"], run["iterations"], run["evaluations"]) == ("FLAT", False, 0, 1)
    assert trace_of(run) == [(0, False, False, "FLAT")] and not run["p"].any() and run["count"] == 1
    run = ref_runs["flat-1"][1]
    assert (run["stop"], run["iterations"], run["evaluations"]) == ("FLAT", 1, 2) and np.array_equal(run["p"], [-1.0, 0, 0, 0, 0, 0])
    assert trace_of(run) == [(1, False, False, "NOT"), (0, False, False, "FLAT")] and run["trace"][0]["a"] == 1.0
    run, whole = ref_runs["iterations"][1], ref_runs["centred-res5"][1]
    assert (run["stop"], run["converged"], run["iterations"], run["evaluations"]) == ("ITERATIONS", True, 3, 5)
    for t, w in zip(run["trace"], whole["trace"]):
        assert all(np.array_equal(t[k], w[k]) for k in ("a", "delta_norm", "trials", "reversed", "fallback", "score", "count", "p"))
    assert [t["stop"] for t in run["trace"]] == ["NOT", "NOT", "ITERATIONS"]
    assert ref_runs["disjoint"][1]["stop"] == "NO_OVERLAP"
    assert NC.branches([(r["stop"], r["trace"]) for _, r in ref_runs.values()]) == NC.EVERY_BRANCH
    # ... and without the new cases it does not: they are what reaches ITERATIONS, FLAT and the fallback
    old = [(r["stop"], r["trace"]) for n, (_, r) in ref_runs.items() if n in [c["name"] for c in NC.align_cases()]]
    assert NC.branches(old) == ({"STEP", "NO_DECREASE"}, {False, True}, {False})


def test_far_follows_centred_and_guess_ends_where_centred_ends(ref_runs):
    for which in ("res5", "res10"):
        c, f, g = ref_runs["centred-" + which][1], ref_runs["far-" + which][1], ref_runs["guess-" + which][1]
        assert (f["stop"], f["iterations"], f["evaluations"]) == (c["stop"], c["iterations"], c["evaluations"])
        assert [(t["trials"], t["reversed"], t["fallback"]) for t in f["trace"]] == [(t["trials"], t["reversed"], t["fallback"]) for t in c["trace"]]
        Xf = NC.far_to_centred(f["X"])
        assert np.abs(Xf[:3, :3] - c["X"][:3, :3]).max() <= 1e-5 and np.abs(Xf[:3, 3] - c["X"][:3, 3]).max() <= 1e-4
        # the guess run takes other steps and stops elsewhere in the flat bottom of the score: it ends where `centred` ends in
        # the sense of the residual against the known motion, not at the parity bars
        case = ref_runs["centred-" + which][0]
        print("%s: guess ends %.3g (rotation), %.3g (translation) from centred; residuals %.4f and %.4f"
              % (which, np.abs(g["X"][:3, :3] - c["X"][:3, :3]).max(), np.abs(g["X"][:3, 3] - c["X"][:3, 3]).max(),
                 NC.residual(g["X"], case), NC.residual(c["X"], case)))
        assert NC.residual(g["X"], case) <= 2 * NC.residual(c["X"], case)


def test_direction_of_rule_n7(mvr):
    rng = np.random.default_rng(5)
    for trial in range(20):
        A = rng.standard_normal((6, 6))
        H = -(A @ A.T) if trial % 2 else A + A.T             # negative definite, or indefinite
        if trial == 7:
            H[:, 5] = H[5, :] = 0.0                           # rank 5: the null direction is dropped
        s = np.zeros(29)
        s[:21], s[21:27] = H[R.TRIU], rng.standard_normal(6)
        want = R.direction(s)
        got, rc = mvr.ndt_direction(s)
        assert rc == 0 and np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
        if trial == 7:
            assert got[5] == 0.0
    s = np.zeros(29)
    assert mvr.ndt_direction(s)[1] == mvr.E_SINGULAR and R.direction(s) is not None and not R.direction(s).any()
    s[3] = np.nan
    assert mvr.ndt_direction(s)[1] == mvr.E_SINGULAR and R.direction(s) is None
    # ... with a gradient too: a NaN or an infinity anywhere in H or g, and delta is not a number (the Jacobi sweeps end at once
    # on a NaN off the diagonal; the diagonal alone used to answer)
    for slot in (3, 9, 0, 20, 21, 26):
        for bad in (np.nan, -np.inf):
            s = pack(-np.eye(6), np.arange(1.0, 7.0), 5.0, 1.0)
            s[slot] = bad
            got, rc = mvr.ndt_direction(s)
            with np.errstate(invalid="ignore"):
                assert rc == mvr.E_SINGULAR and np.isnan(got).all() and R.direction(s) is None, (slot, bad)


def test_argument_errors_of_rule_n11_without_a_device(mvr):
    """mvr_ndt_constants runs exactly the checks the three entry points run before any GPU work; they refuse a NULL context"""
    L = mvr._lib
    d = (C.c_double * 3)()
    ok = mvr.ndt_params(resolution=5.0)
    assert L.mvr_ndt_constants(C.byref(ok), None, d) == mvr.OK
    assert L.mvr_ndt_constants(None, None, d) == mvr.E_ARG and L.mvr_ndt_constants(C.byref(ok), None, None) == mvr.E_ARG
    bad = []
    for field in ("resolution", "step_size", "transformation_epsilon", "min_covar_eigvalue_mult"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            bad.append({field: v})
    bad += [dict(outlier_ratio=v) for v in (0.0, 1.0, -0.1, 1.5, float("nan"))]
    bad += [dict(max_iterations=0), dict(max_line_evals=0), dict(max_iterations=-3)]
    bad += [dict(origin=(0.0, float("nan"), 0.0)), dict(origin=(float("inf"), 0.0, 0.0))]
    bad += [dict(resolution=1e-120), dict(resolution=1e120)]              # d1, d2 not finite / not of their sign
    for kw in bad:
        p = mvr.ndt_params(**dict(dict(resolution=5.0), **kw))
        assert L.mvr_ndt_constants(C.byref(p), None, d) == mvr.E_ARG, kw
    G = np.eye(4)
    G[1, 3] = np.nan
    Gc = mvr.to_cm(G, np.float64)
    assert L.mvr_ndt_constants(C.byref(ok), Gc.ctypes.data_as(C.POINTER(C.c_double)), d) == mvr.E_ARG
    T, X, st = (C.c_float * 16)(), (C.c_double * 16)(), mvr.NdtStats()
    n, x, out = C.c_size_t(), (C.c_double * 6)(), (C.c_double * 29)()
    assert L.mvr_ndt_align(None, 0, 1, -1, C.byref(ok), None, T, X, C.byref(st), None, 0) == mvr.E_ARG
    assert L.mvr_ndt_sums(None, 0, 1, C.byref(ok), None, x, out) == mvr.E_ARG
    assert L.mvr_ndt_cells(None, 0, C.byref(ok), 0, None, None, None, None, C.byref(n)) == mvr.E_ARG


# ---- the loop of N7-N9 on scripted sums: mvr.ndt_newton against R.align, both driven by the same Python evaluation
def pack(H, g, count, score):
    s = np.zeros(29)
    s[:21], s[21:27], s[27], s[28] = np.asarray(H, np.float64)[R.TRIU], g, count, score
    return s


def same(a, b, exact):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if exact:
        return np.array_equal(a.view(np.uint64), b.view(np.uint64)) or np.array_equal(a, b)       # (-0.0 == 0.0 is fine)
    both_nan = np.isnan(a) & np.isnan(b)
    scale = max(1.0, float(np.abs(b[np.isfinite(b)]).max())) if np.isfinite(b).any() else 1.0
    return bool(np.all(both_nan | (a == b) | (np.abs(a - b) <= 1e-12 * scale)))


def both(mvr, make, exact, trace_cap=None, **kw):
    """the product and the reference on two fresh copies of one evaluation; everything the issue lists is equal.  exact: the
    direction is an axis and every length a halving or a sum of halvings, so a, p, p_out and sums_out are the same bits;
    else 1e-12 of the largest entry (the two eigen-solvers differ in the last bits of delta)"""
    f, fr = make(), make()
    got = mvr.ndt_newton(mvr.ndt_params(**kw), f, trace_cap=trace_cap)
    ref = R.align(None, None, R.params(**kw), evaluate=fr)
    assert got["rc"] == (mvr.E_NOCORR if ref["stop"] == "NO_OVERLAP" else mvr.OK)
    for k in ("stop", "converged", "iterations", "evaluations"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert len(f.seen) == len(fr.seen) == ref["evaluations"] and all(same(a, b, exact) for a, b in zip(f.seen, fr.seen))
    n = len(ref["trace"]) if trace_cap is None else min(trace_cap, len(ref["trace"]))
    assert len(got["trace"]) == n
    for k, (g, r) in enumerate(zip(got["trace"], ref["trace"])):
        assert (g["trials"], g["reversed"], g["fallback"], g["stop"]) == (r["trials"], r["reversed"], r["fallback"], r["stop"]), (k, g, r)
        for key in ("a", "p", "delta_norm", "score", "count"):
            assert same(g[key], r[key], exact and key in ("a", "p", "score", "count")), (k, key, g[key], r[key])
    assert same(got["p"], ref["p"], exact) and same(got["sums"], ref["sums"], exact)
    assert same(got["score"], ref["score"], exact) and got["count"] == ref["count"]
    return got, ref


class Bowl:
    """s(p) = c - (p - p0)^T A (p - p0) / 2: g = -A (p - p0), H = -A (flip: the Hessian reported with the wrong sign)"""
    def __init__(self, A, p0, flip=False):
        self.A, self.p0, self.flip, self.seen = A, p0, flip, []

    def __call__(self, p):
        self.seen.append(p.copy())
        d = p - self.p0
        return pack(self.A if self.flip else -self.A, -self.A @ d, 50.0, 100.0 - 0.5 * d @ self.A @ d)


def bowl_matrix():
    rng = np.random.default_rng(11)
    B = rng.standard_normal((6, 6))
    return B @ B.T + 6.0 * np.eye(6)


def test_newton_on_a_quadratic_bowl(mvr):
    A = bowl_matrix()
    p0 = np.array([0.3, -0.2, 0.25, 0.1, -0.15, 0.2])                # |p0| = 0.515
    # one step: |delta| <= step_size, and the step is Newton's whole one; max_iterations 1 keeps the loop off the rounding
    # noise a second direction at p0 would be made of
    got, ref = both(mvr, lambda: Bowl(A, p0), False, step_size=1.0, transformation_epsilon=0.01, max_iterations=1)
    assert (got["stop"], got["iterations"], got["evaluations"]) == ("ITERATIONS", 1, 2)
    assert np.abs(got["p"] - p0).max() <= 1e-14 and abs(got["trace"][0]["a"] - np.linalg.norm(p0)) <= 1e-14
    # capped: steps of exactly step_size along the line to p0, then the rest of it, shorter than epsilon: STEP
    step = 0.2
    got, ref = both(mvr, lambda: Bowl(A, p0), False, step_size=step, transformation_epsilon=0.15)
    n = int(np.ceil(np.linalg.norm(p0) / step))
    assert n == 3 and (got["stop"], got["iterations"], got["evaluations"]) == ("STEP", n, n + 1)
    assert [t["a"] for t in got["trace"][:-1]] == [step] * (n - 1) and abs(got["trace"][-1]["a"] - (np.linalg.norm(p0) - (n - 1) * step)) <= 1e-14
    assert np.abs(got["p"] - p0).max() <= 1e-14 and all(t["trials"] == 1 and not t["reversed"] and not t["fallback"] for t in got["trace"])
    scores = [100.0 - 0.5 * p0 @ A @ p0] + [t["score"] for t in got["trace"]]
    assert all(b > a for a, b in zip(scores, scores[1:])) and abs(scores[-1] - 100.0) <= 1e-12


def test_newton_reverses_a_direction_that_descends(mvr):
    A = bowl_matrix()
    p0 = np.array([0.3, -0.2, 0.25, 0.1, -0.15, 0.2])
    got, ref = both(mvr, lambda: Bowl(A, p0, flip=True), False, step_size=1.0, transformation_epsilon=0.01, max_iterations=1)
    t = got["trace"][0]
    assert t["reversed"] and not t["fallback"] and t["trials"] == 1 and t["score"] > 100.0 - 0.5 * p0 @ A @ p0
    assert np.abs(got["p"] - p0).max() <= 1e-14                      # -H^+ g pointed away; reversed, it is Newton's step


class Script:
    """call k (from 0) returns entry k: (score, g0) or (score, g0, H).  H = -I unless given and g = (g0, 0, ...): delta is
    (g0, 0, ...) exactly, u the x axis, phi'0 = -|g0|.  The count is 100 + k, so every returned row is told from the others."""
    def __init__(self, entries):
        self.entries, self.seen = entries, []

    def __call__(self, p):
        k = len(self.seen)
        self.seen.append(p.copy())
        assert k < len(self.entries), "the script is over: call %d at %r" % (k, p)
        e = self.entries[k]
        if isinstance(e, (int, np.integer)):
            return int(e)
        g = np.zeros(6) if np.ndim(e[1]) == 0 else np.asarray(e[1], np.float64)
        if np.ndim(e[1]) == 0:
            g[0] = e[1]
        return pack(-np.eye(6) if len(e) < 3 else e[2], g, 100.0 + k, e[0])


def test_newton_flat_stops(mvr):
    # g = 0: FLAT on |delta| before any trial
    got, ref = both(mvr, lambda: Script([(10.0, 0.0)]), True)
    assert (got["stop"], got["converged"], got["iterations"], got["evaluations"]) == ("FLAT", False, 0, 1)
    assert len(got["trace"]) == 1 and (got["trace"][0]["a"], got["trace"][0]["trials"], got["trace"][0]["delta_norm"]) == (0.0, 0, 0.0)
    assert not got["p"].any() and got["sums"][27] == 100.0
    # a NaN in H (and, apart, in g): |delta| is not a number
    H = -np.eye(6)
    H[2, 4] = H[4, 2] = np.nan
    for entry in ((10.0, 8.0, H), (10.0, [8.0, np.nan, 0, 0, 0, 0]), (10.0, 8.0, np.full((6, 6), np.inf))):
        got, ref = both(mvr, lambda: Script([entry]), True)
        assert (got["stop"], got["iterations"], got["evaluations"]) == ("FLAT", 0, 1) and np.isnan(got["trace"][0]["delta_norm"])
        assert got["trace"][0]["a"] == 0.0 and not got["p"].any()
    # phi'0 = 0 with delta != 0: H = diag(1, -1, ...) is indefinite, g = (1, 1, 0, ...) has g.H^+ g = 1 - 1 = 0
    H, g = np.diag([1.0, -1.0, 1.0, -1.0, 1.0, -1.0]), np.array([1.0, 1.0, 0, 0, 0, 0])
    delta = R.direction(pack(H, g, 1.0, 0.0))
    assert np.array_equal(delta, [-1.0, 1.0, 0, 0, 0, 0]) and g @ (delta / np.sqrt(delta @ delta)) == 0.0        # exactly, in f64
    got, ref = both(mvr, lambda: Script([(10.0, g, H)]), True)
    assert (got["stop"], got["iterations"], got["evaluations"]) == ("FLAT", 0, 1)
    assert got["trace"][0]["delta_norm"] == np.sqrt(2.0) and got["trace"][0]["trials"] == 0 and not got["trace"][0]["reversed"]
    # after a step: the sums of the taken trial are the current ones, and they are flat
    got, ref = both(mvr, lambda: Script([(10.0, 8.0), (11.0, 0.0)]), True, step_size=1.0, transformation_epsilon=0.01)
    assert (got["stop"], got["iterations"], got["evaluations"]) == ("FLAT", 1, 2) and got["p"][0] == 1.0 and len(got["trace"]) == 2


# s(0) = 10, |delta| = 8, step_size 1, phi'0 = -8: a trial at length a is accepted from 10 + 8e-4 a on
LOW = 10.0001          # above s(0), below the Armijo line at a = 1 (10.0008), 1 / 2 (10.0004) and 1 / 4 (10.0002)
LINE = dict(step_size=1.0, transformation_epsilon=1e-3, max_iterations=1)


def test_newton_scripted_line_searches(mvr):
    def run(scores, **kw):
        return both(mvr, lambda: Script([(10.0, 8.0)] + [(s, 8.0) for s in scores]), True, **dict(LINE, **kw))[0]
    # (a) accepted at trial 3
    got = run([9.0, 9.5, 11.0])
    t = got["trace"][0]
    assert (t["trials"], t["fallback"], t["reversed"], t["a"], got["p"][0], got["sums"][27]) == (3, False, False, 0.25, 0.25, 103.0)
    assert (got["stop"], got["evaluations"]) == ("ITERATIONS", 4)
    # (b) none accepted, none above s(0)
    got = run([9.0, 9.5, 9.9, 10.0], max_line_evals=4)          # (the last: equal to s(0) is not above it)
    t = got["trace"][0]
    assert (got["stop"], got["converged"], got["iterations"], got["evaluations"]) == ("NO_DECREASE", False, 0, 5)
    assert (t["trials"], t["a"], t["fallback"]) == (4, 0.0, False) and not got["p"].any() and (got["sums"][27], got["score"]) == (100.0, 10.0)
    # (c) trial 1 remembered, trial 3 better: the fallback takes trial 3 with trial 3's a and trial 3's sums
    got = run([LOW, 9.0, 10.00015], max_line_evals=3)
    t = got["trace"][0]
    assert (t["trials"], t["fallback"], t["a"], got["p"][0], got["sums"][27], got["score"]) == (3, True, 0.25, 0.25, 103.0, 10.00015)
    assert (got["stop"], got["iterations"], got["evaluations"]) == ("ITERATIONS", 1, 4)
    # (d) trial 1 remembered, the later ones above s(0) but worse: trial 1's a and sums
    got = run([LOW, 10.00005, 10.00002], max_line_evals=3)
    t = got["trace"][0]
    assert (t["trials"], t["fallback"], t["a"], got["p"][0], got["sums"][27], got["score"]) == (3, True, 1.0, 1.0, 101.0, LOW)
    # (e) NaN and -inf are neither accepted nor remembered, and the search goes on
    got = run([np.nan, -np.inf, 11.0])
    assert (got["trace"][0]["trials"], got["trace"][0]["fallback"], got["trace"][0]["a"], got["sums"][27]) == (3, False, 0.25, 103.0)
    got = run([np.nan, -np.inf, LOW], max_line_evals=3)
    assert (got["trace"][0]["trials"], got["trace"][0]["fallback"], got["trace"][0]["a"], got["sums"][27]) == (3, True, 0.25, 103.0)
    got = run([np.nan, -np.inf], max_line_evals=2)
    assert got["stop"] == "NO_DECREASE" and got["trace"][0]["trials"] == 2 and got["score"] == 10.0
    # (f) ten failing trials, the halving far from epsilon: the search ends on max_line_evals
    got = run([9.0] * 10, transformation_epsilon=1e-9)
    assert (got["stop"], got["trace"][0]["trials"], got["evaluations"]) == ("NO_DECREASE", 10, 11)
    assert [p[0] for p in got_seen(mvr, [9.0] * 10, transformation_epsilon=1e-9)[1:]] == [2.0 ** -k for k in range(10)]
    # (g) a large epsilon: the search ends when a < epsilon / 2, after the trials the halving predicts
    for eps in (0.3, 0.25, 0.2500001, 1.0, 2.0, 2.0000001, 3.0):
        want, a = 0, 1.0
        while True:
            want += 1
            a *= 0.5
            if a < eps / 2.0:
                break
        got = run([9.0] * want, transformation_epsilon=eps)
        assert want == {0.3: 3, 0.25: 4, 0.2500001: 3, 1.0: 2, 2.0: 1, 2.0000001: 1, 3.0: 1}[eps]
        assert (got["stop"], got["trace"][0]["trials"], got["evaluations"]) == ("NO_DECREASE", want, want + 1)
    # (h) a taken a = 1 against an epsilon one ulp above, equal, one ulp below: STEP, and twice no stop
    for eps, stop in ((np.nextafter(1.0, 2.0), "STEP"), (1.0, "FLAT"), (np.nextafter(1.0, 0.0), "FLAT")):
        got = both(mvr, lambda: Script([(10.0, 8.0), (11.0, 0.0)]), True, step_size=1.0, transformation_epsilon=eps, max_iterations=5)[0]
        assert (got["stop"], got["iterations"], got["trace"][0]["a"], got["trace"][0]["stop"]) == (stop, 1, 1.0, "STEP" if stop == "STEP" else "NOT")


def got_seen(mvr, scores, **kw):
    f = Script([(10.0, 8.0)] + [(s, 8.0) for s in scores])
    mvr.ndt_newton(mvr.ndt_params(**dict(LINE, **kw)), f)
    return f.seen


def test_newton_iteration_cap_and_the_order_of_the_stops(mvr):
    climb = [(10.0 + k, 8.0) for k in range(6)]
    for cap in (1, 3):
        got = both(mvr, lambda: Script(climb), True, step_size=1.0, transformation_epsilon=0.01, max_iterations=cap)[0]
        assert (got["stop"], got["converged"], got["iterations"], got["evaluations"], got["p"][0]) == ("ITERATIONS", True, cap, cap + 1, float(cap))
        assert [t["stop"] for t in got["trace"]] == ["NOT"] * (cap - 1) + ["ITERATIONS"]
    # N9 asks STEP first: a last allowed step shorter than epsilon says STEP
    got = both(mvr, lambda: Script([(10.0, 2.0 ** -10), (11.0, 8.0)]), True, step_size=1.0, transformation_epsilon=0.01, max_iterations=1)[0]
    assert (got["stop"], got["converged"], got["iterations"], got["trace"][0]["a"]) == ("STEP", True, 1, 2.0 ** -10)
    # no overlap: a count of 0 at the start
    got = both(mvr, NoPairs, True)[0]
    assert (got["rc"], got["stop"], got["iterations"], got["evaluations"], got["trace"]) == (mvr.E_NOCORR, "NO_OVERLAP", 0, 1, [])


class NoPairs:
    def __init__(self):
        self.seen = []

    def __call__(self, p):
        self.seen.append(p.copy())
        return pack(-np.eye(6), np.ones(6), 0.0, 0.0)


def raw_newton(mvr, prm, fn, cap, records, with_trace=True):
    """mvr_ndt_newton on a trace array of `records` records filled with the byte 0xA5 -> (rc, stats, p, sums, the array's bytes)"""
    tr = (mvr.NdtIterTrace * records)()
    C.memset(tr, 0xA5, C.sizeof(tr))

    def call(user, p, out):
        r = fn(np.array(p[:6]))
        if isinstance(r, int):
            return r
        for k in range(29):
            out[k] = r[k]
        return 0
    cb = mvr.NDT_EVAL_FN(call)
    x, s, st = (C.c_double * 6)(), (C.c_double * 29)(), mvr.NdtStats()
    rc = mvr._lib.mvr_ndt_newton(C.byref(prm), cb, None, x, s, C.byref(st), tr if with_trace else None, cap)
    size = C.sizeof(mvr.NdtIterTrace)
    return rc, (st.iterations, st.stop, st.converged, st.evaluations, st.n_pairs, st.score), list(x), list(s), \
        np.frombuffer(bytes(tr), np.uint8).reshape(records, size)


def test_newton_trace_cap_shorter_than_the_run(mvr):
    """4 records: three steps, then NO_DECREASE.  With a cap of 0, 1, 2 (= iterations - 1) and 3 the records below the cap are
    the uncapped run's, those from the cap on keep the bytes they had, and the stats, pose and sums do not change"""
    script = [(10.0, 8.0), (11.0, 8.0), (12.0, 8.0), (13.0, 8.0), (9.0, 8.0)]
    prm = mvr.ndt_params(step_size=1.0, transformation_epsilon=0.01, max_line_evals=1)
    full = raw_newton(mvr, prm, Script(script), 6, 6)
    assert full[0] == 0 and full[1][:4] == (3, mvr.NDT_STOPS.index("NO_DECREASE"), 0, 5)
    assert (full[4][4:] == 0xA5).all() and not (full[4][:4] == 0xA5).all(1).any()
    for cap in (0, 1, 2, 3):
        got = raw_newton(mvr, prm, Script(script), cap, 6)
        assert got[:4] == full[:4], cap
        assert np.array_equal(got[4][:cap], full[4][:cap]) and (got[4][cap:] == 0xA5).all(), cap
        cut = mvr.ndt_newton(prm, Script(script), trace_cap=cap)
        assert len(cut["trace"]) == cap and (cut["iterations"], cut["evaluations"]) == (3, 5)
    none = raw_newton(mvr, prm, Script(script), 6, 6, with_trace=False)
    assert none[:4] == full[:4] and (none[4] == 0xA5).all()
    assert mvr._lib.mvr_ndt_newton(C.byref(prm), mvr.NDT_EVAL_FN(lambda u, p, o: 0), None, (C.c_double * 6)(), None, None,
                                   (mvr.NdtIterTrace * 1)(), -1) == mvr.E_ARG
    assert mvr._lib.mvr_ndt_newton(None, mvr.NDT_EVAL_FN(lambda u, p, o: 0), None, (C.c_double * 6)(), None, None, None, 0) == mvr.E_ARG
    bad = mvr.ndt_params(max_line_evals=0)
    assert mvr._lib.mvr_ndt_newton(C.byref(bad), mvr.NDT_EVAL_FN(lambda u, p, o: 0), None, (C.c_double * 6)(), None, None, None, 0) == mvr.E_ARG


def test_newton_returns_the_callbacks_status_at_once(mvr):
    prm = mvr.ndt_params(step_size=1.0, transformation_epsilon=0.01, max_line_evals=3)
    for k in (1, 4):          # the first call; the fourth: the second trial of the second iteration
        f = Script([(10.0, 8.0), (11.0, 8.0), (9.0, 8.0), (12.0, 8.0)][:k - 1] + [mvr.E_HIP])
        got = mvr.ndt_newton(prm, f)
        assert got == dict(rc=mvr.E_HIP) and len(f.seen) == k
        f = Script([(10.0, 8.0), (11.0, 8.0), (9.0, 8.0), (12.0, 8.0)][:k - 1] + [mvr.E_HIP])
        rc, st, x, s, tr = raw_newton(mvr, prm, f, 6, 6)
        assert rc == mvr.E_HIP and len(f.seen) == k and st[:4] == (0, 0, 0, 0) and not any(x) and not any(s)
