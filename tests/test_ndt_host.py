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


@pytest.fixture(scope="module")
def ref_runs():
    out = {}
    for case in NC.align_cases():
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
        print("%s: stop %s after %d iterations, %d evaluations; smallest margin %.3g |s(0)|; residual %.4f"
              % (name, run["stop"], run["iterations"], run["evaluations"], min(run["margins"]), NC.residual(run["X"], case)))
        assert min(run["margins"]) >= 1e-6, name
        for t in run["trace"]:
            assert not np.isclose(t["a"], case["prm"]["transformation_epsilon"], rtol=1e-6)       # nor the STEP stop


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
