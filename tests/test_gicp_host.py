"""CPU tests of Generalized ICP: the numpy reference (tests/gicp_ref.py) against plain loops and against scipy's BFGS on an
independently written objective, the conditions the align cases of tests/gicp_cases.py promise, the arguments that are refused
before any device is touched, and the layout of the structs against the Python bindings.  No GPU compute here."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import gicp_cases as GC
import gicp_ref as G
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


scipy_minimum = G.scipy_minimum


def test_reference_against_plain_loops():
    for name in ("rand_3", "rand_64", "rand_65", "palette", "half"):
        p, s, q, n = G_in = GC.gathered(GC.list_case(name))
        for X in (np.eye(4), GC.sums_pose()):
            for eps in (1e-3, 1.0):
                got, tot = G.sums(*G_in, X, eps, with_abs=True)
                exp = G.naive_sums(p, s, q, n, X, eps)
                assert got[27] == len(p) == exp[27]
                assert (np.abs(got - exp) <= 1e-12 * tot).all(), (name, eps, np.abs(got - exp) / tot)
                assert abs(G.objective(*G_in, X, eps) - G.naive_F(p, s, q, n, X, eps)) <= 1e-12 * tot[28] / len(p)
    # G3: a side whose normal is NaN, zero or not of unit length
    A = G.side(np.array([[np.nan, 0, 1], [0, 0, 0], [0, 0, 0.5], [0, 3, 0], [np.inf, 0, 0]]), 0.25)
    assert np.array_equal(A[0], np.eye(3)) and np.array_equal(A[1], np.eye(3)) and np.array_equal(A[4], np.eye(3))
    assert np.allclose(A[2], np.diag([1, 1, 0.25]), atol=1e-15) and np.allclose(A[3], np.diag([1, 0.25, 1]), atol=1e-15)
    # G6: the step solves the damped system; a zero pivot is refused; the small-angle branch joins the other
    rng = np.random.default_rng(0)
    M = rng.standard_normal((6, 9))
    H, g = M @ M.T, rng.standard_normal(6)
    d = G.cholesky_solve(H, g, 1e-3)
    assert np.allclose((H + 1e-3 * np.diag(np.diag(H))) @ d, -g, rtol=0, atol=1e-10)
    H0 = H.copy()
    H0[0, :] = H0[:, 0] = 0.0
    assert G.cholesky_solve(H0, g, 1e-3) is None and G.cholesky_solve(H * np.nan, g, 1e-3) is None
    w = np.array([3e-9, -4e-9, 1e-9])
    assert np.allclose(G.rodrigues(w), G.rodrigues(w * 10) - 9 * np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]), atol=1e-15)
    E = G.rodrigues(np.array([0.3, -0.2, 0.5]))
    assert np.allclose(E @ E.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(E) - 1) < 1e-15
    # G8: the outer delta
    a, b = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    b[0, 1], b[2, 3] = 1e-3, 1e-3
    assert G.outer_delta(b, a, G.params()) == max(float(np.float32(1e-3)) / 2e-3, float(np.float32(1e-3)) / 5e-4)


def test_palette_holds_every_kind_of_normal():
    c = GC.list_case("palette")
    ks, kt, par = c["kinds"]
    assert all((k == v).sum() >= 10 for k in (ks, kt) for v in range(6)) and len(par) >= 30
    p, s, q, n = GC.gathered(c)
    M = G.side(s, 1e-3) + G.side(n, 1e-3)
    ev = np.linalg.eigvalsh(M)
    assert ev.min() >= 2e-3 * (1 - 1e-9) and ev.max() <= 2.0 * (1 + 1e-12)
    assert (ev[:, 0] < 2.1e-3).sum() >= 5                                  # parallel unit normals: the smallest eigenvalue is 2 eps
    assert len(GC.list_case("half")["query"]) * 2 == len(GC.list_case("half")["src"])


@pytest.mark.parametrize("name", ["rand_3", "rand_64", "rand_257", "palette", "half", "rand_6001"])
def test_reference_solve_reaches_scipys_minimum(name):
    p, s, q, n = GC.gathered(GC.list_case(name))
    for eps in (1e-3, 1.0):
        X, info, status = G.solve(p, s, q, n, G.params(gicp_epsilon=eps))
        assert status == G.OK and 2 <= info["evaluations"] <= 20 and info["accepted"] >= 1, info
        F_ref, F_sp = G.objective(p, s, q, n, X, eps), scipy_minimum(p, s, q, n, eps)
        print("%s eps %g: F %.12g, scipy %.12g, relative %.2g, %d evaluations" % (name, eps, F_ref, F_sp, (F_ref - F_sp) / F_sp, info["evaluations"]))
        assert info["f1"] == F_ref <= info["f0"]
        assert F_ref <= F_sp * (1 + 1e-9)
        assert np.allclose(X[:3, :3] @ X[:3, :3].T, np.eye(3), atol=1e-14) and np.array_equal(X[3], [0, 0, 0, 1])
    # eps = 1: W = I / 2 and the minimum is the SVD estimator's
    Xk = G.kabsch(p, q)
    assert np.abs(X[:3, :3] - Xk[:3, :3]).max() <= 1e-5 and np.abs(X[:3, 3] - Xk[:3, 3]).max() <= 1e-4


def test_reference_refusals():
    p, s, q, n = GC.gathered(GC.list_case("rand_64"))
    assert G.solve(p[:2], s[:2], q[:2], n[:2], G.params())[2] == G.E_NOCORR
    z = np.zeros((5, 3))
    X, info, status = G.solve(z, s[:5], z, n[:5], G.params())             # every point at the origin: the rotation rows of H are 0
    assert status == G.E_SINGULAR and info["evaluations"] == 1 and np.array_equal(X, np.eye(4))
    X, info, status = G.solve(p, s, q, n, G.params(max_inner_iterations=1))
    assert status == G.OK and info["evaluations"] == 1 and np.array_equal(X, np.eye(4))


def how_it_ended(info, status, log, prm):
    if status == G.E_SINGULAR:
        return "singular"
    last = log[-1]
    if last["decision"] == "R" and last["lam_after"] > 1e9:
        return "lambda"
    if last["decision"] == "A" and last["w"] < prm["inner_rot_tol"] and last["v"] < prm["inner_trans_tol"]:
        return "tol"
    assert info["evaluations"] == prm["max_inner_iterations"]
    return "cap"


def allowed_undecided(spec, evaluations):
    return {evaluations if k == "last" else k for k in spec}


@pytest.mark.parametrize("name", GC.BRANCH_NAMES)
def test_branch_cases_reach_their_branches(name):
    """what tests/gicp_cases.py says each branch case is for, on the reference alone"""
    want, c = GC.BRANCH[name], GC.branch_case(name)
    assert c["tgt"].dtype == np.float32 and c["src"].dtype == np.float32
    X, info, status, log = GC.reference_run(name)
    prm = G.params(**GC.branch_params(name))
    pat, und = G.pattern(log), G.undecided(log)
    margins = [abs(e["fc"] - e["f"]) / (e["tot"] + e["totc"]) for e in log if e["decided"] and e["tot"] + e["totc"] > 0]
    print("%s: %s, %d evaluations, lambda %g, %s, undecided %s, smallest decided margin %.3g, f %.6g -> %.6g"
          % (name, pat or "-", info["evaluations"], info["lambda"], how_it_ended(info, status, log, prm), und, min(margins) if margins else 0.0,
             info["f0"], info["f1"]))
    assert re.fullmatch(want["pattern"], pat), pat
    assert how_it_ended(info, status, log, prm) == want["end"]
    assert pat.count("R") == want["rejects"] and info["accepted"] == pat.count("A") and info["evaluations"] == len(log) + 1
    assert info["evaluations"] == want.get("evals", info["evaluations"]) <= 34
    # the cap on what may be undecided, and never the first decision
    assert set(und) <= allowed_undecided(want["undecided"], info["evaluations"]) and 2 not in und, und
    assert info["lambda"] == G.lambda_of(pat)
    if want.get("small_arm"):
        last = [e for e in log if e["decision"] == "A"][-1]
        assert last is log[-1] and 0.0 < last["w"] < 1e-8
    if name == "exact_fit":
        assert all(e["tot"] == 0.0 and e["totc"] == 0.0 and e["decided"] for e in log)
        assert info["lambda"] == 1e10 and info["f0"] == info["f1"] == 0.0 and np.array_equal(X, np.eye(4))
    if want["end"] == "singular":
        assert np.array_equal(X, np.eye(4)) and info["accepted"] == 0
    if name == "collinear_origin":
        p = GC.gathered(c)[0]
        assert G.sums(*GC.gathered(c), np.eye(4), 1e-3)[0] == 0.0 and np.abs(p).max() > 10.0      # H[0][0] = 0 though the cloud does not sit at the origin
        assert np.isfinite(info["f0"])
    if name in ("nan_point", "inf_target"):
        assert not np.isfinite(info["f0"])
    if name == "turn_0.3_long":
        d = GC.gathered(c)[0] @ (X - c["T"])[:3, :3].T + (X - c["T"])[:3, 3]
        assert np.abs(X - c["T"]).max() < 3e-4 and np.abs(d).max() < 1e-3


def test_the_old_list_cases_take_one_path():
    """every list case, at both values of eps: accepts only, ended by the tolerance, and only the last decisions are undecided --
    which is why tests/test_gpu_gicp.py holds their counters to the reference over the decided prefix only"""
    for name in GC.LIST_NAMES + ("big",):                 # big: the list of the GPU test at the 256 compute units of an MI355X
        for eps in (1e-3, 1.0):
            if name == "big":
                log = []
                X, info, status = G.solve(*GC.gathered(GC.big_list(256)), G.params(gicp_epsilon=eps), log=log)
            else:
                X, info, status, log = GC.reference_run(name, eps)
            pat, und = G.pattern(log), G.undecided(log)
            print("%s eps %g: %s, undecided %s" % (name, eps, pat, und))
            assert status == G.OK and re.fullmatch("A+", pat) and how_it_ended(info, status, log, G.params()) == "tol"
            assert 1 <= len(und) <= GC.LIST_UNDECIDED_TAIL and min(und) > info["evaluations"] - GC.LIST_UNDECIDED_TAIL
            assert GC.decided_prefix(log) >= 6


def test_the_non_finite_rule_of_the_reference():
    for name in ("nan_point", "inf_target"):
        X, info, status, log = GC.reference_run(name)
        assert status == G.E_SINGULAR and info["evaluations"] == 1 and info["accepted"] == 0 and log == [] and np.array_equal(X, np.eye(4))
    c = GC.branch_case("inf_target")
    sm = G.sums(*GC.gathered(c), np.eye(4), 1e-3)
    assert sm[27] == len(c["query"]) and not np.isfinite(sm[28])
    # a NaN in a source point the list does not name is not seen
    a, b = GC.unlisted_nan()
    assert not np.isfinite(b["src"][:, :3]).all() and all(np.array_equal(x, y) for x, y in zip(GC.gathered(a), GC.gathered(b)))


@pytest.mark.parametrize("name", GC.UNIT_CASES)
def test_the_reference_is_homogeneous_in_the_unit_of_length(name):
    c = GC.any_case(name)
    X0, i0, st0 = G.solve(*GC.gathered(c), G.params())
    assert st0 == G.OK
    for s in GC.UNIT_SCALES:
        X, info, st = G.solve(*GC.gathered(GC.in_unit(c, s)), G.params(inner_trans_tol=1e-5 * s))
        assert st == G.OK and np.array_equal(X[:3, :3], X0[:3, :3]) and np.array_equal(X[:3, 3] / s, X0[:3, 3])
        assert (info["evaluations"], info["accepted"], info["lambda"]) == (i0["evaluations"], i0["accepted"], i0["lambda"])
        assert info["f1"] / s ** 2 == i0["f1"] and info["f0"] / s ** 2 == i0["f0"]


def test_long_double_terms_against_the_f64_terms():
    """G.terms_ld is the reference of the sums over the range of gicp_epsilon; at 1e-3 and 1 it must agree with G.terms, whose
    inverse is LAPACK's, within that one's error"""
    for name in ("palette", "rand_65"):
        g = GC.gathered(GC.list_case(name))
        for X in (np.eye(4), GC.sums_pose()):
            for eps in (1.0, 1e-3):
                a, tot = G.sums(*g, X, eps, with_abs=True)
                b, tot_ld = G.sums_ld(*g, X, eps)
                assert a[27] == b[27] == len(g[0])
                assert (np.abs(a - b) <= 1e-12 * tot).all() and (np.abs(tot - tot_ld) <= 1e-12 * tot).all()
    # palette's parallel pairs: A + B has the eigenvalue 2 eps, so W has 1 / (2 eps) along the common normal
    c = GC.list_case("palette")
    p, s, q, n = GC.gathered(c)
    par = c["kinds"][2]
    ok = [k for k in par if np.isfinite(s[k]).all() and (s[k] ** 2).sum() > 0]
    assert len(ok) >= 10
    for eps in (1e-6, 1e-9):
        k = np.isin(np.arange(len(p)), ok)
        u = (s[k] / np.linalg.norm(s[k], axis=1, keepdims=True)).astype(np.longdouble)
        t = G.terms_ld(u.astype(np.float64) * 0, s[k], -u.astype(np.float64), n[k], np.eye(4), eps)   # r = the unit normal
        assert np.abs(t[:, 28].astype(np.float64) * 2 * eps - 1.0).max() < 1e-6


@pytest.fixture(scope="module")
def aligned(mvr):
    out = {}
    for name in GC.ALIGN:
        c = GC.align_case(mvr, name)
        sn, tn = G.knn_normals(c["src"], GC.K_NORMALS), G.knn_normals(c["tgt"], GC.K_NORMALS)
        prm = G.params(max_corr_dist=c["max_dist"])
        out[name] = G.align(c["src"], sn, c["tgt"], tn, prm, G.tree_search(c["tgt"], c["max_dist"], False)) + (prm,)
    return out


def test_conditions_of_the_align_cases(mvr, aligned):
    for name in GC.ALIGN:
        c = GC.align_case(mvr, name)
        fin, st, trace, prm = aligned[name]
        assert st["state"] == "TRANSFORM" and st["converged"] and 2 <= st["iterations"] < prm["max_iterations"], (name, st)
        assert all(2 <= t["info"]["evaluations"] <= 20 for t in trace) and trace[-1]["delta"] < 1.0 <= trace[-2]["delta"]
        start, end = G.rms_to(np.eye(4), c["T_true"], c["src"]), G.rms_to(fin, c["T_true"], c["src"])
        print("%s: rms to the true pose %.3f -> %.3f mm in %d iterations, evaluations %s" % (name, start, end, st["iterations"], [t["info"]["evaluations"] for t in trace]))
        assert end < start
        if name == "synth_6001":
            svd = G.rms_to(G.svd_icp(c["src"], c["tgt"], c["max_dist"], 50), c["T_true"], c["src"])
            print("  reciprocal SVD ICP, 50 iterations: %.3f mm" % svd)
            assert end <= 0.5 * start and end <= svd


def test_the_true_pose_is_the_turntable_step(mvr):
    c = GC.align_case(mvr, "synth_6001")
    sp = mvr.synth_params(12, 1)
    raw = mvr.synth_view(sp, 1, 6001)[:, :3].astype(np.float64)
    piv, ax = mvr.synth_prior(sp)
    prior = mvr.axis_rotation(piv, ax, mvr.turntable_angle(1, 12))
    posed = raw @ prior[:3, :3].T + prior[:3, 3]
    assert np.abs(posed - c["src"][:, :3]).max() < 1e-4                    # the source is the raw view under the prior
    true_axis = np.array(sp.axis) / np.linalg.norm(np.array(sp.axis))
    on_view0 = raw @ mvr.axis_rotation(np.array(sp.pivot), true_axis, mvr.turntable_angle(1, 12))[:3, :3].T
    on_view0 += mvr.axis_rotation(np.array(sp.pivot), true_axis, mvr.turntable_angle(1, 12))[:3, 3]
    via = posed @ c["T_true"][:3, :3].T + c["T_true"][:3, 3]
    assert np.abs(via - on_view0).max() < 1e-9
    # ... and it lays view 1 onto the surface view 0 samples: the nearest view-0 point is within the sampling distance
    from scipy.spatial import cKDTree
    d, _ = cKDTree(c["tgt"][:, :3].astype(np.float64)).query(via)
    d0, _ = cKDTree(c["tgt"][:, :3].astype(np.float64)).query(posed)
    assert np.median(d) < np.median(d0)


def test_null_and_out_of_range_arguments_are_refused(mvr):
    lib = mvr._lib
    T = np.full(16, 5.0, np.float32)
    Tp = T.ctypes.data_as(C.POINTER(C.c_float))
    X = np.full(16, 7.0)
    Xp = X.ctypes.data_as(C.POINTER(C.c_double))
    out = np.full(29, 9.0)
    p = mvr.gicp_params()
    assert (p.max_corr_dist, p.use_reciprocal, p.fma_dist, p.max_iterations, p.max_inner_iterations) == (5.0, 0, 0, 200, 20)
    assert (p.transformation_epsilon, p.rotation_epsilon, p.gicp_epsilon, p.inner_rot_tol, p.inner_trans_tol, p.inner_chunk) == (5e-4, 2e-3, 1e-3, 1e-6, 1e-5, 4)
    assert mvr.gicp_params(max_corr_dist=4, gicp_epsilon=0.5, inner_chunk=3).inner_chunk == 3
    with pytest.raises(TypeError):
        mvr.gicp_params(nonsense=1)
    q = np.zeros(3, np.int32)
    qp = q.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.mvr_icp_align_gicp(None, 0, 1, 2, C.byref(p), None, 0, Tp, None, None, 0) == mvr.E_ARG
    assert lib.mvr_gicp_sums(None, 0, 1, qp, qp, 3, Xp, 1e-3, out.ctypes.data_as(C.POINTER(C.c_double))) == mvr.E_ARG
    assert lib.mvr_gicp_solve(None, 0, 1, qp, qp, 3, C.byref(p), Xp, None) == mvr.E_ARG
    assert (T == 5.0).all() and (X == 7.0).all() and (out == 9.0).all()    # nothing written


def test_struct_layout_equals_the_bindings(mvr, tmp_path):
    P, Tr, In = mvr.GicpParams, mvr.GicpIterTrace, mvr.GicpInfo
    fields = [("mvr_gicp_params", P, [f[0] for f in P._fields_]), ("mvr_gicp_iter_trace", Tr, [f[0] for f in Tr._fields_]),
              ("mvr_gicp_info", In, [f[0] for f in In._fields_])]
    body, exp = [], []
    for cname, cls, names in fields:
        body.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        exp.append(C.sizeof(cls))
        for f in names:
            body.append('  printf("%%zu\\n", offsetof(%s, %s));' % (cname, f.rstrip("_")))
            exp.append(getattr(cls, f).offset)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mvr_hip.h"\nint main(void) {\n' + "\n".join(body) + "\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got == exp
    assert [f[0] for f in P._fields_] == ["max_corr_dist", "use_reciprocal", "fma_dist", "max_iterations", "max_inner_iterations", "transformation_epsilon",
                                          "rotation_epsilon", "gicp_epsilon", "inner_rot_tol", "inner_trans_tol", "inner_chunk"]
    for sym in ("mvr_gicp_default_params", "mvr_icp_align_gicp", "mvr_gicp_sums", "mvr_gicp_solve"):
        assert sym in mvr.SIGNATURES
