"""GPU tests of the Generalized-ICP optimiser on the branch cases of tests/gicp_cases.py: every branch of gicp_step_kernel
(csrc/mvr_gicp.hip; rules G5-G7 in include/mvr_hip.h) against the numpy reference of tests/gicp_ref.py, decision by decision.

max_inner_iterations only caps the loop, so gicp_solve(max_inner_iterations=k) returns the state after k evaluations:
  1. for every k up to the reference's count: while every decision so far is DECIDED (gicp_ref.decided: |f_c - f| above 1e-9 of
     the terms' absolute values -- ten times the bound each sum is held to -- or every term exactly 0), evaluations, accepted and
     lambda equal the reference's exactly, rc its status, and X its X: the largest displacement of a listed source point is
     within TRANS_TOL, and outside the far frames the entries are within the parity bars.  At every k, decided or not, the
     checks that need no reference: f1 does not rise with k, f1 is the objective at the GPU's own X, lambda follows from the
     GPU's own decisions by G7's operations, X[3] = (0, 0, 0, 1), R R^T = I within 1e-13.  The full run is a run capped at its own
     count, bit for bit, at inner_chunk 1, 4 and 0;
  2. the sums for gicp_epsilon from 1e-1 down to 1e-9 against the long-double terms (gicp_ref.terms_ld) within 1e-13 / eps of the
     sum of the terms' absolute values -- the 1e-10 of eps = 1e-3 continued along the 1 / eps law of the inverse -- and in frames
     1e4, 1e5 and 1e6 away within the unchanged 1e-10;
  3. the unit of length: clouds, targets and inner_trans_tol times 2^-30 ... 2^30 give the same bits of R, t / scale,
     f / scale^2 and the same counters;
  4. the non-finite rule of G7, and a NaN in a point the list does not name.

The bar on f1 against the objective F that numpy recomputes at the GPU's X is 1e-9 F, unless the roundings of y = R p + t
alone -- which the two sides do not share -- can move F by more than that: then it is the first-order bound of that effect,
B = (2 / m) sum_i sum_c |(W r)_ic| dy_ic, with W and r = y - q of the very list and
dy_ic = 12 * 2^-53 * (|R_c0 p_x| + |R_c1 p_y| + |R_c2 p_z| + |t_c|): three products and three sums, each rounded by at most
2^-53 of a value no larger than that sum, on each of the two sides.  B / F grows as 1 / |r|: with coordinates near 900 it
passes 1e-9 once the residuals fall under a few thousandths of a unit, long before r is "nothing but rounding".  A fixed floor
on F below which the term is let in was tried at 1e-13 and is wrong: two decided steps above it differ by more than 1e-9 F
between two correct f64 evaluations (exact_shift at evaluation 5, F = 3.4e-11: 1.7e-9 F; coplanar at evaluation 6,
F = 6.6e-10: 1.6e-9 F), besides all_equal_away's last step (F = 1.5e-23: 0.02 F).  The test prints, per
case, the worst |f1 - F| / F, and every step that differs by more than 1e-9 F with the bound it is held to."""
import importlib

import numpy as np
import pytest

import gicp_cases as GC
import gicp_ref as G
from conftest import PKG

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_parity.py:17
SUM_TOL = 1e-10
S, T_ = 20, 21
U32, U64 = np.uint32, np.uint64


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    with mvr.Context(0) as c:
        yield c


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U32 if a.dtype == np.float32 else U64)


def load_list(ctx, c):
    ctx.upload(S, c["src"])
    ctx.upload(T_, c["tgt"])
    ctx.upload_normals(S, c["snrm"])
    ctx.upload_normals(T_, c["tnrm"])


def solve(mvr, ctx, c, **kw):
    return ctx.gicp_solve(S, T_, c["query"], c["match"], mvr.gicp_params(**kw))


def same_run(a, b):
    return a[2] == b[2] and np.array_equal(bits(a[0]), bits(b[0])) and a[1]["evaluations"] == b[1]["evaluations"] \
        and a[1]["accepted"] == b[1]["accepted"] and all(bits(np.float64(a[1][k]).reshape(1))[0] == bits(np.float64(b[1][k]).reshape(1))[0]
                                                          for k in ("lambda", "f0", "f1"))


def displacement(X, Y, p):
    d = p @ (np.asarray(X, np.float64) - Y)[:3, :3].T + (np.asarray(X, np.float64) - Y)[:3, 3]
    return float(np.sqrt((d * d).sum(1)).max())


def objective_bar(F, g, X, eps):
    """(the bar, whether it is the rounding bound B and not 1e-9 F)"""
    p, s, q, n = g
    r = p @ X[:3, :3].T + X[:3, 3] - q
    Wr = np.abs(np.einsum("mab,mb->ma", G.weights(s, n, eps), r))
    dy = 12.0 * 2.0 ** -53 * (np.abs(p) @ np.abs(X[:3, :3]).T + np.abs(X[:3, 3]))
    B = 2.0 / len(p) * float((Wr * dy).sum())
    return max(1e-9 * F, B), B > 1e-9 * F


def reference_free(name, k, X, info, g, decisions, eps=1e-3):
    """what holds of any run, whatever the reference decided"""
    assert np.array_equal(X[3], [0, 0, 0, 1]) and np.abs(X[:3, :3] @ X[:3, :3].T - np.eye(3)).max() <= 1e-13, (name, k)
    F = G.objective(*g, X, eps)
    bar, rounding = objective_bar(F, g, X, eps)
    err = abs(info["f1"] - F)
    if rounding and err > 1e-9 * F:
        print("%s evaluation %d: F %.3g, |f1 - F| / F = %.3g against the rounding bound %.3g" % (name, k, F, err / F, bar / F))
    assert err <= bar, (name, k, info["f1"], F, bar)
    assert info["lambda"] == G.lambda_of(decisions), (name, k, decisions, info["lambda"])
    assert info["accepted"] == decisions.count("A") and info["evaluations"] == len(decisions) + 1
    return abs(info["f1"] - F) / F if F > 0 else 0.0


@pytest.mark.parametrize("name", GC.BRANCH_NAMES)
def test_the_trajectory_decision_by_decision(mvr, ctx, name):
    want, c = GC.BRANCH[name], GC.branch_case(name)
    load_list(ctx, c)
    g = GC.gathered(c)
    Xr, ir, status, log = GC.reference_run(name)
    K, prefix, kw = ir["evaluations"], GC.decided_prefix(log), GC.branch_params(name)
    assert 1 <= K <= 34
    full = [solve(mvr, ctx, c, inner_chunk=ch, **kw) for ch in (1, 4, 0)]
    assert same_run(full[0], full[1]) and same_run(full[0], full[2]), name
    if want["end"] == "singular":
        X, info, rc = full[0]
        assert rc == mvr.E_SINGULAR == status and info["evaluations"] == 1 == K and info["accepted"] == 0 and info["lambda"] == 1e-3
        assert np.array_equal(bits(X), bits(np.eye(4)))
        # under a cap of 1 the non-finite rule still fires (it belongs to the first evaluation); the pivot test does not (it
        # belongs to the step, and the cap comes first), as in the reference
        X1, i1, rc1 = solve(mvr, ctx, c, max_inner_iterations=1)
        assert rc1 == G.solve(*g, G.params(max_inner_iterations=1))[2] == (0 if name == "collinear_origin" else mvr.E_SINGULAR)
        assert same_run((X, info, rc1), (X1, i1, rc1))
        if name == "collinear_origin":
            assert np.isfinite(info["f0"]) and abs(info["f0"] - ir["f0"]) <= 1e-9 * ir["f0"] and info["f1"] == info["f0"]
        else:
            assert not np.isfinite(info["f0"]) and not np.isfinite(info["f1"])
        print("%s: E_SINGULAR after 1 evaluation, X = I, f0 %r" % (name, info["f0"]))
        return
    runs, decisions, worst, worst_f, worst_k = [], "", 0.0, 0.0, 0
    for k in range(1, K + 1):
        X, info, rc = run = solve(mvr, ctx, c, **dict(kw, max_inner_iterations=k))
        runs.append(run)
        if k > 1 and info["evaluations"] == k:             # the GPU's own decision at evaluation k, from its counters
            decisions += "A" if info["accepted"] == runs[-2][1]["accepted"] + 1 else "R"
        if k > 1:
            assert info["f1"] <= runs[-2][1]["f1"] and info["f0"] == runs[0][1]["f0"], (name, k)
            if info["evaluations"] < k:                    # ended before the cap: the same state as under the cap before
                assert same_run(run, runs[-2]), (name, k)
        worst_f = max(worst_f, reference_free(name, k, X, info, g, decisions))
        if k <= prefix:
            Xk, lam, acc = GC.state_after(log, k)
            assert rc == 0 and (info["evaluations"], info["accepted"], info["lambda"]) == (k, acc, lam), (name, k, info, acc, lam)
            d = displacement(X, Xk, g[0])
            if d > worst:
                worst, worst_k = d, k
            assert d <= TRANS_TOL, (name, k, d)
            if name not in GC.FAR_FRAMES:
                dr, dt = np.abs(X[:3, :3] - Xk[:3, :3]).max(), np.abs(X[:3, 3] - Xk[:3, 3]).max()
                assert dr <= ROT_TOL and dt <= TRANS_TOL, (name, k, dr, dt)
    assert abs(runs[0][1]["f0"] - ir["f0"]) <= 1e-9 * ir["f0"]
    if prefix >= 2:
        assert decisions[:prefix - 1] == G.pattern(log)[:prefix - 1]
    # the full run is the run capped at its own count
    E = full[0][1]["evaluations"]
    assert full[0][2] == 0 and (E == K if prefix == K else prefix <= E <= kw.get("max_inner_iterations", 20))
    capped = runs[E - 1] if E <= K else solve(mvr, ctx, c, **dict(kw, max_inner_iterations=E))
    assert same_run(full[0], capped), (name, E)
    print("%s: %s (reference %s), %d evaluations, lambda %g; decided up to evaluation %d of %d; worst displacement %.3g at evaluation %d, "
          "worst |f1 - F| / F %.3g; f %.6g -> %.6g" % (name, decisions, G.pattern(log), E, full[0][1]["lambda"], prefix, K, worst, worst_k,
                                                       worst_f, full[0][1]["f0"], full[0][1]["f1"]))
    if name == "exact_fit":
        X, info, rc = full[0]
        assert np.array_equal(bits(X), bits(np.eye(4))) and info["f0"] == 0.0 and info["f1"] == 0.0
        assert info["evaluations"] == 14 and info["accepted"] == 0 and info["lambda"] == 1e10 and decisions == "R" * 13


@pytest.mark.parametrize("name", ["palette", "rand_65"])
def test_sums_over_the_range_of_epsilon(mvr, ctx, name):
    c = GC.list_case(name)
    load_list(ctx, c)
    g = GC.gathered(c)
    for eps in (1e-1, 1e-3, 1e-6, 1e-9):
        worst = 0.0
        for X in (np.eye(4), GC.sums_pose()):
            got = ctx.gicp_sums(S, T_, c["query"], c["match"], X, eps)
            exp, tot = G.sums_ld(*g, X, eps)
            assert got[27] == len(c["query"]) == exp[27]
            err = np.abs(got - exp)
            worst = max(worst, float(np.max(err[tot > 0] / tot[tot > 0])))
            assert (err <= 1e-13 / eps * tot).all(), (name, eps, err / np.maximum(tot, 1e-300))
        print("%s eps %g: worst |sum - reference| / sum |terms| = %.3g = %.3g / eps (bar 1e-13 / eps)" % (name, eps, worst, worst * eps))


@pytest.mark.parametrize("name", ["far_1e4", "far_1e5", "far_1e6"])
def test_sums_in_far_frames(mvr, ctx, name):
    c = GC.branch_case(name)
    load_list(ctx, c)
    g = GC.gathered(c)
    off = float(name.split("_")[1]) * np.array(GC.FAR_DIR)
    assert np.abs(g[0].mean(0) - off).max() < 1000.0
    worst = 0.0
    for X in (np.eye(4), GC.small_motion(np.random.default_rng(50), angle=0.3, shift=3.0, centre=off + np.array([0.0, 0.0, 900.0]))):
        got = ctx.gicp_sums(S, T_, c["query"], c["match"], X, 1e-3)
        exp, tot = G.sums_ld(*g, X, 1e-3)
        assert got[27] == len(c["query"]) == exp[27]
        err = np.abs(got - exp)
        worst = max(worst, float(np.max(err[tot > 0] / tot[tot > 0])))
        assert (err <= SUM_TOL * tot).all(), (name, err / np.maximum(tot, 1e-300))
    print("%s: worst |sum - reference| / sum |terms| = %.3g" % (name, worst))


@pytest.mark.parametrize("name", GC.UNIT_CASES)
def test_the_unit_of_length(mvr, ctx, name):
    c = GC.any_case(name)
    load_list(ctx, c)
    X0, i0, rc0 = solve(mvr, ctx, c)
    assert rc0 == 0 and i0["evaluations"] >= 7
    for s in GC.UNIT_SCALES:
        load_list(ctx, GC.in_unit(c, s))
        X, info, rc = solve(mvr, ctx, c, inner_trans_tol=1e-5 * s)
        assert rc == 0 and np.array_equal(bits(X[:3, :3]), bits(X0[:3, :3])), (name, s)
        assert np.array_equal(bits(X[:3, 3] / s), bits(X0[:3, 3])) and np.array_equal(X[3], [0, 0, 0, 1]), (name, s)
        assert (info["evaluations"], info["accepted"], info["lambda"]) == (i0["evaluations"], i0["accepted"], i0["lambda"]), (name, s)
        assert info["f1"] / s ** 2 == i0["f1"] and info["f0"] / s ** 2 == i0["f0"], (name, s)
    print("%s: %d evaluations, %d accepted at every scale" % (name, i0["evaluations"], i0["accepted"]))


def test_the_non_finite_rule(mvr, ctx):
    for name in ("nan_point", "inf_target"):
        c = GC.branch_case(name)
        load_list(ctx, c)
        for kw in (dict(), dict(inner_chunk=0), dict(max_inner_iterations=60), dict(gicp_epsilon=1.0)):
            X, info, rc = solve(mvr, ctx, c, **kw)
            assert rc == mvr.E_SINGULAR and info["evaluations"] == 1 and info["accepted"] == 0 and np.array_equal(bits(X), bits(np.eye(4)))
            assert not np.isfinite(info["f0"])
        sm = ctx.gicp_sums(S, T_, c["query"], c["match"])
        assert sm[27] == len(c["query"]) and not np.isfinite(sm[28])
    # a NaN in source points the list does not name changes nothing
    clean, dirty = GC.unlisted_nan()
    out = []
    for c in (clean, dirty):
        load_list(ctx, c)
        out.append((solve(mvr, ctx, c), [ctx.gicp_sums(S, T_, c["query"], c["match"], X) for X in (np.eye(4), GC.sums_pose())]))
    assert out[0][0][2] == 0 and same_run(out[0][0], out[1][0])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(out[0][1], out[1][1])) and np.isfinite(out[0][1][0]).all()
