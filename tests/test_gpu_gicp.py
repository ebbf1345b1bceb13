"""GPU tests of Generalized ICP (rules G1-G10 at mvr_icp_align_gicp in include/mvr_hip.h) against the numpy reference of
tests/gicp_ref.py on the cases of tests/gicp_cases.py:
  1. gicp_sums == the reference's sums within 1e-10 of the sum of the terms' absolute values, the count exactly;
  2. gicp_solve == the reference's solve within the parity bars, its counters and lambda exactly while the reference's decisions
     are decided (gicp_ref.decided), at or below scipy's minimum, == Umeyama at eps = 1, singular;
  3. inner_chunk 1, 3 and 0 and two runs give the same bits; 4. an align replayed iteration by iteration from its trace;
  5. the accuracy conditions of synth_6001 on the GPU's result; 6. refusals, too few survivors, empty clouds, the slots are left
  alone, out = T_out applied to the input.

The bound of 1: each term goes through an inverse of condition <= 1 / eps = 1000 and a few dozen f64 operations, which is
<~ 5e-12 relative; the fixed-order sum adds less (the reference's sums are exactly rounded).  1e-10 leaves a margin of ~20x."""
import importlib

import numpy as np
import pytest

import gicp_cases as GC
import gicp_ref as G
from conftest import PKG

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_parity.py:17
SUM_TOL = 1e-10
S, T_, CUR, OUT = 20, 21, 22, 23
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


def load_list(ctx, c, s=S, t=T_):
    ctx.upload(s, c["src"])
    ctx.upload(t, c["tgt"])
    ctx.upload_normals(s, c["snrm"])
    ctx.upload_normals(t, c["tnrm"])


def load_align(ctx, c, s=S, t=T_):
    """the pair with 20-NN normals estimated on the device"""
    ctx.upload(s, c["src"])
    ctx.upload(t, c["tgt"])
    ctx.estimate_normals([s, t], k=GC.K_NORMALS)


def get_case(ctx, name):
    return GC.big_list(ctx.device_info()[1]) if name == "big" else GC.list_case(name)


def within_bars(X, Y, what):
    dr, dt = np.abs(np.asarray(X, np.float64)[:3, :3] - Y[:3, :3]).max(), np.abs(np.asarray(X, np.float64)[:3, 3] - Y[:3, 3]).max()
    assert dr <= ROT_TOL and dt <= TRANS_TOL, (what, dr, dt)
    return dr, dt


LISTS = GC.LIST_NAMES + ("big",)


@pytest.mark.parametrize("name", LISTS)
def test_sums_equal_the_reference(mvr, ctx, name):
    c = get_case(ctx, name)
    load_list(ctx, c)
    g = GC.gathered(c)
    if name == "big":
        assert len(c["query"]) == ctx.device_info()[1] * 256 + 257
    worst = 0.0
    for X in (np.eye(4), GC.sums_pose()):
        for eps in ((1e-3, 1.0) if name in ("palette", "rand_65") else (1e-3,)):
            got = ctx.gicp_sums(S, T_, c["query"], c["match"], X, eps)
            exp, tot = G.sums(*g, X, eps, with_abs=True)
            assert got[27] == len(c["query"]) == exp[27]
            err = np.abs(got - exp)
            ratio = float(np.max(err[tot > 0] / tot[tot > 0]))
            worst = max(worst, ratio)
            print("%s eps %g: worst |sum - reference| / sum |terms| = %.3g" % (name, eps, ratio))
            assert (err <= SUM_TOL * tot).all(), (name, eps, err / np.maximum(tot, 1e-300))
            again = ctx.gicp_sums(S, T_, c["query"], c["match"], X, eps)
            assert np.array_equal(bits(got), bits(again))
    assert worst < SUM_TOL


@pytest.mark.parametrize("name", LISTS)
def test_solve_equals_the_reference(mvr, ctx, name):
    c = get_case(ctx, name)
    load_list(ctx, c)
    p, s, q, n = g = GC.gathered(c)
    for eps in (1e-3, 1.0):
        X, info, rc = ctx.gicp_solve(S, T_, c["query"], c["match"], mvr.gicp_params(gicp_epsilon=eps))
        log = []
        Xr, ir, status = G.solve(*g, G.params(gicp_epsilon=eps), log=log)
        assert rc == status == 0
        dr, dt = within_bars(X, Xr, (name, eps))
        F_gpu = G.objective(*g, X, eps)
        print("%s eps %g: rotation within %.2g, translation within %.2g; %d evaluations (reference %d), F %.12g (reference %.12g)"
              % (name, eps, dr, dt, info["evaluations"], ir["evaluations"], F_gpu, ir["f1"]))
        # the counters equal the reference's, exactly, for as long as the reference's decisions are decided (gicp_ref.decided;
        # tests/test_gicp_host.py: all but the last one or two of these cases); max_inner_iterations = k is the state after k
        prefix = GC.decided_prefix(log)
        assert prefix >= 6
        for k in range(1, prefix + 1):
            _, ik, rck = ctx.gicp_solve(S, T_, c["query"], c["match"], mvr.gicp_params(gicp_epsilon=eps, max_inner_iterations=k))
            _, lam, acc = GC.state_after(log, k)
            assert rck == 0 and (ik["evaluations"], ik["accepted"], ik["lambda"]) == (k, acc, lam), (name, eps, k, ik)
        assert prefix <= info["evaluations"] <= 20 and prefix - 1 <= info["accepted"] < info["evaluations"]
        assert abs(info["f1"] - F_gpu) <= 1e-9 * F_gpu and abs(info["f0"] - ir["f0"]) <= 1e-9 * ir["f0"] and info["f1"] < info["f0"]
        assert F_gpu <= ir["f1"] * (1 + 1e-9)
        if name != "big":                                  # (scipy's numerical gradient over 50 000 points takes many seconds)
            assert F_gpu <= G.scipy_minimum(*g, eps) * (1 + 1e-9)
        assert np.array_equal(X[3], [0, 0, 0, 1]) and np.allclose(X[:3, :3] @ X[:3, :3].T, np.eye(3), atol=1e-13)
    # eps = 1: W = I / 2, the minimum is the SVD estimator's on the same list
    m2 = ctx.pair_moments2_from_corr(S, T_, c["query"], c["match"], np.zeros(3))
    Tu, _ = mvr.umeyama_from_moments(mvr.moments_from_moments2(m2))
    within_bars(X, Tu.astype(np.float64), (name, "umeyama"))


def test_solve_singular_and_short_lists(mvr, ctx):
    """All points equal is the singular case.  H = sum J^T W J then has rank 3, but G6 solves H + lambda diag(H), which is positive
    definite whenever diag(H) > 0; the pivot rule of G6 therefore fires when the common point is the origin, where J's rotation
    columns -- and with them three diagonal entries of H -- are exactly 0.  (Elsewhere such a list ends by G7's lambda > 1e9.)"""
    c = GC.list_case("rand_64")
    z = np.ones((5, 4), np.float32)
    z[:, :3] = 0.0                                         # every point at the origin: the rotation rows of H are 0 (G6's pivot)
    ctx.upload(S, z)
    ctx.upload(T_, z)
    ctx.upload_normals(S, c["snrm"][:5])
    ctx.upload_normals(T_, c["tnrm"][:5])
    idx = np.arange(5, dtype=np.int32)
    X, info, rc = ctx.gicp_solve(S, T_, idx, idx, mvr.gicp_params())
    assert rc == mvr.E_SINGULAR and info["evaluations"] == 1 and info["accepted"] == 0 and np.array_equal(X, np.eye(4))
    X, info, rc = ctx.gicp_solve(S, T_, idx[:2], idx[:2], mvr.gicp_params())
    assert rc == mvr.E_NOCORR and np.array_equal(X, np.eye(4))
    load_list(ctx, c)
    X, info, rc = ctx.gicp_solve(S, T_, c["query"], c["match"], mvr.gicp_params(max_inner_iterations=1))
    assert rc == 0 and info["evaluations"] == 1 and np.array_equal(X, np.eye(4))
    assert np.array_equal(ctx.gicp_sums(S, T_, [], []), np.zeros(29))


def same_trace(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        for key in ("n_found", "n_corr", "inner_evals", "inner_accepted", "stages"):
            assert x[key] == y[key], (what, k, key)
        for key in ("mse", "f0", "f1", "lambda"):
            assert bits(np.float64(x[key]).reshape(1))[0] == bits(np.float64(y[key]).reshape(1))[0], (what, k, key)
        assert np.array_equal(bits(x["tr"]), bits(y["tr"])), (what, k)


def test_chunks_and_runs_give_the_same_bits(mvr, ctx):
    c = GC.list_case("rand_6001")
    load_list(ctx, c)
    runs = [ctx.gicp_solve(S, T_, c["query"], c["match"], mvr.gicp_params(inner_chunk=ch)) for ch in (1, 3, 0, 0, 50)]
    for X, info, rc in runs[1:]:
        assert rc == 0 and np.array_equal(bits(X), bits(runs[0][0])) and info == runs[0][1]
    a = GC.align_case(mvr, "synth_2003")
    load_align(ctx, a)
    chain = [mvr.rejector("median", 2.0)]
    out = []
    for ch in (1, 3, 0, 0):
        out.append(ctx.icp_align_gicp(S, T_, OUT, mvr.gicp_params(max_corr_dist=a["max_dist"], inner_chunk=ch), chain, return_trace=True))
    with mvr.Context(0) as other:                          # a context that has run nothing else
        load_align(other, a)
        out.append(other.icp_align_gicp(S, T_, OUT, mvr.gicp_params(max_corr_dist=a["max_dist"]), chain, return_trace=True))
    T0, st0, rc0, tr0 = out[0]
    assert rc0 == 0 and st0["iterations"] == len(tr0) >= 2 and max(t["inner_evals"] for t in tr0) > 3
    for T, st, rc, tr in out[1:]:
        assert rc == 0 and np.array_equal(bits(T), bits(T0))
        assert (st["iterations"], st["state"], st["n_corr"], st["mse"]) == (st0["iterations"], st0["state"], st0["n_corr"], st0["mse"])
        same_trace(tr, tr0, "chunks")


@pytest.mark.parametrize("chain", [[], [("median", 2.0), ("trimmed", 0.8)]], ids=["empty", "median_trimmed"])
def test_align_replayed_from_its_trace(mvr, ctx, chain):
    a = GC.align_case(mvr, "synth_6001")
    load_align(ctx, a)
    rej = [mvr.rejector(*r) for r in chain]
    prm = G.params(max_corr_dist=a["max_dist"])
    T, st, rc, trace = ctx.icp_align_gicp(S, T_, OUT, mvr.gicp_params(max_corr_dist=a["max_dist"]), rej, return_trace=True)
    assert rc == 0 and st["converged"] and st["state"] == "TRANSFORM" and 2 <= st["iterations"] == len(trace) < 200
    tgt, tnrm = G.xyz(ctx.download(T_)), G.xyz(ctx.download_normals(T_))
    ctx.transform_f32(CUR, S, np.eye(4, dtype=np.float32))                 # the current source, normals with it
    fin = np.eye(4, dtype=np.float32)
    worst = [0.0, 0.0]
    for k, it in enumerate(trace):
        found = ctx.correspondences(CUR, T_, a["max_dist"], reciprocal=False)
        q, m, d, stages = ctx.correspondences_rejected(CUR, T_, a["max_dist"], rej, reciprocal=False)
        assert it["n_found"] == len(found[0]) and it["n_corr"] == len(q) >= 3
        assert [(s["n_in"], s["n_out"], bits(np.float32(s["threshold"]).reshape(1))[0]) for s in it["stages"]] == \
               [(s["n_in"], s["n_out"], bits(np.float32(s["threshold"]).reshape(1))[0]) for s in stages], k
        mse = d.astype(np.float64).sum() / len(d)
        assert abs(it["mse"] - mse) <= 1e-12 * mse, (k, it["mse"], mse)
        cur, cn = G.xyz(ctx.download(CUR)), G.xyz(ctx.download_normals(CUR))
        Xr, ir, status = G.solve(cur[q], cn[q], tgt[m], tnrm[m], prm)
        assert status == 0
        dr, dt = within_bars(it["tr"], Xr, k)
        worst = [max(worst[0], dr), max(worst[1], dt)]
        assert abs(it["f0"] - ir["f0"]) <= 1e-9 * ir["f0"] and abs(it["f1"] - ir["f1"]) <= 1e-9 * ir["f1"]
        assert 2 <= it["inner_evals"] <= 20 and 1 <= it["inner_accepted"] < it["inner_evals"]
        assert np.array_equal(it["tr"][3], [0, 0, 0, 1])
        new = mvr.mat4f_mul(it["tr"], fin)
        delta = G.outer_delta(new, fin, prm)                               # G8: the last iteration is the first below 1
        assert (delta < 1.0) == (k == len(trace) - 1), (k, delta)
        fin = new
        ctx.transform_f32(CUR, CUR, it["tr"])
    print("replay (%s): rotation within %.2g, translation within %.2g; survivors %s, evaluations %s, f %.4g -> %.4g"
          % (chain, worst[0], worst[1], [it["n_corr"] for it in trace], [it["inner_evals"] for it in trace], trace[0]["f0"], trace[-1]["f1"]))
    assert np.array_equal(bits(T), bits(fin)) and st["n_corr"] == trace[-1]["n_corr"] and st["mse"] == trace[-1]["mse"]
    # the output is final * input, normals rotated with it
    ctx.transform_f32(CUR, S, T)
    assert np.array_equal(bits(ctx.download(OUT)), bits(ctx.download(CUR)))
    assert np.array_equal(bits(ctx.download_normals(OUT)), bits(ctx.download_normals(CUR)))


def test_accuracy_on_the_turntable_pair(mvr, ctx):
    for name in GC.ALIGN:
        a = GC.align_case(mvr, name)
        load_align(ctx, a)
        before = bits(ctx.download(S)), bits(ctx.download_normals(S)), bits(ctx.download(T_)), bits(ctx.download_normals(T_))
        T, st, rc = ctx.icp_align_gicp(S, T_, -1, mvr.gicp_params(max_corr_dist=a["max_dist"]))
        assert rc == 0 and st["converged"] and st["state"] == "TRANSFORM" and st["iterations"] < 200, (name, st)
        after = bits(ctx.download(S)), bits(ctx.download_normals(S)), bits(ctx.download(T_)), bits(ctx.download_normals(T_))
        assert all(np.array_equal(x, y) for x, y in zip(before, after))  # the slots are left alone
        start, end = G.rms_to(np.eye(4), a["T_true"], a["src"]), G.rms_to(T, a["T_true"], a["src"])
        print("%s: rms to the true pose %.3f -> %.3f mm in %d iterations" % (name, start, end, st["iterations"]))
        assert end < start
        if name == "synth_6001":
            Ts, ss, rcs = ctx.icp_align(S, T_, -1, mvr.icp_params(reciprocal=True, max_dist=a["max_dist"], max_iter=50, teps=0.0, feps=0.0))
            svd = G.rms_to(Ts, a["T_true"], a["src"])
            print("  icp_align (reciprocal, SVD, %d iterations): %.3f mm" % (ss["iterations"], svd))
            assert rcs == 0 and end <= 0.5 * start and end <= svd


def test_refusals_and_edges(mvr, ctx):
    a = GC.align_case(mvr, "synth_2003")
    ok = mvr.gicp_params(max_corr_dist=a["max_dist"])

    def refused(f, *args, **kw):
        with pytest.raises(mvr.MvrError) as e:
            f(*args, **kw)
        assert e.value.status == mvr.E_ARG, e.value

    # G1: normals on both sides
    c = GC.list_case("rand_65")
    for have in ((), (S,), (T_,)):
        ctx.upload(S, c["src"])
        ctx.upload(T_, c["tgt"])
        for slot in have:
            ctx.upload_normals(slot, c["snrm"] if slot == S else c["tnrm"])
        refused(ctx.icp_align_gicp, S, T_, OUT, ok)
        refused(ctx.gicp_solve, S, T_, c["query"], c["match"], ok)
        refused(ctx.gicp_sums, S, T_, c["query"], c["match"])
    load_list(ctx, c)
    # G10
    nan, inf = float("nan"), float("inf")
    bad = [dict(gicp_epsilon=v) for v in (0.0, -1e-3, 1.0 + 1e-9, nan, inf)]
    for key in ("transformation_epsilon", "rotation_epsilon", "inner_rot_tol", "inner_trans_tol"):
        bad += [{key: v} for v in (0.0, -1.0, nan, inf)]
    bad += [dict(max_inner_iterations=0), dict(max_inner_iterations=-3)]
    for kw in bad:
        p = mvr.gicp_params(max_corr_dist=30.0, **kw)
        refused(ctx.icp_align_gicp, S, T_, OUT, p)
        refused(ctx.gicp_solve, S, T_, c["query"], c["match"], p)
    for eps in (0.0, 1.5, nan):
        refused(ctx.gicp_sums, S, T_, c["query"], c["match"], None, eps)
    # R10 and R8 carry over
    refused(ctx.icp_align_gicp, S, T_, OUT, ok, [mvr.rejector(7)])
    refused(ctx.icp_align_gicp, S, T_, OUT, ok, [mvr.rejector("one_to_one")] * (mvr.MAX_REJECTORS + 1))
    refused(ctx.icp_align_gicp, mvr.MAX_SLOTS, T_, OUT, ok)
    q, m = c["query"], c["match"]
    for bq, bm in ((np.where(np.arange(65) == 3, q[4], q), m), (np.where(np.arange(65) == 0, 65, q), m), (q, np.where(np.arange(65) == 5, -1, m)),
                   (q, np.where(np.arange(65) == 5, 65, m))):
        refused(ctx.gicp_sums, S, T_, bq, bm)
        refused(ctx.gicp_solve, S, T_, bq, bm, ok)
    # gicp_epsilon = 1 is inside the range
    assert ctx.gicp_solve(S, T_, q, m, mvr.gicp_params(gicp_epsilon=1.0))[2] == 0
    # empty clouds (R9)
    ctx.clear(CUR)
    for s, t in ((CUR, T_), (S, CUR)):
        T, st, rc = ctx.icp_align_gicp(s, t, -1, ok)
        assert rc == mvr.E_NOCORR and st["state"] == "NO_CORRESPONDENCES" and not st["converged"] and np.array_equal(T, np.eye(4, dtype=np.float32))
    # fewer than 3 survivors (G2)
    load_align(ctx, a)
    T, st, rc, trace = ctx.icp_align_gicp(S, T_, -1, ok, [mvr.rejector("trimmed", 0.0, 2)], return_trace=True)
    assert rc == mvr.E_NOCORR and st["state"] == "NO_CORRESPONDENCES" and not st["converged"]
    assert st["iterations"] == 0 and st["n_corr"] == 2 and np.array_equal(T, np.eye(4, dtype=np.float32))
    assert len(trace) == 1 and trace[0]["n_corr"] == 2 and trace[0]["stages"][0]["n_out"] == 2 and trace[0]["n_found"] > 100
    # max_iterations ends an align that has not settled: converged, as PCL
    T, st, rc = ctx.icp_align_gicp(S, T_, OUT, mvr.gicp_params(max_corr_dist=a["max_dist"], max_iterations=1))
    assert rc == 0 and st["converged"] and st["state"] == "ITERATIONS" and st["iterations"] == 1
    ctx.transform_f32(CUR, S, T)
    assert np.array_equal(bits(ctx.download(OUT)), bits(ctx.download(CUR)))
