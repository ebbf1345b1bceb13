"""GPU tests of the correspondence rejectors (rules R1-R10 at mvr_correspondences_rejected in include/mvr_hip.h) against the numpy
reference of tests/reject_ref.py on the cases of tests/reject_cases.py:
  1. correspondences_rejected == the reference applied to correspondences() of the same slots: lists, counts and thresholds
     bit for bit, reciprocal or not, with and without fma;
  2. reject_correspondences on host lists (shuffled too), a list longer than one sweep of the grid, R8's and R10's refusals;
  3. an empty chain == correspondences();
  4. an align replayed iteration by iteration from its trace; 5. an empty chain against icp_align; 6. fewer than 3 survivors;
  7. the slots are left alone; 8. two runs give the same bits."""
import importlib

import numpy as np
import pytest

import reject_cases as RC
import reject_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_parity.py:17
S, T_, CUR, OUT = 20, 21, 22, 23
U32 = np.uint32


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def cases(mvr):
    return RC.build(mvr)


@pytest.fixture(scope="module")
def ctx(mvr):
    with mvr.Context(0) as c:
        yield c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def rej(mvr, chain):
    return [mvr.rejector(*r) for r in chain]


def load(ctx, case, s=S, t=T_):
    ctx.upload(s, case["src"])
    ctx.upload(t, case["tgt"])
    if "snrm" in case:
        ctx.upload_normals(s, case["snrm"])
        ctx.upload_normals(t, case["tnrm"])


def same_lists(got, exp, what):
    for g, e, name in zip(got[:2], exp[:2], ("query", "match")):
        assert np.array_equal(g, e), (what, name)
    assert np.array_equal(bits(got[2]), bits(exp[2])), (what, "d2")


def same_stages(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        assert (g["n_in"], g["n_out"]) == (e["n_in"], e["n_out"]), (what, k, g, e)
        assert bits([g["threshold"]])[0] == bits([e["threshold"]])[0], (what, k, g, e)


@pytest.mark.parametrize("name", RC.NAMES)
def test_chain_after_the_search_equals_the_reference(mvr, ctx, cases, name):
    case = cases[name]
    load(ctx, case)
    done = 0
    for rec in (0, 1):
        for fma in (0, 1):
            base = ctx.correspondences(S, T_, case["max_dist"], reciprocal=bool(rec), fma=bool(fma))
            for chain, recs in case["chains"]:
                if rec not in recs:
                    continue
                exp = R.apply_chain(*base, chain, case.get("snrm"), case.get("tnrm"))
                got = ctx.correspondences_rejected(S, T_, case["max_dist"], rej(mvr, chain), reciprocal=bool(rec), fma=bool(fma))
                what = (name, chain, rec, fma)
                same_lists(got, exp, what)
                same_stages(got[3], exp[3], what)
                if not name.startswith("degenerate"):
                    assert all(3 <= s["n_out"] < s["n_in"] for s in got[3]), what
                done += 1
    assert done >= 2 * len(case["chains"])


def test_host_lists_equal_the_reference(mvr, ctx, cases):
    rng = np.random.default_rng(1)
    for name in ("lattice", "shared_target", "rand_257_palette", "synth_257"):
        case = cases[name]
        load(ctx, case)
        q, m, d = ctx.correspondences(S, T_, case["max_dist"], reciprocal=False)
        o = rng.permutation(len(q))
        for chain, _ in case["chains"]:
            exp = R.apply_chain(q, m, d, chain, case.get("snrm"), case.get("tnrm"))
            for order in (np.arange(len(q)), o):
                got = ctx.reject_correspondences(S, T_, q[order], m[order], d[order], rej(mvr, chain))
                same_lists(got, exp, (name, chain))
                same_stages(got[3], exp[3], (name, chain))
    # a list of the caller's own making: a sparse subset of the queries, +inf and +0 among the distances
    case = cases["rand_65"]
    load(ctx, case)
    q = np.array([64, 3, 17, 40, 5, 9, 33], np.int32)
    m = np.array([0, 256, 0, 7, 7, 7, 100], np.int32)
    d = np.array([np.inf, 0.0, 2.5, 1.0, 1.0, 1.0, np.inf], np.float32)
    for chain in ([("median", 1.0)], [("trimmed", 0.9)], [("one_to_one",)], [("trimmed", 1.0), ("one_to_one",), ("median", 1e30)], [("distance", 1e150)]):
        exp = R.apply_chain(q, m, d, chain)
        got = ctx.reject_correspondences(S, T_, q, m, d, rej(mvr, chain))
        same_lists(got, exp, chain)
        same_stages(got[3], exp[3], chain)


def test_a_list_longer_than_one_sweep(mvr, ctx):
    """BIG entries: the strided kernels go round twice and a trimmed block takes two tiles; four values of d2, so that the median
    and the cut lie in runs of tens of thousands of equal distances; every target is shared by three queries"""
    n = RC.BIG
    rng = np.random.default_rng(2)
    cloud = np.ones((n, 4), np.float32)
    cloud[:, :3] = rng.random((n, 3), np.float32)
    ctx.upload(S, cloud)
    ctx.upload(T_, cloud[:n // 3 + 1])
    q = np.arange(n, dtype=np.int32)
    m = (q // 3).astype(np.int32)
    d = rng.choice(np.array([0.5, 1.0, 2.0, 3.0], np.float32), n)
    d[rng.integers(0, n, 50)] = rng.random(50, np.float32)
    for chain in ([("median", 1.0), ("trimmed", 0.4)], [("trimmed", 0.77), ("one_to_one",)], [("one_to_one",), ("trimmed", 0.5), ("median", 0.9)]):
        exp = R.apply_chain(q, m, d, chain)
        got = ctx.reject_correspondences(S, T_, q, m, d, rej(mvr, chain))
        same_lists(got, exp, chain)
        same_stages(got[3], exp[3], chain)
        assert all(3 <= s["n_out"] < s["n_in"] for s in got[3]), (chain, got[3])
    ctx.clear(S)
    ctx.clear(T_)


def test_refusals(mvr, ctx, cases):
    case = cases["rand_65"]
    load(ctx, case)
    q, m, d = ctx.correspondences(S, T_, case["max_dist"], reciprocal=False)
    ok = [mvr.rejector("median", 2.0)]

    def refused(f, *a, **kw):
        with pytest.raises(mvr.MvrError) as e:
            f(*a, **kw)
        assert e.value.status == mvr.E_ARG, e.value

    # R8
    for bad in (dict(q=np.where(np.arange(len(q)) == 3, q[4], q)), dict(q=np.where(np.arange(len(q)) == 0, 65, q)), dict(q=np.where(np.arange(len(q)) == 0, -1, q)),
                dict(m=np.where(np.arange(len(q)) == 5, 257, m)), dict(m=np.where(np.arange(len(q)) == 5, -1, m)),
                dict(d=np.where(np.arange(len(q)) == 7, np.float32(np.nan), d)), dict(d=np.where(np.arange(len(q)) == 7, np.float32(-1.0), d))):
        refused(ctx.reject_correspondences, S, T_, bad.get("q", q), bad.get("m", m), bad.get("d", d), ok)
    # R10
    for chain in ([mvr.rejector(5)], [mvr.rejector(-1)], [mvr.rejector("median", np.nan)], [mvr.rejector("surface_normal", np.inf)],
                  [mvr.rejector("distance", -1.0)], [mvr.rejector("median", -0.5)], [mvr.rejector("trimmed", -0.1)],
                  [mvr.rejector("surface_normal", 0.5)],                              # (no normals in these slots: R5)
                  [mvr.rejector("one_to_one")] * (mvr.MAX_REJECTORS + 1)):
        refused(ctx.correspondences_rejected, S, T_, 30.0, chain)
        refused(ctx.reject_correspondences, S, T_, q, m, d, chain)
        refused(ctx.icp_align_rejected, S, T_, OUT, mvr.icp_params(), chain)
    refused(ctx.correspondences_rejected, mvr.MAX_SLOTS, T_, 30.0, ok)
    refused(ctx.correspondences_rejected, S, -1, 30.0, ok)
    # a negative cosine is a legitimate threshold; empty clouds are no error
    ctx.clear(CUR)
    got = ctx.correspondences_rejected(CUR, T_, 30.0, ok)
    assert len(got[0]) == 0 and got[3][0]["n_in"] == got[3][0]["n_out"] == 0
    got = ctx.correspondences_rejected(S, CUR, 30.0, ok)
    assert len(got[0]) == 0
    T, st, rc = ctx.icp_align_rejected(S, CUR, -1, mvr.icp_params(), ok)
    assert rc == mvr.E_NOCORR and st["state"] == "NO_CORRESPONDENCES"


def test_empty_chain_equals_correspondences(mvr, ctx, cases):
    for name in ("synth_6001", "rand_65", "degenerate_n1", "degenerate_no_match"):
        case = cases[name]
        load(ctx, case)
        for rec in (False, True):
            base = ctx.correspondences(S, T_, case["max_dist"], reciprocal=rec)
            got = ctx.correspondences_rejected(S, T_, case["max_dist"], [], reciprocal=rec)
            same_lists(got, base, (name, rec))
            assert got[3] == []


def kabsch(p, q):
    """TransformationEstimationSVD in f64: the rigid motion that takes p to q"""
    mp, mq = p.mean(0), q.mean(0)
    H = (q - mq).T @ (p - mp)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    Rm = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, mq - Rm @ mp
    return T


def point_to_plane(p, q, n):
    """TransformationEstimationPointToPlaneLLS in f64"""
    A = np.concatenate([np.cross(p, n), n], 1)
    b = (n * (q - p)).sum(1)
    x = np.linalg.solve(A.T @ A, A.T @ b)
    (ca, cb, cg), (sa, sb, sg) = np.cos(x[:3]), np.sin(x[:3])
    T = np.eye(4)
    T[:3, :3] = [[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca], [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca],
                 [-sb, cb * sa, cb * ca]]
    T[:3, 3] = x[3:]
    return T


@pytest.fixture(scope="module")
def pair_4097(mvr):
    return RC._synth_pair(mvr, 4097, 4097, normals=True)


@pytest.mark.parametrize("plane", [False, True])
def test_align_replayed_from_its_trace(mvr, ctx, pair_4097, plane):
    pair = pair_4097
    load(ctx, pair)
    chain = [("median", 2.0), ("trimmed", 0.8)] + ([("surface_normal", 0.999)] if plane else [])
    p = mvr.icp_params(reciprocal=True, max_dist=4.0, max_iter=6, teps=0.0, feps=0.0, point_to_plane=plane)
    T, st, rc, trace = ctx.icp_align_rejected(S, T_, OUT, p, rej(mvr, chain), return_trace=True)
    assert rc == 0 and st["iterations"] == len(trace) == 6 and st["state"] == "ITERATIONS"
    tgt, tnrm = pair["tgt"][:, :3].astype(np.float64), pair["tnrm"][:, :3].astype(np.float64)
    ctx.transform_f32(CUR, S, np.eye(4, dtype=np.float32))                 # the current source, normals with it
    fin = np.eye(4, dtype=np.float32)
    worst = [0.0, 0.0]
    for k, it in enumerate(trace):
        found = ctx.correspondences(CUR, T_, 4.0, reciprocal=True)
        q, m, d, stages = ctx.correspondences_rejected(CUR, T_, 4.0, rej(mvr, chain), reciprocal=True)
        assert it["n_found"] == len(found[0]) and it["n_corr"] == len(q) >= 3
        same_stages(it["stages"], stages, k)
        assert all(s["n_out"] < s["n_in"] for s in stages[:2]), (k, stages)
        mse = d.astype(np.float64).sum() / len(d)
        assert abs(it["mse"] - mse) <= 1e-12 * mse, (k, it["mse"], mse)
        cur = ctx.download(CUR)[:, :3].astype(np.float64)
        Te = point_to_plane(cur[q], tgt[m], tnrm[m]) if plane else kabsch(cur[q], tgt[m])
        dr, dt = np.abs(it["tr"][:3, :3] - Te[:3, :3]).max(), np.abs(it["tr"][:3, 3] - Te[:3, 3]).max()
        worst = [max(worst[0], dr), max(worst[1], dt)]
        assert dr <= ROT_TOL and dt <= TRANS_TOL, (k, dr, dt)
        assert np.array_equal(it["tr"][3], [0, 0, 0, 1])
        fin = mvr.mat4f_mul(it["tr"], fin)
        ctx.transform_f32(CUR, CUR, it["tr"])
    print("replay (%s): rotation within %.2g, translation within %.2g; survivors %s, mse %.4g -> %.4g"
          % ("point to plane" if plane else "SVD", worst[0], worst[1], [it["n_corr"] for it in trace], trace[0]["mse"], trace[-1]["mse"]))
    assert np.array_equal(bits(T), bits(fin)) and st["n_corr"] == trace[-1]["n_corr"] and st["mse"] == trace[-1]["mse"]
    # the output is final * input, normals rotated with it
    ctx.transform_f32(CUR, S, T)
    assert np.array_equal(bits(ctx.download(OUT)), bits(ctx.download(CUR)))
    assert np.array_equal(bits(ctx.download_normals(OUT)), bits(ctx.download_normals(CUR)))
    assert trace[-1]["mse"] < trace[0]["mse"]


def test_empty_chain_against_icp_align(mvr, ctx, cases, pair_4097):
    for pair, kw in ((cases["synth_6001"], dict(max_iter=5, teps=1e-9, feps=1e-6)), (pair_4097, dict(max_iter=10)),
                     (pair_4097, dict(max_iter=4, teps=0.0, feps=0.0, reciprocal=False))):
        load(ctx, pair)
        p = mvr.icp_params(max_dist=4.0, **kw)
        T0, st0, rc0 = ctx.icp_align(S, T_, OUT, p)
        T1, st1, rc1, trace = ctx.icp_align_rejected(S, T_, CUR, p, [], return_trace=True)
        assert rc0 == rc1 == 0
        assert (st0["iterations"], st0["state"], st0["n_corr"]) == (st1["iterations"], st1["state"], st1["n_corr"]), (st0, st1)
        dr, dt = np.abs(T0[:3, :3] - T1[:3, :3]).max(), np.abs(T0[:3, 3] - T1[:3, 3]).max()
        assert dr <= ROT_TOL and dt <= TRANS_TOL, (dr, dt)
        if st0["iterations"] == 1:                         # the same correspondences, summed in another order
            assert abs(st0["mse"] - st1["mse"]) <= 1e-12 * st0["mse"]
        assert len(trace) == st1["iterations"] and all(t["n_found"] == t["n_corr"] and t["stages"] == [] for t in trace)


def test_fewer_than_three_survivors(mvr, ctx, cases):
    load(ctx, cases["synth_257"])
    p = mvr.icp_params(max_dist=40.0, max_iter=5, teps=0.0, feps=0.0)
    T, st, rc, trace = ctx.icp_align_rejected(S, T_, -1, p, [mvr.rejector("trimmed", 0.0, 2)], return_trace=True)
    assert rc == mvr.E_NOCORR and st["state"] == "NO_CORRESPONDENCES" and not st["converged"]
    assert st["iterations"] == 0 and st["n_corr"] == 2 and np.array_equal(T, np.eye(4, dtype=np.float32))
    assert len(trace) == 1 and trace[0]["n_corr"] == 2 and trace[0]["stages"][0]["n_out"] == 2 and trace[0]["n_found"] > 100


def test_slots_are_left_alone_and_runs_repeat(mvr, ctx, cases):
    case = cases["synth_normals_6001"]
    load(ctx, case)
    chain = rej(mvr, [("median", 2.0), ("one_to_one",), ("trimmed", 0.7), ("surface_normal", 0.9995)])
    a = ctx.correspondences_rejected(S, T_, 4.0, chain, reciprocal=False)
    for slot, key, nkey in ((S, "src", "snrm"), (T_, "tgt", "tnrm")):
        assert np.array_equal(bits(ctx.download(slot)), bits(case[key])) and np.array_equal(bits(ctx.download_normals(slot)), bits(case[nkey]))
    b = ctx.correspondences_rejected(S, T_, 4.0, chain, reciprocal=False)
    same_lists(a, b, "again")
    same_stages(a[3], b[3], "again")
    assert all(3 <= s["n_out"] < s["n_in"] for s in a[3]), a[3]
    p = mvr.icp_params(max_dist=4.0, max_iter=4, teps=0.0, feps=0.0)
    r0 = ctx.icp_align_rejected(S, T_, OUT, p, chain, return_trace=True)
    out0 = ctx.download(OUT)
    with mvr.Context(0) as other:                          # a context that has run nothing else
        load(other, case)
        r1 = other.icp_align_rejected(S, T_, OUT, p, chain, return_trace=True)
        out1 = other.download(OUT)
    assert np.array_equal(bits(r0[0]), bits(r1[0])) and np.array_equal(bits(out0), bits(out1))
    for t0, t1 in zip(r0[3], r1[3]):
        assert t0["n_corr"] == t1["n_corr"] and t0["mse"] == t1["mse"] and np.array_equal(bits(t0["tr"]), bits(t1["tr"]))
        same_stages(t0["stages"], t1["stages"], "two contexts")
    assert np.array_equal(bits(ctx.download(S)), bits(case["src"]))
