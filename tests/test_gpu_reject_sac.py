"""GPU tests of the sample-consensus rejector (rules C1-C12 at mvr_reject_sample_consensus in include/mvr_hip.h) against the
numpy reference of tests/reject_sac_ref.py, which replays the library's answer from its trace, on the cases of
tests/reject_sac_cases.py:
  1. every case through the dedicated entry with a trace: checks (a)-(f) of the reference;
  2. result and trace bit-identical for every chunk size, with and without a trace, twice in a row, for a shuffled list;
  3. three routes to the same chain agree bit for bit; 4. an align with the stage replayed from its trace, its pose under gross
  outliers, last_sample_consensus(); 5. GICP accepts the stage; 6. C12's refusals, the slots left alone."""
import importlib

import numpy as np
import pytest

import reject_cases as RC
import reject_sac_cases as SC
import reject_sac_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

S, T_, CUR, OUT = 20, 21, 22, 23
U32 = np.uint32
bits = R.bits


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def cases():
    return SC.build()


@pytest.fixture(scope="module")
def ctx(mvr):
    with mvr.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def synth(mvr):
    return RC._synth_pair(mvr, 6001, 5000)


@pytest.fixture(scope="module")
def synth_normals(mvr):
    return RC._synth_pair(mvr, 4097, 4097, normals=True)


def rej_of(mvr, case):
    return mvr.rejector("sample_consensus", case["value"], max_iterations=case["max_iterations"], refine=case["refine"], seed=case["seed"])


def load(ctx, case):
    ctx.upload(S, case["src"])
    ctx.upload(T_, case["tgt"])
    if "snrm" in case:
        ctx.upload_normals(S, case["snrm"])
        ctx.upload_normals(T_, case["tnrm"])


def run(mvr, ctx, case, trace=True):
    return ctx.reject_sample_consensus(S, T_, case["q"], case["m"], case["d"], rej_of(mvr, case), return_trace=trace)


def same_result(a, b, what):
    for k in ("found", "live", "valid", "inliers", "ransac_inliers", "iterations", "attempts", "skipped", "best_attempt", "refine_rounds", "k"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert np.array_equal(bits(a["T"]), bits(b["T"])) and np.array_equal(bits(a["ransac_T"]), bits(b["ransac_T"])), what


def same_run(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2])), what
    same_result(a[3], b[3], what)
    if len(a) > 4 and len(b) > 4:
        for k in ("status", "query", "match", "inliers"):
            assert np.array_equal(a[4][k], b[4][k]), (what, k)
        assert np.array_equal(bits(a[4]["T"]), bits(b[4]["T"])) and np.array_equal(a[4]["k"].view(np.uint64), b[4]["k"].view(np.uint64)), what


@pytest.mark.parametrize("name", SC.NAMES)
def test_every_case_replayed_from_its_trace(mvr, ctx, cases, name):
    case = cases[name]
    load(ctx, case)
    got = run(mvr, ctx, case)
    fig = R.verify(case["src"], case["tgt"], case["q"], case["m"], case["d"], case["value"], case["max_iterations"], case["refine"], case["seed"],
                   got, check_c=case["check_c"])
    res = got[3]
    print("%s: %d attempts (%d counted, %.0f %% well conditioned), T within %.2g / %.2g of Kabsch; %d of %d kept, %d refine rounds"
          % (name, res["attempts"], fig["counted"], 100 * fig["well"], fig["worst_rot"], fig["worst_trans"], len(got[0]), len(case["q"]), res["refine_rounds"]))
    assert res["found"] == case["found"], name
    if case["check_c"] and res["attempts"]:
        assert fig["well"] >= 0.9, (name, fig["well"])
    if case["planted"] is not None:
        q, m, d = R.sort_list(case["q"], case["m"], case["d"])
        keep = case["planted"]
        assert np.array_equal(got[0], q[keep]) and np.array_equal(got[1], m[keep]) and np.array_equal(bits(got[2]), bits(d[keep])), name
        if case["refine"]:
            assert fig["refit_checked"], name
    same_result(ctx.last_sample_consensus(), res, name) if len(case["q"]) else None
    if name == "all_inliers":
        assert res["attempts"] == res["iterations"] == 1
    if name == "unrelated":
        assert res["attempts"] == 71 and res["inliers"] == len(case["q"])      # max_iterations + 1: more than the first chunk of 64
    assert np.array_equal(bits(ctx.download(S)), bits(case["src"])) and np.array_equal(bits(ctx.download(T_)), bits(case["tgt"]))


def test_the_synthetic_pair_replayed_from_its_trace(mvr, ctx, synth):
    load(ctx, synth)
    q, m, d = ctx.correspondences(S, T_, 4.0, reciprocal=False)
    assert len(q) > 4000
    for refine in (False, True):
        case = dict(synth, q=q, m=m, d=d, value=1.5, max_iterations=200, refine=refine, seed=11)
        got = run(mvr, ctx, case)
        fig = R.verify(synth["src"], synth["tgt"], q, m, d, 1.5, 200, refine, 11, got)
        res = got[3]
        print("synthetic pair (refine %d): %d attempts, %d of %d kept (RANSAC %d), %d refine rounds, T within %.2g / %.2g of Kabsch on %.0f %% of the attempts"
              % (refine, res["attempts"], res["inliers"], res["live"], res["ransac_inliers"], res["refine_rounds"], fig["worst_rot"], fig["worst_trans"], 100 * fig["well"]))
        assert res["found"] and 100 < res["inliers"] < res["live"]


def test_chunks_traces_repeats_and_order_do_not_change_a_bit(mvr, ctx, cases):
    for name in ("planted_257", "planted_30", "unrelated", "non_finite", "duplicates"):
        case = cases[name]
        load(ctx, case)
        ctx.tune(rej_sac_chunk=0)
        base = run(mvr, ctx, case)
        for chunk in (1, 7, 64, 65, 256):
            ctx.tune(rej_sac_chunk=chunk)
            same_run(run(mvr, ctx, case), base, (name, chunk))
        ctx.tune(rej_sac_chunk=0)
        same_run(run(mvr, ctx, case, trace=False), base, (name, "no trace"))
        same_run(run(mvr, ctx, case), base, (name, "again"))
        same_run(run(mvr, ctx, SC.shuffled(case)), base, (name, "shuffled"))
    with pytest.raises(mvr.MvrError):
        ctx.tune(rej_sac_chunk=257)


def sac(mvr, value=1.5, **kw):
    return mvr.rejector("sample_consensus", value, **dict(dict(max_iterations=200, seed=3), **kw))


@pytest.mark.parametrize("order", ["median_first", "one_to_one_last"])
def test_three_routes_agree(mvr, ctx, synth, order):
    load(ctx, synth)
    done = 0
    for rec in (False, True):
        for fma in (False, True):
            for refine in (False, True):
                stage = sac(mvr, refine=refine)
                chain = [mvr.rejector("median", 2.0), stage] if order == "median_first" else [stage, mvr.rejector("one_to_one")]
                k_sac = chain.index(stage)
                a = ctx.correspondences_rejected(S, T_, 4.0, chain, reciprocal=rec, fma=fma)
                last_a = ctx.last_sample_consensus()
                q, m, d = ctx.correspondences(S, T_, 4.0, reciprocal=rec, fma=fma)
                b = ctx.reject_correspondences(S, T_, q, m, d, chain)
                last_b = ctx.last_sample_consensus()
                if order == "median_first":
                    q1, m1, d1, st1 = ctx.reject_correspondences(S, T_, q, m, d, chain[:1])
                    c = ctx.reject_sample_consensus(S, T_, q1, m1, d1, stage)
                    c_stages = st1 + [dict(n_in=c[3]["live"], n_out=c[3]["inliers"], threshold=np.float32(0))]
                    before = (q1, m1, d1)
                else:
                    c0 = ctx.reject_sample_consensus(S, T_, q, m, d, stage)
                    q1, m1, d1, st1 = ctx.reject_correspondences(S, T_, c0[0], c0[1], c0[2], chain[1:])
                    c = (q1, m1, d1, c0[3])
                    c_stages = [dict(n_in=c0[3]["live"], n_out=c0[3]["inliers"], threshold=np.float32(0))] + st1
                    before = (q, m, d)
                what = (order, rec, fma, refine)
                # the list entries have no fma argument (C5): they agree with each other always, with the search's entry without fma
                for x, y in ((b, c),) + (((a, b),) if not fma else ()):
                    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(bits(x[2]), bits(y[2])), what
                same_result(last_b, c[3], what)
                assert [(s["n_in"], s["n_out"], float(s["threshold"])) for s in b[3]] == [(s["n_in"], s["n_out"], float(s["threshold"])) for s in c_stages], what
                if not fma:
                    same_result(last_a, last_b, what)
                    assert [(s["n_in"], s["n_out"]) for s in a[3]] == [(s["n_in"], s["n_out"]) for s in b[3]], what
                # the stage records of the search's entry, with fma too: in = what the stage before left, out = the C5 inliers of its T
                st = a[3]
                assert st[0]["n_in"] == len(q) and st[1]["n_in"] == st[0]["n_out"] and st[-1]["n_out"] == len(a[0]), what
                assert (st[k_sac]["n_in"], st[k_sac]["n_out"], float(st[k_sac]["threshold"])) == (last_a["live"], last_a["inliers"], 0.0), what
                assert last_a["found"] and 3 <= last_a["inliers"] < last_a["live"], what
                bq, bm, _ = before
                mask = R.inlier_mask(last_a["T"], synth["src"][bq, :3], synth["tgt"][bm, :3], 1.5, fma=fma)
                if order == "median_first":
                    assert np.array_equal(a[0], bq[mask]) and np.array_equal(a[1], bm[mask]), what
                else:
                    assert mask.sum() == st[0]["n_out"] and set(a[0]) <= set(bq[mask]), what
                done += 1
    assert done == 8


def kabsch(p, q):
    return R.kabsch(p, q)[0]


def test_align_replayed_from_its_trace(mvr, ctx, synth_normals):
    pair = synth_normals
    load(ctx, pair)
    chain = [sac(mvr, 1.0, refine=True), mvr.rejector("median", 2.0)]
    p = mvr.icp_params(reciprocal=True, max_dist=4.0, max_iter=5, teps=0.0, feps=0.0)
    T, st, rc, trace = ctx.icp_align_rejected(S, T_, OUT, p, chain, return_trace=True)
    last = ctx.last_sample_consensus()
    assert rc == 0 and st["iterations"] == len(trace) == 5 and st["state"] == "ITERATIONS"
    tgt = pair["tgt"][:, :3].astype(np.float64)
    ctx.transform_f32(CUR, S, np.eye(4, dtype=np.float32))                 # the current source
    fin = np.eye(4, dtype=np.float32)
    for k, it in enumerate(trace):
        found = ctx.correspondences(CUR, T_, 4.0, reciprocal=True)
        q, m, d, stages = ctx.correspondences_rejected(CUR, T_, 4.0, chain, reciprocal=True)
        assert it["n_found"] == len(found[0]) and it["n_corr"] == len(q) >= 3
        assert [(s["n_in"], s["n_out"], float(s["threshold"])) for s in it["stages"]] == [(s["n_in"], s["n_out"], float(s["threshold"])) for s in stages], k
        assert all(s["n_out"] < s["n_in"] for s in stages), (k, stages)
        mse = d.astype(np.float64).sum() / len(d)
        assert abs(it["mse"] - mse) <= 1e-12 * mse
        cur = ctx.download(CUR)[:, :3].astype(np.float64)
        ok, dr, dt = R.close_to(it["tr"], kabsch(cur[q], tgt[m]))
        assert ok, (k, dr, dt)
        fin = mvr.mat4f_mul(it["tr"], fin)
        if k == len(trace) - 1:
            same_result(ctx.last_sample_consensus(), last, "the last iteration's stage")
            assert last["live"] == it["n_found"] and last["inliers"] == stages[0]["n_out"]
        ctx.transform_f32(CUR, CUR, it["tr"])
    assert np.array_equal(bits(T), bits(fin)) and st["n_corr"] == trace[-1]["n_corr"]
    ctx.transform_f32(CUR, S, T)
    assert np.array_equal(bits(ctx.download(OUT)), bits(ctx.download(CUR)))
    assert np.array_equal(bits(ctx.download(S)), bits(pair["src"]))


NO_CAP = 1e3          # a search distance beyond the object's extent: PCL's ICP has no cap by default, the rejector is the outlier handling


def test_pose_under_gross_outliers(mvr, ctx):
    """A fifth of the target -- the points whose normals lie closest to the z axis -- is replaced by a copy of itself shifted by
    10 mm along z, and the search has no distance cap, as a PCL ICP that relies on its rejector has none.  Two views of a
    sampled surface have no exact pose: which pairs an align keeps decides it at the level of the sampling, far above the parity
    bars.  So the pose "without gross outliers" is the one the same call reaches on the target without those points, and the
    bars say that the wrong group must not change a single decision of the stage.  That is what the rules promise: on the CPU
    (brute force at the prior's pose) 714 source points lie nearer to the copy than to any remaining target point, every one of
    them at least 7.1 mm from it; a source point with a remaining target point within that distance has the same match in both
    runs.  So the two lists differ only in pairs that are wrong by millimetres either way; such a pair is no inlier of a motion
    that wins the loop, the count of every winning attempt is the same, the loop stops at the same attempt, and the refits sum
    over the same pairs."""
    pair = RC._synth_pair(mvr, 6001, 5000, normals=True)
    tgt = pair["tgt"]
    block = np.argsort(-np.abs(pair["tnrm"][:, 2]), kind="stable")[:len(tgt) // 5]
    keep = np.setdiff1d(np.arange(len(tgt)), block)
    shifted = tgt[block].copy()
    shifted[:, 2] += np.float32(10.0)
    with_copy = np.ascontiguousarray(np.concatenate([tgt[keep], shifted]))
    chain = [sac(mvr, 1.5, refine=True, max_iterations=500)]
    p = mvr.icp_params(reciprocal=False, max_dist=NO_CAP, max_iter=20, teps=0.0, feps=0.0)
    poses = []
    for t in (np.ascontiguousarray(tgt[keep]), with_copy):
        ctx.upload(S, pair["src"])
        ctx.upload(T_, t)
        T, st, rc, trace = ctx.icp_align_rejected(S, T_, -1, p, chain, return_trace=True)
        assert rc == 0, st
        poses.append((T, st, trace))
    plain, _, _ = ctx.icp_align(S, T_, -1, p)
    # what the first iteration met: the copy is matched, and none of its pairs is kept
    q0, m0, d0 = ctx.correspondences(S, T_, NO_CAP, reciprocal=False)
    q1, m1, _, _ = ctx.correspondences_rejected(S, T_, NO_CAP, chain, reciprocal=False)
    to_copy, kept_copy = int((m0 >= len(keep)).sum()), int((m1 >= len(keep)).sum())
    nearest = float(np.sqrt(d0[m0 >= len(keep)].min()))
    (Ta, sa, ta), (Tb, sb, tb) = poses
    dr, dt = np.abs(Ta[:3, :3] - Tb[:3, :3]).max(), np.abs(Ta[:3, 3] - Tb[:3, 3]).max()
    pr, pt = np.abs(Ta[:3, :3] - plain[:3, :3]).max(), np.abs(Ta[:3, 3] - plain[:3, 3]).max()
    print("gross outliers: %d of %d pairs go to the copy (the nearest at %.2f mm), %d kept; with the stage the pose moves by %.3g (rotation) / %.3g "
          "(translation), survivors per iteration %s -> %s; plain icp_align moves by %.3g / %.3g"
          % (to_copy, len(q0), nearest, kept_copy, dr, dt, [t["n_corr"] for t in ta][-6:], [t["n_corr"] for t in tb][-6:], pr, pt))
    assert len(q0) == len(pair["src"]) and to_copy > 100 and nearest > 1.5 and kept_copy == 0
    assert 100 < sb["n_corr"] < len(q0) - to_copy
    assert dr <= R.ROT_TOL and dt <= R.TRANS_TOL, (dr, dt)
    assert pr > 100 * R.ROT_TOL or pt > 100 * R.TRANS_TOL                      # (the same target moves a plain align)


def test_gicp_accepts_the_stage(mvr, ctx, synth_normals):
    load(ctx, synth_normals)
    p = mvr.gicp_params(max_corr_dist=4.0, max_iterations=3, use_reciprocal=1)
    chain = [sac(mvr, refine=True), mvr.rejector("one_to_one")]
    T, st, rc, trace = ctx.icp_align_gicp(S, T_, -1, p, chain, return_trace=True)
    assert rc == 0 and len(trace) >= 1 and np.isfinite(T).all()
    for it in trace:
        a, b = it["stages"]
        assert a["n_in"] == it["n_found"] and 3 <= a["n_out"] < a["n_in"] and b["n_in"] == a["n_out"] and b["n_out"] == it["n_corr"]
    last = ctx.last_sample_consensus()
    assert last["found"] and (last["live"], last["inliers"]) == (trace[-1]["stages"][0]["n_in"], trace[-1]["stages"][0]["n_out"])
    again = ctx.icp_align_gicp(S, T_, -1, p, chain, return_trace=True)
    assert np.array_equal(bits(T), bits(again[0]))


def test_refusals(mvr, ctx, cases):
    case = cases["planted_65"]
    load(ctx, case)
    q, m, d = case["q"], case["m"], case["d"]
    ok = rej_of(mvr, case)

    def refused(f, *a, **kw):
        with pytest.raises(mvr.MvrError) as e:
            f(*a, **kw)
        assert e.value.status == mvr.E_ARG, e.value

    with mvr.Context(0) as fresh:
        refused(fresh.last_sample_consensus)
    n = len(q)
    # R8
    for bad in (dict(q=np.where(np.arange(n) == 3, q[4], q)), dict(q=np.where(np.arange(n) == 0, 65, q)), dict(q=np.where(np.arange(n) == 0, -1, q)),
                dict(m=np.where(np.arange(n) == 5, 65, m)), dict(m=np.where(np.arange(n) == 5, -1, m)),
                dict(d=np.where(np.arange(n) == 7, np.float32(np.nan), d)), dict(d=np.where(np.arange(n) == 7, np.float32(-1.0), d))):
        refused(ctx.reject_sample_consensus, S, T_, bad.get("q", q), bad.get("m", m), bad.get("d", d), ok)
    # C12, and R10's
    for r in (mvr.rejector("sample_consensus", 0.0), mvr.rejector("sample_consensus", -0.05), mvr.rejector("sample_consensus", np.nan),
              mvr.rejector("sample_consensus", np.inf), mvr.rejector("sample_consensus", 0.05, max_iterations=(1 << 24) + 1)):
        refused(ctx.reject_sample_consensus, S, T_, q, m, d, r)
        refused(ctx.correspondences_rejected, S, T_, 30.0, [r])
        refused(ctx.reject_correspondences, S, T_, q, m, d, [mvr.rejector("median", 2.0), r])
        refused(ctx.icp_align_rejected, S, T_, OUT, mvr.icp_params(), [r])
        refused(ctx.icp_align_gicp, S, T_, OUT, mvr.gicp_params(), [r])
    refused(ctx.reject_sample_consensus, S, T_, q, m, d, mvr.rejector("median", 2.0))
    refused(ctx.reject_sample_consensus, mvr.MAX_SLOTS, T_, q, m, d, ok)
    refused(ctx.reject_sample_consensus, S, -1, q, m, d, ok)
    assert np.array_equal(bits(ctx.download(S)), bits(case["src"])) and np.array_equal(bits(ctx.download(T_)), bits(case["tgt"]))
    # the largest max_iterations is accepted; empty clouds and lists are no error
    got = ctx.reject_sample_consensus(S, T_, q, m, d, mvr.rejector("sample_consensus", 0.05, max_iterations=1 << 24, seed=1))
    assert got[3]["found"]
    e = np.zeros(0, np.int32)
    got = ctx.reject_sample_consensus(S, T_, e, e, np.zeros(0, np.float32), ok, return_trace=True)
    assert len(got[0]) == 0 and not got[3]["found"] and got[3]["attempts"] == 0 and np.array_equal(got[3]["T"], np.eye(4, dtype=np.float32))
    ctx.clear(CUR)
    got = ctx.reject_sample_consensus(CUR, T_, e, e, np.zeros(0, np.float32), ok)
    assert len(got[0]) == 0 and not got[3]["found"]
    got = ctx.correspondences_rejected(CUR, T_, 30.0, [ok])
    assert len(got[0]) == 0 and got[3][0]["n_in"] == got[3][0]["n_out"] == 0
