"""GPU test of the C++ layer of the sample-consensus rejector through tests/cxx/reject_sac_driver.cpp (compiled here, as
tests/test_gpu_reject_cxx.py compiles its driver), on the 6 001-point pair of tests/reject_cases.py:
  * pcl::registration::CorrespondenceRejectorSampleConsensus on its own list returns the survivors, the motion and the record of
    Context.reject_sample_consensus bit for bit, under PCL's names and the older ones; getInliersIndices gives the survivors'
    positions in the list; without clouds it prints an error and returns nothing;
  * added to a pcl::IterativeClosestPoint it is a stage of the chain: the final transformation is Context.icp_align_rejected's,
    and getBestTransformation afterwards is what Context.last_sample_consensus returns."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import reject_cases as RC
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

MAX_DIST, MAX_ITERATIONS, THRESHOLD, SAC_ITERATIONS, SEED = 4.0, 4, 1.5, 200, 2 ** 33 + 5
DBL_MAX = sys.float_info.max
KEYS = ("found", "live", "valid", "inliers", "ransac_inliers", "iterations", "attempts", "best_attempt", "refine_rounds")


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def direct(mvr):
    case = RC.build(mvr)["synth_6001"]
    out = dict(case=case)
    with mvr.Context(0) as ctx:
        ctx.upload(0, case["src"])
        ctx.upload(1, case["tgt"])
        out["list"] = ctx.correspondences(0, 1, MAX_DIST, reciprocal=False)
        sac = mvr.rejector("sample_consensus", THRESHOLD, max_iterations=SAC_ITERATIONS, refine=True, seed=SEED)
        out["own"] = ctx.reject_sample_consensus(0, 1, *out["list"], sac)
        out["old"] = ctx.reject_sample_consensus(0, 1, *out["list"], mvr.rejector("sample_consensus", THRESHOLD, max_iterations=SAC_ITERATIONS, seed=SEED))
        p = mvr.icp_params(reciprocal=True, max_dist=MAX_DIST, max_iter=MAX_ITERATIONS, teps=0.0, feps=-DBL_MAX)       # the shim's (PCL's) defaults
        out["icp"] = ctx.icp_align_rejected(0, 1, 2, p, [sac, mvr.rejector("median", 2.0)], return_trace=True)
        out["last"] = ctx.last_sample_consensus()
    return out


@pytest.fixture(scope="module")
def driven(built, direct, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("reject_sac_cxx")
    exe = str(tmp / "reject_sac_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "reject_sac_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    case, files = direct["case"], []
    for key in ("src", "tgt"):
        files.append(str(tmp / (key + ".f32")))
        np.ascontiguousarray(case[key], np.float32).tofile(files[-1])
    q, m, d = direct["list"]
    files.append(str(tmp / "list.u32"))
    np.stack([q.astype(np.uint32), m.astype(np.uint32), bits(d)], 1).tofile(files[-1])
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe] + files + [repr(MAX_DIST), str(MAX_ITERATIONS), repr(THRESHOLD), str(SAC_ITERATIONS), str(SEED)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


def cm_bits(T):
    return bits(np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(16))


def record(res):
    return [int(res[k]) & 0xFFFFFFFF for k in KEYS]


def triples(lists):
    q, m, d = lists[:3]
    return np.stack([q.astype(np.uint32), m.astype(np.uint32), bits(d)], 1)


def test_the_rejector_on_its_own_list(driven, direct):
    out, err = driven
    q, m, d, res = direct["own"]
    assert res["found"] and 3 <= len(q) < len(direct["list"][0]) and res["refine_rounds"] >= 1
    assert np.array_equal(np.asarray(out["own_kept"], np.uint32).reshape(-1, 3), triples(direct["own"]))
    assert np.array_equal(np.asarray(out["own_T"], np.uint32), cm_bits(res["T"])) and out["own_result"] == record(res)
    # the list is in ascending query index, so the survivors' positions are where their queries stand in it
    assert np.array_equal(direct["list"][0][np.asarray(out["own_inliers"], np.int64)], q)
    q0, _, _, res0 = direct["old"]
    assert np.array_equal(np.asarray(out["old_kept"], np.uint32).reshape(-1, 3), triples(direct["old"]))
    assert np.array_equal(np.asarray(out["old_T"], np.uint32), cm_bits(res0["T"])) and res0["refine_rounds"] == 0
    assert out["own_api"] == [1] * 7 and out["name"] == "CorrespondenceRejectorSampleConsensus"
    assert "[pcl::registration::CorrespondenceRejectorSampleConsensus::getRemainingCorrespondences] No input cloud dataset was given!" in err


def test_the_rejector_inside_an_icp(driven, direct):
    out, _ = driven
    T, st, rc, trace = direct["icp"]
    assert rc == 0 and st["iterations"] == MAX_ITERATIONS
    assert np.array_equal(np.asarray(out["icp_T"], np.uint32), cm_bits(T))
    last = direct["last"]
    assert np.array_equal(np.asarray(out["icp_best"], np.uint32), cm_bits(last["T"])) and out["icp_result"] == record(last)
    assert (last["live"], last["inliers"]) == (trace[-1]["stages"][0]["n_in"], trace[-1]["stages"][0]["n_out"])
    assert all(t["stages"][0]["n_out"] < t["stages"][0]["n_in"] for t in trace)                              # the stage did reject
    converged, iterations, n_corr, n_out, median = out["icp_api"]
    assert (converged, iterations, n_corr, n_out) == (int(st["converged"]), st["iterations"], st["n_corr"], len(direct["case"]["src"]))
    assert median == bits([trace[-1]["stages"][1]["threshold"]])[0] != 0
