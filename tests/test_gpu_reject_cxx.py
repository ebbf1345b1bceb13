"""GPU test of the C++ layer of the correspondence rejectors through tests/cxx/reject_driver.cpp (compiled here, as
tests/test_gpu_sac_cxx.py compiles its driver), on the 6 001-point pair with normals of tests/reject_cases.py:
  * pcl::IterativeClosestPoint with two rejectors added (a third added and removed again) returns the final transformation of
    the C-ABI call (Context.icp_align_rejected) bit for bit, tells its median rejector the median of the last iteration, and
    with the chain cleared returns what Context.icp_align returns;
  * with PointNormal clouds the surface-normal rejector reads the normals the ICP uploaded, and the output carries the points
    and normals of the library's output slot;
  * CorrespondenceRejectorMedianDistance::getCorrespondences and CorrespondenceRejectorSurfaceNormal::getRemainingCorrespondences
    on a list return what Context.reject_correspondences returns; getMedianDistance is set; a negative factor prints an error
    and returns nothing."""
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

MAX_DIST, MAX_ITERATIONS = 4.0, 4
DBL_MAX = sys.float_info.max


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def direct(mvr):
    case = RC.build(mvr)["synth_normals_6001"]
    out = dict(case=case)
    with mvr.Context(0) as ctx:
        ctx.upload(0, case["src"])
        ctx.upload(1, case["tgt"])
        p = mvr.icp_params(reciprocal=True, max_dist=MAX_DIST, max_iter=MAX_ITERATIONS, teps=0.0, feps=-DBL_MAX)       # the shim's (PCL's) defaults
        chain = [mvr.rejector("median", 2.0), mvr.rejector("trimmed", float(np.float32(0.8)), 10)]
        out["icp"] = ctx.icp_align_rejected(0, 1, 2, p, chain, return_trace=True)
        out["plain"] = ctx.icp_align(0, 1, 2, p)
        out["list"] = ctx.correspondences(0, 1, MAX_DIST, reciprocal=False)
        out["median"] = ctx.reject_correspondences(0, 1, *out["list"], [mvr.rejector("median", 1.25)])
        ctx.upload_normals(0, case["snrm"])
        ctx.upload_normals(1, case["tnrm"])
        p = mvr.icp_params(reciprocal=False, max_dist=MAX_DIST, max_iter=MAX_ITERATIONS, teps=0.0, feps=-DBL_MAX)
        chain = [mvr.rejector("one_to_one"), mvr.rejector("surface_normal", 0.9995)]
        out["normal"] = ctx.icp_align_rejected(0, 1, 2, p, chain)
        out["normal_out"] = (ctx.download(2), ctx.download_normals(2))
        out["normal_kept"] = ctx.reject_correspondences(0, 1, *out["list"], [mvr.rejector("surface_normal", 0.9995)])
    return out


@pytest.fixture(scope="module")
def driven(built, direct, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("reject_cxx")
    exe = str(tmp / "reject_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "reject_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    case, files = direct["case"], []
    for key in ("src", "tgt", "snrm", "tnrm"):
        files.append(str(tmp / (key + ".f32")))
        np.ascontiguousarray(case[key], np.float32).tofile(files[-1])
    q, m, d = direct["list"]
    files.append(str(tmp / "list.u32"))
    np.stack([q.astype(np.uint32), m.astype(np.uint32), bits(d)], 1).tofile(files[-1])
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe] + files + [repr(MAX_DIST), str(MAX_ITERATIONS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


def cm_bits(T):
    return bits(np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(16))


def test_icp_with_rejectors_equals_the_c_abi_call(driven, direct):
    out, _ = driven
    T, st, rc, trace = direct["icp"]
    assert rc == 0 and st["iterations"] == MAX_ITERATIONS
    assert np.array_equal(np.asarray(out["icp_T"], np.uint32), cm_bits(T))
    removed, not_removed, left, second_is_trimmed, getters, converged, iterations, n_corr, n_out = out["icp_api"]
    assert (removed, not_removed, left, second_is_trimmed, getters) == (1, 0, 2, 1, 1)
    assert (converged, iterations, n_corr, n_out) == (int(st["converged"]), st["iterations"], st["n_corr"], len(direct["case"]["src"]))
    assert all(s["n_out"] < s["n_in"] for t in trace for s in t["stages"])                                   # the chain did reject
    assert out["icp_median"][0] == bits([trace[-1]["stages"][0]["threshold"]])[0] != 0                        # getMedianDistance is set
    assert out["names"] == ["CorrespondenceRejectorMedianDistance", "CorrespondenceRejectorTrimmed", "CorrespondenceRejectorDistance"]
    assert out["cleared"] == [0] and np.array_equal(np.asarray(out["plain_T"], np.uint32), cm_bits(direct["plain"][0]))
    assert not np.array_equal(cm_bits(T), cm_bits(direct["plain"][0]))


def test_icp_on_clouds_with_normals(driven, direct):
    out, _ = driven
    T, st, rc = direct["normal"]
    assert rc == 0 and np.array_equal(np.asarray(out["normal_T"], np.uint32), cm_bits(T))
    assert out["normal_api"] == [st["n_corr"], 1]
    pts, nrm = direct["normal_out"]
    exp = np.stack([bits(pts[::97, 0]), bits(nrm[::97, 0]), bits(nrm[::97, 2])], 1).reshape(-1)
    assert np.array_equal(np.asarray(out["normal_out"], np.uint32), exp)


def test_rejectors_on_their_own(driven, direct):
    out, err = driven
    q, m, d, stages = direct["median"]
    assert 3 <= len(q) < len(direct["list"][0])
    assert np.array_equal(np.asarray(out["median_kept"], np.uint32).reshape(-1, 3), np.stack([q.astype(np.uint32), m.astype(np.uint32), bits(d)], 1))
    assert out["median_distance"][0] == bits([stages[0]["threshold"]])[0] != 0
    q, m, d, _ = direct["normal_kept"]
    assert 3 <= len(q) < len(direct["list"][0])
    assert np.array_equal(np.asarray(out["normal_kept"], np.uint32).reshape(-1, 3), np.stack([q.astype(np.uint32), m.astype(np.uint32), bits(d)], 1))
    assert out["refused"] == [0] and "[pcl::registration::CorrespondenceRejectorMedianDistance::getRemainingCorrespondences]" in err
