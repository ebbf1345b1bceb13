"""GPU test of the C++ layer of Generalized ICP through tests/cxx/gicp_driver.cpp (compiled here, as tests/test_gpu_reject_cxx.py
compiles its driver), on the 6 001-point turntable pair of tests/gicp_cases.py:
  * pcl::GeneralizedIterativeClosestPoint on PointXYZ clouds estimates the 20-NN normals inside and returns what
    Context.icp_align_gicp returns on slots whose normals Context.estimate_normals made, within the parity bars; PCL's defaults;
    align(out, guess) starts from the source under the guess; a rejector and reciprocal correspondences reach the call;
  * on PointNormal clouds it uses the clouds' own normals, and the output carries the points and normals of the output slot;
  * ScanCloud::alignGICP returns the same pose."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import gicp_cases as GC
import reject_cases as RC
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_parity.py:17
MAX_DIST = 4.0


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def guess_matrix(mvr):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = GC.small_motion(np.random.default_rng(60), angle=0.004, shift=0.0)[:3, :3].astype(np.float32)
    T[:3, 3] = (0.2, -0.1, 0.15)
    return T


@pytest.fixture(scope="module")
def direct(mvr):
    case = RC._synth_pair(mvr, 6001, 6001, normals=True, config=1)
    out = dict(case=case, guess=guess_matrix(mvr))
    p = mvr.gicp_params(max_corr_dist=MAX_DIST)
    with mvr.Context(0) as ctx:
        ctx.upload(0, case["src"])
        ctx.upload(1, case["tgt"])
        ctx.estimate_normals([0, 1], k=20)
        out["xyz"] = ctx.icp_align_gicp(0, 1, 2, p)
        out["xyz_out"] = ctx.download(2)
        out["fitness"] = ctx.fitness(0, 1, out["xyz"][0])
        out["chain"] = ctx.icp_align_gicp(0, 1, 2, mvr.gicp_params(max_corr_dist=MAX_DIST, use_reciprocal=1), [mvr.rejector("median", 2.0)],
                                          return_trace=True)
        ctx.transform_f32(3, 0, out["guess"])
        out["guess_T"] = mvr.mat4f_mul(ctx.icp_align_gicp(3, 1, 2, p)[0], out["guess"])
        ctx.upload_normals(0, case["snrm"])
        ctx.upload_normals(1, case["tnrm"])
        out["normal"] = ctx.icp_align_gicp(0, 1, 2, mvr.gicp_params(max_corr_dist=MAX_DIST, gicp_epsilon=0.01))
        out["normal_out"] = (ctx.download(2), ctx.download_normals(2))
    return out


@pytest.fixture(scope="module")
def driven(built, direct, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("gicp_cxx")
    exe = str(tmp / "gicp_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "gicp_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    case, files = direct["case"], []
    for key in ("src", "tgt", "snrm", "tnrm"):
        files.append(str(tmp / (key + ".f32")))
        np.ascontiguousarray(case[key], np.float32).tofile(files[-1])
    files.append(str(tmp / "guess.f32"))
    np.ascontiguousarray(direct["guess"].T).reshape(16).tofile(files[-1])
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe] + files + [repr(MAX_DIST)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


def from_words(words):
    return np.asarray(words, np.uint32).view(np.float32).reshape(4, 4).T.astype(np.float64)


def within_bars(A, B, what):
    dr, dt = np.abs(A[:3, :3] - B[:3, :3]).max(), np.abs(A[:3, 3] - B[:3, 3]).max()
    print("%s: rotation within %.2g, translation within %.2g" % (what, dr, dt))
    assert dr <= ROT_TOL and dt <= TRANS_TOL, (what, dr, dt)


def test_point_xyz_clouds_get_their_normals_inside(driven, direct):
    out, _ = driven
    T, st, rc = direct["xyz"]
    assert rc == 0 and st["state"] == "TRANSFORM" and out["defaults"] == [200, 20, 20, 1, 1, 1, 1, 0]
    within_bars(from_words(out["xyz_T"]), T.astype(np.float64), "PointXYZ")
    assert out["xyz_api"] == [1, st["iterations"], st["n_corr"], len(direct["case"]["src"]), 2]
    pts = direct["xyz_out"]
    got = np.asarray(out["xyz_out"], np.uint32).view(np.float32).reshape(-1, 2)
    assert np.abs(got - pts[::97][:, [0, 2]]).max() <= 1e-3
    assert abs(float(np.asarray(out["xyz_fitness"], np.uint32).view(np.float32)[0]) - direct["fitness"]) <= 1e-4 * direct["fitness"]
    within_bars(from_words(out["guess_T"]), direct["guess_T"].astype(np.float64), "guess")
    assert np.abs(direct["guess_T"] - T).max() < 0.05                     # ... and it ends where the align without a guess ends
    Tc, sc, rcc, trace = direct["chain"]
    assert rcc == 0 and all(s["n_out"] < s["n_in"] for t in trace for s in t["stages"])
    within_bars(from_words(out["chain_T"]), Tc.astype(np.float64), "median rejector, reciprocal")
    assert out["chain_median"][0] == bits([trace[-1]["stages"][0]["threshold"]])[0] != 0


def test_point_normal_clouds_use_their_normals(driven, direct):
    out, _ = driven
    T, st, rc = direct["normal"]
    assert rc == 0
    within_bars(from_words(out["normal_T"]), T.astype(np.float64), "PointNormal")
    assert not np.array_equal(bits(T), bits(direct["xyz"][0]))
    pts, nrm = direct["normal_out"]
    got = np.asarray(out["normal_out"], np.uint32).view(np.float32).reshape(-1, 3)
    assert np.abs(got[:, 0] - pts[::97, 0]).max() <= 1e-3 and np.abs(got[:, 1:] - nrm[::97][:, [0, 2]]).max() <= 1e-5


def test_scan_cloud_align_gicp(driven, direct):
    out, _ = driven
    T, st, rc = direct["xyz"]
    assert out["scan_ok"] == [1, st["iterations"]]
    pose = np.asarray(out["scan_pose"], np.float64).reshape(4, 4).T        # RowMatrixd: the row-vector convention
    within_bars(pose, T.astype(np.float64), "ScanCloud::alignGICP")
