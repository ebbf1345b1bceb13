"""GPU test of the C++ layers of the sample-consensus alignment through tests/cxx/align_driver.cpp (compiled here, as
tests/test_gpu_fpfh_cxx.py compiles its driver): pcl::SampleConsensusPrerejective after pcl::NormalEstimation and
pcl::FPFHEstimation, and ScanCloud::alignPrerejective after ScanCloud::estimateNormals, return the pose of the Python path
(Context.align_prerejective) on the recovery case of tests/test_gpu_align.py, bit for bit."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import align_cases as AC
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def clouds(mvr):
    """the two downsampled clouds of the recovery case and what the Python path returns for them"""
    s_raw, t_raw = AC.recovery_view(mvr)
    out = []
    with mvr.Context(0) as ctx:
        for slot, raw in ((0, s_raw), (1, t_raw)):
            ctx.upload(slot, raw)
            ctx.voxel_grid(slot, slot, AC.REC_LEAF)
            ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS)
            out.append((ctx.download(slot), ctx.fpfh(slot, AC.REC_FPFH_RADIUS)))
        res = ctx.align_prerejective(0, 1, out[0][1], out[1][1], **AC.REC_PARAMS)
        ctx.transform_f32(2, 0, res["T"])
        moved = ctx.download(2)
        _, d2 = ctx.nn(2, 1)
    return out[0][0], out[1][0], res, moved, int((d2.astype(np.float64) < AC.REC_MAX_DIST ** 2).sum())


@pytest.fixture(scope="module")
def driven(built, clouds, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("align_cxx")
    exe = str(tmp / "align_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "align_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    files = []
    for name, p in (("source", clouds[0]), ("target", clouds[1])):
        files.append(str(tmp / (name + ".f32")))
        np.ascontiguousarray(p, np.float32).tofile(files[-1])
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    a = AC.REC_PARAMS
    args = [repr(AC.REC_NORMAL_RADIUS), repr(AC.REC_FPFH_RADIUS), str(a["max_iterations"]), str(a["nr_samples"]), str(a["k"]), repr(a["similarity"]),
            repr(a["max_dist"]), repr(a["inlier_fraction"]), str(a["seed"])]
    r = subprocess.run([exe] + files + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


def cm_bits(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(16).view(np.uint32)


def test_sample_consensus_prerejective_shim(driven, clouds):
    out, err = driven
    s, t, res, moved, inliers = clouds
    assert res["converged"] and out["shim_converged"] == 1
    assert np.array_equal(np.asarray(out["shim_T"], np.uint32), cm_bits(res["T"]))
    assert out["shim_result_inliers"] == res["inliers"] == out["shim_inliers"] == inliers
    assert out["shim_fitness_bits"] == int(np.float64(res["error"]).view(np.uint64))
    assert out["shim_aligned"] == len(s) and np.array_equal(np.asarray(out["shim_first"], np.uint32), moved[0, :3].view(np.uint32))
    assert out["guess_best"] == -1 and np.array_equal(np.asarray(out["guess_T"], np.uint32), cm_bits(res["T"]))
    assert out["refused"] == [0, 0] and "features must be set" in err


def test_scan_cloud_align_prerejective(driven, clouds):
    out, err = driven
    res = clouds[2]
    assert out["scan_ok"] == 1 and out["scan_refused"] == 0 and out["scan_best"] == res["best_iteration"] and out["scan_inliers"] == res["inliers"]
    assert np.array_equal(np.asarray(out["scan_T"], np.uint32), cm_bits(res["T"]))
    assert np.array_equal(np.asarray(out["scan_pose"], np.uint32), cm_bits(res["T"]))      # through the scene's row-vector type and back
    assert "[ScanCloud::computeFPFH] The cloud has no normals" in err
