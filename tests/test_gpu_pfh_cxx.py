"""GPU test of the C++ layers of the PFH descriptors through tests/cxx/pfh_driver.cpp (compiled here, as
tests/test_gpu_fpfh_cxx.py compiles its driver): pcl::PFHEstimation::compute after pcl::NormalEstimation in radius and in k
mode, pcl::SampleConsensusPrerejective on PFHSignature125 rows, ScanCloud::computePFH and ScanCloud::alignPrerejectivePFH give
the bits of the C-ABI calls (Context.pfh, Context.align_prerejective) on the same two scans."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

N, CONFIG, NORMAL_RADIUS, RADIUS, K = 4000, 3, 6.0, 8.0, 16
ITERATIONS, SEED, MAX_DIST = 2000, 7, 4.0
SIMILARITY, FRACTION = float(np.float32(0.8)), float(np.float32(0.25))      # the setters of PCL take floats


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def driven(built, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("pfh_cxx")
    exe = str(tmp / "pfh_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "pfh_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe, str(N), str(CONFIG), repr(NORMAL_RADIUS), repr(RADIUS), str(K), str(ITERATIONS), str(SEED), repr(MAX_DIST)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


@pytest.fixture(scope="module")
def direct(mvr):
    sp = mvr.synth_params(12, CONFIG)
    p, q = mvr.synth_view(sp, 0, N), mvr.synth_view(sp, 1, N)
    with mvr.Context(0) as ctx:
        ctx.upload(0, p); ctx.upload(1, q)
        ctx.estimate_normals([0, 1], radius=NORMAL_RADIUS)
        f, cnt = ctx.pfh(0, radius=RADIUS, return_neighbors=True)
        fk = ctx.pfh(0, k=K)
        g = ctx.pfh(1, radius=RADIUS)
        res = ctx.align_prerejective(0, 1, f, g, max_iterations=ITERATIONS, nr_samples=3, k=2, similarity=SIMILARITY, max_dist=MAX_DIST,
                                     inlier_fraction=FRACTION, seed=SEED)
    assert cnt.mean() > 15 and np.isfinite(f).all(1).mean() > 0.99
    return f, fk, res


def result_tuple(res):
    return [int(res["converged"]), res["best_iteration"], res["inliers"], res["rejected"], res["scored"]]


def test_pfh_estimation_compute(driven, direct):
    out, err = driven
    f, fk, res = direct
    assert out["shim_size"] == N and out["descriptor_size"] == 125
    assert np.array_equal(np.asarray(out["shim"], np.uint32).reshape(-1, 125), bits(f))
    assert np.array_equal(np.asarray(out["shim_k"], np.uint32).reshape(-1, 125), bits(fk))
    assert out["modes"] == [RADIUS, 0, 0.0, K]                            # setKSearch after setRadiusSearch: the k mode
    assert out["shim_dense"] == int(np.isfinite(f).all())
    assert out["throws"] == [1, 1]
    assert out["refused"] == [0, 0, 0, 0, 0]
    assert "No input dataset was given" in err and "differs from the number of points" in err and "(setKSearch)" in err


def test_sample_consensus_prerejective_on_pfh_rows(driven, direct):
    out, err = driven
    f, fk, res = direct
    assert out["align"] == result_tuple(res) and out["aligned_size"] == N
    assert out["align_error"] == res["error"]
    T = np.asarray(out["align_T"], np.uint32).view(np.float32).reshape(4, 4).T          # column-major in the result
    assert np.array_equal(bits(T), bits(res["T"]))
    assert (out["inlier_list"] > 0) == bool(res["converged"])
    print("PFH rows through pcl::SampleConsensusPrerejective: converged %d at iteration %d, %d inliers of %d, rejected %d, scored %d"
          % tuple(result_tuple(res)[:3] + [N] + result_tuple(res)[3:]))


def test_scan_cloud_compute_pfh_and_align(driven, direct):
    out, err = driven
    f, fk, res = direct
    assert out["scan_ok"] == 1 and out["scan_points"] == N
    assert np.array_equal(np.asarray(out["scan"], np.uint32).reshape(-1, 125), bits(f))
    assert out["scan_refused"] == [0, 0, 0, 0]
    assert "[ScanCloud::computePFH] The cloud has no normals" in err and "[ScanCloud::computePFH] The radius" in err
    assert out["scan_align"] == [int(res["converged"])] + result_tuple(res)
    T = np.asarray(out["scan_align_T"], np.uint32).view(np.float32).reshape(4, 4).T
    assert np.array_equal(bits(T), bits(res["T"]))
