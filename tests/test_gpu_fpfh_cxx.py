"""GPU test of the C++ layers of the FPFH descriptors through tests/cxx/fpfh_driver.cpp (compiled here, as
tests/test_gpu_mls_cxx.py compiles its driver): pcl::FPFHEstimation::compute after pcl::NormalEstimation, and
ScanCloud::computeFPFH after ScanCloud::estimateNormals, give the bits of the C-ABI call (Context.fpfh) on the same scan."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

N, CONFIG, NORMAL_RADIUS, RADIUS = 6000, 3, 5.0, 8.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def driven(built, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("fpfh_cxx")
    exe = str(tmp / "fpfh_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "fpfh_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe, str(N), str(CONFIG), repr(NORMAL_RADIUS), repr(RADIUS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


@pytest.fixture(scope="module")
def direct(mvr):
    p = mvr.synth_view(mvr.synth_params(12, CONFIG), 0, N)
    with mvr.Context(0) as ctx:
        ctx.upload(0, p)
        ctx.estimate_normals(0, radius=NORMAL_RADIUS)
        f, cnt = ctx.fpfh(0, RADIUS, return_counts=True)
    assert cnt.mean() > 15 and np.isfinite(f).all(1).mean() > 0.99
    return f


def test_fpfh_estimation_compute(driven, direct):
    out, err = driven
    assert out["shim_size"] == N and out["descriptor_size"] == 33
    assert np.array_equal(np.asarray(out["shim"], np.uint32).reshape(-1, 33), bits(direct))
    assert out["shim_dense"] == int(np.isfinite(direct).all())
    assert out["throws"] == [1, 1, 1]
    assert out["refused"] == [0, 0, 0, 0]
    assert "No input dataset was given" in err and "differs from the number of points" in err and "must be finite and > 0 (setRadiusSearch)" in err


def test_scan_cloud_compute_fpfh(driven, direct):
    out, err = driven
    assert out["scan_ok"] == 1 and out["scan_points"] == N
    assert np.array_equal(np.asarray(out["scan"], np.uint32).reshape(-1, 33), bits(direct))
    assert out["scan_refused"] == [0, 0, 0, 0]
    assert "[ScanCloud::computeFPFH] The cloud has no normals" in err and "[ScanCloud::computeFPFH] The radius" in err
