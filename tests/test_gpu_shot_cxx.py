"""GPU test of the C++ layers of the SHOT descriptors through tests/cxx/shot_driver.cpp (compiled here, as
tests/test_gpu_pfh_cxx.py compiles its driver): pcl::SHOTLocalReferenceFrameEstimation and pcl::SHOTEstimation (frames passed in,
an LRF radius of its own, setIndices, setSearchSurface), pcl::SampleConsensusPrerejective on SHOT352 rows, ScanCloud::computeSHOT,
computeSHOTAt and alignPrerejectiveSHOT (every point, and the keypoint route) give the bits of the C-ABI calls (Context.shot_lrf,
Context.shot, Context.shot_at, Context.align_prerejective) on the same two scans."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

N, CONFIG, NORMAL_RADIUS, RADIUS = 2000, 3, 6.0, 12.0
ITERATIONS, SEED, MAX_DIST = 2000, 7, 4.0
SIMILARITY, FRACTION = float(np.float32(0.8)), float(np.float32(0.25))      # the setters of PCL take floats
PICKS = np.array([5, 3, 3, N - 1, 0], np.uint32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def driven(built, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("shot_cxx")
    exe = str(tmp / "shot_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "shot_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe, str(N), str(CONFIG), repr(NORMAL_RADIUS), repr(RADIUS), str(ITERATIONS), str(SEED), repr(MAX_DIST)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


@pytest.fixture(scope="module")
def direct(mvr, driven):
    out, _ = driven
    sp = mvr.synth_params(12, CONFIG)
    p, q = mvr.synth_view(sp, 0, N), mvr.synth_view(sp, 1, N)
    a = dict(max_iterations=ITERATIONS, nr_samples=3, k=2, similarity=SIMILARITY, max_dist=MAX_DIST, inlier_fraction=FRACTION, seed=SEED)
    d = {}
    with mvr.Context(0) as ctx:
        ctx.upload(0, p); ctx.upload(1, q)
        ctx.estimate_normals([0, 1], radius=NORMAL_RADIUS)
        d["lrf"] = ctx.shot_lrf(0, RADIUS)
        d["f"], d["rf"], d["nb"] = ctx.shot(0, RADIUS, return_lrf=True, return_neighbors=True)
        d["rf_075"] = ctx.shot(0, RADIUS, lrf_radius=float(np.float32(0.75 * RADIUS)), return_lrf=True)[1]
        d["at"] = ctx.shot_at(0, 0, RADIUS, indices=PICKS)
        d["g"] = ctx.shot(1, RADIUS)
        d["res"] = ctx.align_prerejective(0, 1, d["f"], d["g"], **a)
        tabs = []
        for slot, key, f in ((0, out["keys_s"], d["f"]), (1, out["keys_t"], d["g"])):
            t = np.full_like(f, np.nan)
            t[key] = f[key]
            tabs.append(t)
        d["kres"] = ctx.align_prerejective(0, 1, tabs[0], tabs[1], **a)
    assert d["nb"].mean() > 15 and np.isfinite(d["f"]).all(1).mean() > 0.95
    return d


def result_tuple(res):
    return [int(res["converged"]), res["best_iteration"], res["inliers"], res["rejected"], res["scored"]]


def table(v, width):
    return np.asarray(v, np.uint32).reshape(-1, width)


def test_frames_and_rows_of_the_pcl_classes(driven, direct):
    out, err = driven
    d = direct
    assert out["shim_size"] == N and out["descriptor_size"] == 352
    assert np.array_equal(table(out["lrf"], 9), bits(d["lrf"]))
    assert np.array_equal(table(out["shim"], 352), bits(d["f"])) and np.array_equal(table(out["shim_rf"], 9), bits(d["rf"]))
    assert np.array_equal(table(out["shim_fed"], 352), bits(d["f"]))                  # setInputReferenceFrames with its own frames
    assert np.array_equal(table(out["shim_lrf_radius_rf"], 9), bits(d["rf_075"])) and not np.array_equal(bits(d["rf_075"]), bits(d["rf"]))
    assert np.array_equal(table(out["shim_indices"], 352), bits(d["at"])) and np.array_equal(bits(d["at"]), bits(d["f"][PICKS]))
    assert np.array_equal(table(out["shim_surface"], 352), bits(d["at"]))
    assert out["shim_dense"] == int(np.isfinite(d["f"]).all())
    assert out["refused"] == [0, 0, 0]
    assert "No input dataset was given" in err and "differs from the number of points" in err and "(setRadiusSearch)" in err


def test_sample_consensus_prerejective_on_shot352(driven, direct, mvr):
    out, _ = driven
    res = direct["res"]
    assert out["align"] == result_tuple(res) and out["aligned_size"] == N
    assert np.array_equal(np.asarray(out["align_T"], np.uint32), bits(mvr.to_cm(res["T"], np.float32)).reshape(-1))


def test_scan_cloud(driven, direct, mvr):
    out, err = driven
    d = direct
    assert out["scan_ok"] == [1, 1, 1] and out["scan_points"] == N
    assert out["scan_refused"] == [0, 0, 0, 0, 0]
    assert "has no normals" in err and "must be finite and > 0" in err and "lies beyond the cloud" in err
    assert np.array_equal(table(out["scan"], 352), bits(d["f"])) and np.array_equal(table(out["scan_rf"], 9), bits(d["rf"]))
    assert np.array_equal(table(out["scan_at"], 352), bits(d["at"])) and np.array_equal(table(out["scan_over"], 352), bits(d["at"]))
    for key, res in (("scan_align", d["res"]), ("key_align", d["kres"])):
        assert out[key][1:] == result_tuple(res) and out[key][0] == int(res["converged"])
        assert np.array_equal(np.asarray(out[key + "_T"], np.uint32), bits(mvr.to_cm(res["T"], np.float32)).reshape(-1))
    assert 0 < len(out["keys_s"]) < N and 0 < len(out["keys_t"]) < N
