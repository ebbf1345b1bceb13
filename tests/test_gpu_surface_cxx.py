"""GPU test of the C++ layers of the features over a search surface through tests/cxx/surface_driver.cpp (compiled here, as
tests/test_gpu_iss_cxx.py compiles its driver), on the two downsampled clouds of the recovery case of tests/test_gpu_align.py:
  * pcl::NormalEstimation with setSearchSurface / setIndices and ScanCloud::estimateNormalsFrom return the bits of
    Context.estimate_normals_at;
  * ScanCloud::computeFPFHAt / computePFHAt, by indices and over another cloud as surface, return the bits of Context.fpfh_at /
    pfh_at -- and, by indices, the rows of the whole-cloud calls (rule Q5);
  * ScanCloud::alignPrerejectivePFH with use_keypoints, which computes descriptors at the keypoints only (and alignPrerejective,
    which still computes every row), return pose, best_iteration and inliers of the four-argument overload fed with full tables, and the pose of the Python path on
    NaN-masked full tables."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import align_cases as AC
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32 = np.float32
ISS = dict(salient_radius=10.0, non_max_radius=6.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)      # those of tests/test_gpu_iss_cxx.py
PARAMS = dict(AC.REC_PARAMS, max_iterations=2000)      # (the two paths agree at any iteration count: a short run)
STEP, K_INDICES = 37, 12


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def direct(mvr):
    """the two clouds and what the Python path returns for them"""
    s_raw, t_raw = AC.recovery_view(mvr)
    out = {}
    with mvr.Context(0) as ctx:
        pts, key, fpfh, pfh = [], [], [], []
        for slot, raw in ((0, s_raw), (1, t_raw)):
            ctx.upload(slot, raw)
            ctx.voxel_grid(slot, slot, AC.REC_LEAF)
            ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS)
            pts.append(ctx.download(slot))
            fpfh.append(ctx.fpfh(slot, AC.REC_FPFH_RADIUS))
            pfh.append(ctx.pfh(slot, radius=AC.REC_FPFH_RADIUS))
            key.append(ctx.iss_keypoints(-1, slot, return_index=True, **ISS)[1])
        n = len(pts[0])
        idx = np.array([i for i in range(n - 1, -1, -1) if i % STEP == 0], np.uint32)
        idx = np.concatenate([idx, idx[:1]])
        out.update(s=pts[0], t=pts[1], idx=idx, fpfh=fpfh, pfh=pfh, key=key)
        out["fpfh_indices"] = ctx.fpfh_at(0, 0, AC.REC_FPFH_RADIUS, indices=idx)
        out["pfh_indices"] = ctx.pfh_at(0, 0, indices=idx, radius=AC.REC_FPFH_RADIUS)
        ctx.upload(2, pts[1])                                             # the target's points alone, over the source and its normals
        out["fpfh_surface"] = ctx.fpfh_at(2, 0, AC.REC_FPFH_RADIUS)
        out["pfh_surface"] = ctx.pfh_at(2, 0, radius=AC.REC_FPFH_RADIUS)
        out["ne_surface"] = np.c_[ctx.estimate_normals_at(2, 0, radius=AC.REC_NORMAL_RADIUS)]
        out["ne_indices"] = np.c_[ctx.estimate_normals_at(0, 0, indices=idx, k=K_INDICES)]
        for name, tables in (("fpfh", fpfh), ("pfh", pfh)):
            masked = []
            for f, k in zip(tables, key):
                m = np.full_like(f, np.nan)
                m[k] = f[k]
                masked.append(m)
            out[name + "_res"] = ctx.align_prerejective(0, 1, masked[0], masked[1], **PARAMS)
    return out


@pytest.fixture(scope="module")
def driven(built, direct, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("surface_cxx")
    exe = str(tmp / "surface_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "surface_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    files = []
    for name, p in (("source", direct["s"]), ("target", direct["t"])):
        files.append(str(tmp / (name + ".f32")))
        np.ascontiguousarray(p, F32).tofile(files[-1])
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    a = PARAMS
    args = [str(tmp), repr(ISS["salient_radius"]), repr(ISS["non_max_radius"]), repr(ISS["gamma_21"]), repr(ISS["gamma_32"]), str(ISS["min_neighbors"]),
            repr(AC.REC_NORMAL_RADIUS), repr(AC.REC_FPFH_RADIUS), str(a["max_iterations"]), str(a["nr_samples"]), str(a["k"]), repr(a["similarity"]),
            repr(a["max_dist"]), repr(a["inlier_fraction"]), str(a["seed"]), str(STEP)]
    r = subprocess.run([exe] + files + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    tables = {n: np.fromfile(str(tmp / (n + ".f32")), F32) for n in ("ne_surface", "ne_indices", "fpfh_indices", "pfh_indices", "fpfh_surface",
                                                                      "pfh_surface", "normals_from")}
    return json.loads(r.stdout), r.stderr, tables


def cm_bits(T):
    return np.ascontiguousarray(np.asarray(T, F32).T).reshape(16).view(np.uint32)


def test_normal_estimation_with_surface_and_indices(driven, direct):
    out, err, tab = driven
    assert out["ne_surface"] == len(direct["t"]) and out["ne_indices"] == len(direct["idx"]) and out["ne_refused"] == 0
    assert "lies outside the input cloud" in err
    assert np.array_equal(bits(tab["ne_surface"]), bits(direct["ne_surface"]).reshape(-1))
    assert np.array_equal(bits(tab["ne_indices"]), bits(direct["ne_indices"]).reshape(-1))
    assert out["normals_from"] == len(direct["t"]) and np.array_equal(bits(tab["normals_from"]), bits(direct["ne_surface"]).reshape(-1))
    assert np.isfinite(direct["ne_surface"]).all(1).any() and np.isnan(direct["ne_surface"]).any()      # (the clouds overlap in part)


def test_scan_cloud_descriptors_at(driven, direct):
    out, err, tab = driven
    idx = direct["idx"]
    assert out["at_ok"] == 1 and out["at_refused"] == [0, 0, 0] and out["at_rows"] == [len(idx), len(idx)]
    for text in ("[ScanCloud::computeFPFHAt] The cloud has no normals", "[ScanCloud::computePFHAt] The cloud has no normals",
                 "[ScanCloud::computeFPFHAt] The radius", "[ScanCloud::computePFHAt] The radius", "lies beyond the cloud"):
        assert text in err, text
    for name, full in (("fpfh", direct["fpfh"][0]), ("pfh", direct["pfh"][0])):
        assert np.array_equal(bits(tab[name + "_indices"]), bits(direct[name + "_indices"]).reshape(-1)), name
        assert np.array_equal(bits(tab[name + "_indices"]), bits(full[idx]).reshape(-1)), name                  # Q5
        assert np.array_equal(bits(tab[name + "_surface"]), bits(direct[name + "_surface"]).reshape(-1)), name
    assert out["surface_ok"] == 1 and out["surface_rows"] == [len(direct["t"])] * 2
    assert np.isfinite(direct["fpfh_surface"]).all(1).any()


def test_align_prerejective_computes_descriptors_at_the_keypoints(driven, direct):
    out, err, tab = driven
    for name in ("fpfh", "pfh"):
        res = direct[name + "_res"]
        assert out[name + "_same"] == 1, name
        assert out[name + "_ok"] == [int(res["converged"])] * 2, name
        assert np.array_equal(np.asarray(out[name + "_T"], np.uint32), cm_bits(res["T"])), name
        assert out[name + "_inliers"] == res["inliers"] and out[name + "_best"] == res["best_iteration"], name
    print("keypoints: %d of %d source and %d of %d target points; FPFH: iteration %d, %d inliers; PFH: converged %d, iteration %d, %d inliers"
          % (len(direct["key"][0]), len(direct["s"]), len(direct["key"][1]), len(direct["t"]), out["fpfh_best"], out["fpfh_inliers"],
             out["pfh_ok"][0], out["pfh_best"], out["pfh_inliers"]))
