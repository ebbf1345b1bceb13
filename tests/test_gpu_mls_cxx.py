"""GPU test of the C++ layers of the moving-least-squares smoothing through tests/cxx/mls_driver.cpp (compiled here, as
tests/test_grid_size_host.py compiles its driver): pcl::MovingLeastSquares::process, ScanCloud::smooth and the smoothing overload
of Registrator::saveRegisteredPoints, against the Python path (Context.mls) on the same scans and on the file tree the driver
wrote."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import pcd_py
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F32 = np.float32
V, N, CONFIG = 3, 20000, 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def driven(built, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("mls_cxx")
    exe = str(tmp / "mls_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "mls_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    for d in ("raw", "mls", "mls_vox", "bad"):
        os.makedirs(tmp / d)
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe, str(V), str(N), str(CONFIG), str(tmp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr, tmp


def xyz_of(rec):
    return np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(F32)


def test_moving_least_squares_process(driven, mvr):
    out, err, _ = driven
    p = mvr.synth_view(mvr.synth_params(V, CONFIG), 0, N)
    assert out["defaults"] == [2, 1] and out["gauss"] == 1.2 * 1.2
    with mvr.Context(0) as ctx:
        ctx.upload(0, p)
        n, idx, curv = ctx.mls(1, 0, 1.2, compute_normals=True, return_index=True, return_curvature=True)
        xyz, nrm = ctx.download(1), ctx.download_normals(1)
        assert 0 < n < N                                  # some points have fewer than 3 neighbours at this density
        assert np.array_equal(out["mls_idx"], idx)
        assert np.array_equal(np.asarray(out["mls_xyz"], np.uint32).reshape(-1, 3), bits(xyz[:, :3]))
        assert np.array_equal(np.asarray(out["mls_nrm"], np.uint32).reshape(-1, 3), bits(nrm[:, :3]))
        assert np.array_equal(np.asarray(out["mls_curv"], np.uint32), bits(curv))
        ctx.mls(1, 0, 1.2, order=1)
        assert np.array_equal(np.asarray(out["plane_inplace_xyz"], np.uint32).reshape(-1, 3), bits(ctx.download(1)[:, :3]))
    assert out["none"] == 0 and out["bad"] == 0
    assert "No input dataset given" in err and "must be finite and > 0" in err


def test_scan_cloud_smooth(driven, mvr):
    out, err, _ = driven
    p = mvr.synth_view(mvr.synth_params(V, CONFIG), 0, N)
    with mvr.Context(0) as ctx:
        ctx.upload(0, p)
        n, idx, curv = ctx.mls(1, 0, 1.2, compute_normals=True, return_index=True, return_curvature=True)
        xyz, nrm = ctx.download(1), ctx.download_normals(1)
    assert out["scan_rich_ok"] == 1 and out["scan_dropped"] == [N - n, N - n] and out["scan_bad"] == 0 and out["scan_after_bad"] == 1
    assert np.array_equal(out["scan_idx"], idx)           # the records' curvature held the original index
    assert np.array_equal(np.asarray(out["scan_xyz"], np.uint32).reshape(-1, 3), bits(xyz[:, :3]))
    assert np.array_equal(np.asarray(out["scan_nrm"], np.uint32).reshape(-1, 3), bits(nrm[:, :3]))
    assert np.array_equal(np.asarray(out["scan_curv"], np.uint32), bits(curv))
    assert "[ScanCloud::smooth]" in err


def test_save_registered_points_smoothed(driven, mvr):
    """the smoothed merged cloud on disk is Context.mls of the merged cloud the reference's overload wrote next to it; colours
    follow their points; the downsampled variant is Context.voxel_grid of the smoothed one"""
    out, err, tmp = driven
    assert out["merged_bad"] == 0 and os.listdir(os.path.join(tmp, "bad")) == [] and "[Registrator::saveRegisteredPoints]" in err
    _, raw = pcd_py.read_pcd(os.path.join(tmp, "raw", "points.pcd"))
    _, sm = pcd_py.read_pcd(os.path.join(tmp, "mls", "points.pcd"))
    _, vx = pcd_py.read_pcd(os.path.join(tmp, "mls_vox", "points.pcd"))
    assert out["merged"][0] == V * N == len(raw["x"]) and out["merged"][1] == len(sm["x"]) == out["merged_out"] and out["merged"][2] == len(vx["x"])
    p = np.ones((V * N, 4), F32)
    p[:, :3] = xyz_of(raw)
    with mvr.Context(0) as ctx:
        ctx.upload(0, p)
        n, idx = ctx.mls(1, 0, 2.0, order=2, return_index=True)
        got = ctx.download(1)
        m = ctx.voxel_grid(2, 1, 1.5)
        vox = ctx.download(2)
    assert 0 < n <= V * N and n == out["merged"][1]
    assert np.array_equal(bits(xyz_of(sm)), bits(got[:, :3])) and not np.array_equal(bits(got[:, :3]), bits(p[idx, :3]))
    assert np.array_equal(sm["rgb"].view(np.uint32), raw["rgb"].view(np.uint32)[idx])
    assert np.array_equal(bits(sm["normal_x"].astype(F32)), bits(raw["normal_x"].astype(F32)[idx]))
    assert m == out["merged"][2] < n and np.array_equal(bits(xyz_of(vx)), bits(vox[:, :3]))
    assert len(open(os.path.join(tmp, "mls", "points.asc")).read().strip().split("\n")) == n
