"""GPU test of the C++ layers of the boundary estimation and of the ISS keypoints with a border through
tests/cxx/boundary_driver.cpp (compiled here, as tests/test_gpu_iss_cxx.py compiles its driver), on a 6 000-point view with
the normals of the library's radius-mode estimation:
  * pcl::BoundaryEstimation::compute returns the flags of the C-ABI call (Context.boundary), at PCL's default threshold and
    at a set one; a non-zero setKSearch, missing normals and a missing radius print an error and compute nothing;
  * pcl::ISSKeypoint3D with setNormals + setBorderRadius, and with setNormalRadius + setBorderRadius, returns the indices and
    points of Context.iss_keypoints with border_radius on the same normals;
  * ScanCloud::detectBoundary and ScanCloud::detectKeypoints with border parameters return them too; a border radius of 0 is
    the detector without a border; a cloud without normals and a threshold outside the accepted range are refused."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import fpfh_cases as FC
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

N = 6000
RADIUS, NORMAL_RADIUS, BORDER_RADIUS = 8.0, 5.0, 7.0                   # 2.3 mm between neighbouring points
ISS = dict(salient_radius=8.0, non_max_radius=5.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)
ANGLE = 1.25                                                           # an exact f32: setAngleThreshold takes a float


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def direct(mvr):
    p = FC.view(mvr, N)
    with mvr.Context(0) as ctx:
        ctx.upload(0, p)
        ctx.estimate_normals(0, radius=NORMAL_RADIUS)
        nrm = ctx.download_normals(0)
        out = dict(p=p, nrm=nrm, flag=ctx.boundary(0, RADIUS), flag_angle=ctx.boundary(0, RADIUS, ANGLE))
        out["plain"] = ctx.iss_keypoints(-1, 0, return_index=True, **ISS)[1]
        out["key"] = ctx.iss_keypoints(1, 0, return_index=True, border_radius=BORDER_RADIUS, **ISS)[1]
        out["points"] = ctx.download(1)
        out["key_angle"] = ctx.iss_keypoints(-1, 0, return_index=True, border_radius=BORDER_RADIUS, angle_threshold=ANGLE, **ISS)[1]
    return out


@pytest.fixture(scope="module")
def driven(built, direct, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("boundary_cxx")
    exe = str(tmp / "boundary_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "boundary_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    files = []
    for name, a in (("cloud", direct["p"]), ("normals", direct["nrm"])):
        files.append(str(tmp / (name + ".f32")))
        np.ascontiguousarray(a, np.float32).tofile(files[-1])
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    args = [repr(RADIUS), repr(ISS["salient_radius"]), repr(ISS["non_max_radius"]), str(ISS["min_neighbors"]), repr(BORDER_RADIUS), repr(NORMAL_RADIUS), repr(ANGLE)]
    r = subprocess.run([exe] + files + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


def test_the_case_has_a_border(direct):
    n = len(direct["p"])
    assert 50 < direct["flag"].sum() < n // 4 and direct["flag_angle"].sum() > direct["flag"].sum()      # a lower threshold: more boundary points
    lost = np.setdiff1d(direct["plain"], direct["key"])
    print("%d points, %d boundary points; %d keypoints without a border, %d with (%d lost), %d at threshold %.2f"
          % (n, direct["flag"].sum(), len(direct["plain"]), len(direct["key"]), len(lost), len(direct["key_angle"]), ANGLE))
    assert len(direct["key"]) > 30 and len(lost) > 10 and not np.array_equal(direct["key"], direct["key_angle"])


def test_boundary_estimation_shim(driven, direct):
    out, err = driven
    assert out["default_angle"] == int(np.float32(np.pi / 2).view(np.uint32))
    assert np.array_equal(np.asarray(out["be_default"], bool), direct["flag"]) and set(out["be_default"]) == {0, 1}
    assert np.array_equal(np.asarray(out["be_angle"], bool), direct["flag_angle"])
    assert out["be_refused"] == [0, 0, 0]
    assert err.count("[pcl::BoundaryEstimation::compute] The k-neighbour mode (setKSearch 10) is not offered") == 1
    assert "dataset containing the normals" in err and "[pcl::BoundaryEstimation::compute] The search radius" in err


def test_iss_keypoint3d_with_a_border(driven, direct):
    out, err = driven
    key = direct["key"]
    assert np.array_equal(np.asarray(out["iss_normals_index"], np.uint32), key)
    assert np.array_equal(np.asarray(out["iss_normals_points"], np.uint32).reshape(-1, 3), np.ascontiguousarray(direct["points"][:, :3]).view(np.uint32))
    assert np.array_equal(np.asarray(out["iss_angle_index"], np.uint32), direct["key_angle"])
    # the normals of setNormalRadius are those of mvr_cloud_estimate_normals at that radius: the ones `direct` used
    assert np.array_equal(np.asarray(out["iss_normal_radius_index"], np.uint32), key)
    assert out["iss_refused"] == 0 and err.count("[pcl::ISSKeypoint3D::compute] The number of points in the input dataset differs") == 1
    assert "The border estimation" not in err


def test_scan_cloud_with_a_border(driven, direct):
    out, err = driven
    assert out["scan_refused"] == [0, 0, 0, 0] and "[ScanCloud::detectKeypoints] A border radius needs normals" in err and "[ScanCloud::detectBoundary] The cloud has no normals" in err
    assert out["scan_ok"] == [1, 1, 1] and out["scan_untouched"] == 1 and out["border_off_by_default"] == 1
    assert np.array_equal(np.asarray(out["scan_index"], np.uint32), direct["key"])
    assert np.array_equal(np.asarray(out["scan_no_border_index"], np.uint32), direct["plain"])
    assert np.array_equal(np.asarray(out["scan_plain_index"], np.uint32), direct["plain"])
    assert np.array_equal(np.asarray(out["scan_boundary"], bool), direct["flag"])
    assert out["scan_bad_angle"] == [0, 0] and "[ScanCloud::detectKeypoints] The border radius" in err
