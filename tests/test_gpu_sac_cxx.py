"""GPU test of the C++ layers of the plane segmentation through tests/cxx/sac_driver.cpp (compiled here, as
tests/test_gpu_iss_cxx.py compiles its driver), on the 6 001-point view with a platter of tests/sac_cases.py:
  * pcl::SACSegmentation::segment returns the indices and coefficients of the C-ABI call (Context.segment_plane) and
    pcl::ExtractIndices::filter, with setNegative(true) and without, the points of Context.extract_indices; the perpendicular
    model finds the platter along its axis and something much smaller along an axis that lies in it; another method or model
    throws, a missing threshold and an index outside the cloud print an error and return nothing;
  * ScanCloud::segmentPlane returns them too and changes nothing; ScanCloud::removePlane leaves the other points, the rich
    records following; parameters outside their range are refused;
  * Registrator::setPlatterRemoval: off by default; switched on, saveRegisteredPoints (plain and with a voxel grid) writes the
    merged object without the points ScanCloud::removePlane takes out along the registrator's axis, and counts them."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import sac_cases as SC
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

THRESHOLD, MAX_ITERATIONS, SEED, AXIS, EPS = 0.5, 1000, 3, (0.0, 0.0, 1.0), 0.1


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def direct(mvr):
    p = SC.CASES["platter"][0]
    with mvr.Context(0) as ctx:
        ctx.upload(0, p)
        res, idx = ctx.segment_plane(-1, 0, THRESHOLD, max_iterations=MAX_ITERATIONS, seed=SEED, return_index=True)
        out = dict(p=p, res=res, idx=idx)
        out["perp"] = ctx.segment_plane(-1, 0, THRESHOLD, model="perpendicular_plane", axis=AXIS, eps_angle=EPS, max_iterations=MAX_ITERATIONS,
                                        seed=SEED, return_index=True)[1]
        out["perp_other"] = ctx.segment_plane(-1, 0, THRESHOLD, model="perpendicular_plane", axis=AXIS[1:] + AXIS[:1], eps_angle=EPS,
                                              max_iterations=MAX_ITERATIONS, seed=SEED, return_index=True)[1]
        assert ctx.extract_indices(1, 0, idx, negative=True) == len(p) - len(idx)
        out["negative"] = ctx.download(1)
        assert ctx.extract_indices(1, 0, idx) == len(idx)
        out["positive"] = ctx.download(1)
    return out


@pytest.fixture(scope="module")
def driven(built, direct, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("sac_cxx")
    exe = str(tmp / "sac_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "sac_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    cloud = str(tmp / "cloud.f32")
    np.ascontiguousarray(direct["p"], np.float32).tofile(cloud)
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    args = [repr(THRESHOLD), str(MAX_ITERATIONS), str(SEED)] + [repr(a) for a in AXIS] + [repr(EPS)]
    args.append(str(tmp))
    r = subprocess.run([exe, cloud] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


def xyz_bits(p):
    return np.ascontiguousarray(p[:, :3]).view(np.uint32)


def test_the_case_has_a_platter(direct):
    n, res = len(direct["p"]), direct["res"]
    print("%d points, %d on the plane after %d iterations; %d along the axis, %d along an axis in the platter"
          % (n, len(direct["idx"]), res["iterations"], len(direct["perp"]), len(direct["perp_other"])))
    assert res["found"] and 2950 <= len(direct["idx"]) <= 3001 and np.array_equal(direct["perp"], direct["idx"])
    assert 0 < len(direct["perp_other"]) < len(direct["idx"]) // 10


def test_sac_segmentation_and_extract_indices(driven, direct):
    out, err = driven
    assert out["defaults"] == [50, 1, 1]
    assert np.array_equal(np.asarray(out["seg_index"], np.uint32), direct["idx"]) and out["seg_iterations"] == direct["res"]["iterations"]
    assert np.array_equal(np.asarray(out["seg_coefficients"], np.uint32), direct["res"]["coefficients"].view(np.uint32))
    assert np.array_equal(np.asarray(out["extract_negative"], np.uint32).reshape(-1, 3), xyz_bits(direct["negative"]))
    assert np.array_equal(np.asarray(out["extract_positive"], np.uint32).reshape(-1, 3), xyz_bits(direct["positive"]))
    assert np.array_equal(np.asarray(out["perp_index"], np.uint32), direct["perp"])
    assert np.array_equal(np.asarray(out["perp_other_index"], np.uint32), direct["perp_other"])
    assert out["refused"] == [2, 0, 0]
    assert "[pcl::SACSegmentation::segment] The distance threshold" in err and "[pcl::ExtractIndices::filter] The index" in err


def test_scan_cloud_segments_and_removes_the_plane(driven, direct):
    out, err = driven
    n, idx = len(direct["p"]), direct["idx"]
    keep = np.ones(n, bool)
    keep[idx] = False
    assert out["scan_ok"] == [1, 1] and np.array_equal(np.asarray(out["scan_index"], np.uint32), idx)
    assert out["scan_refused"] == [0, 0, 0, n] and "[ScanCloud::segmentPlane] The threshold" in err
    assert out["scan_removed"] == len(idx)
    assert np.array_equal(np.asarray(out["scan_points"], np.uint32).reshape(-1, 3), xyz_bits(direct["p"][keep]))
    assert np.array_equal(np.asarray(out["scan_rich_follow"]), np.nonzero(keep)[0])


def test_platter_removal_in_front_of_save_registered_points(driven, direct):
    out, err = driven
    n, on_plane = len(direct["p"]), len(direct["perp"])
    plain, written, taken, removed, merged, equal, written_leaf, taken_leaf, small, read, back, off_again = out["platter"]
    assert out["platter_off_by_default"] == 1 and plain == n                       # off: the merged object as it is
    assert taken == removed == on_plane and written == merged == n - on_plane      # on: ScanCloud::removePlane along the registrator's axis
    assert equal == 1 and read == 1 and back == written_leaf                       # the points left are removePlane's; the file holds what the last call wrote
    assert taken_leaf == on_plane and 0 < written_leaf == small < written          # the voxel-grid variant removes the platter first
    assert off_again == 1                                                          # a threshold of 0 switches it off again
