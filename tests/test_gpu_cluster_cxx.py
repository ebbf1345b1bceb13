"""GPU test of the C++ layers of the Euclidean cluster extraction through tests/cxx/cluster_driver.cpp (compiled here, as
tests/test_gpu_sac_cxx.py compiles its driver), on the two interpenetrating sheets of tests/cluster_cases.py with three blobs
beside them (957 points with normals):
  * pcl::EuclideanClusterExtraction::extract returns the lists of the C-ABI call (Context.euclidean_clusters), with setIndices
    and without; pcl::extractEuclideanClusters with normals -- from a second cloud and from a PointNormal cloud's own -- the
    lists of the call with eps_angle; a missing tolerance, input or an index outside the cloud print an error and return nothing;
  * ScanCloud::extractClusters returns them too and changes nothing; ScanCloud::keepLargestClusters leaves the first `keep`
    clusters in their original order, the rich records following; parameters outside their range are refused;
  * Registrator::setObjectIsolation: off by default, and then saveRegisteredPoints writes, byte for byte, the files that
    io::savePCDFile / io::savePointsASC write from the merged cloud without the Registrator; switched on, it writes the merged
    object without the points ScanCloud::keepLargestClusters drops (plain and with a voxel grid), and counts them."""
import importlib
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as CC
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

TOLERANCE, MIN_SIZE, MAX_SIZE, EPS, KEEP = 0.6, 10, 100000, math.pi / 4, 2


def the_cloud():
    sp, sn = CC.sheets()
    b = CC.blobs([100, 50, 7], 21)
    b[:, 0] += 40.0
    bn = CC.nrm(np.tile([0.0, 0.0, 1.0], (len(b), 1)))
    order = np.random.default_rng(22).permutation(len(sp) + len(b))
    return np.concatenate([sp, b])[order], np.concatenate([sn, bn])[order]


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def direct(mvr):
    p, nrm = the_cloud()
    kw = dict(min_size=MIN_SIZE, max_size=MAX_SIZE, return_lists=True, return_labels=True)
    with mvr.Context(0) as ctx:
        ctx.upload(0, p)
        ctx.upload_normals(0, nrm)
        out = dict(p=p, nrm=nrm)
        out["plain"] = ctx.euclidean_clusters(-1, 0, TOLERANCE, **kw)
        out["third"] = ctx.euclidean_clusters(-1, 0, TOLERANCE, index=np.arange(0, len(p), 3), **kw)
        out["normals"] = ctx.euclidean_clusters(-1, 0, TOLERANCE, eps_angle=EPS, **kw)
        out["isolate"] = ctx.euclidean_clusters(-1, 0, TOLERANCE, min_size=MIN_SIZE, return_lists=True, return_labels=True)
    return out


@pytest.fixture(scope="module")
def driven(built, direct, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("cluster_cxx")
    exe = str(tmp / "cluster_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "cluster_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    cloud, normals = str(tmp / "cloud.f32"), str(tmp / "normals.f32")
    np.ascontiguousarray(direct["p"], np.float32).tofile(cloud)
    np.ascontiguousarray(direct["nrm"], np.float32).tofile(normals)
    for sub in ("off", "direct", "on", "off_again"):
        os.mkdir(str(tmp / sub))
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    args = [repr(TOLERANCE), str(MIN_SIZE), str(MAX_SIZE), repr(EPS), str(KEEP), str(tmp)]
    r = subprocess.run([exe, cloud, normals] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr, tmp


def same_lists(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(a, np.uint32), b) for a, b in zip(got, want))


def test_the_case_has_what_the_test_needs(direct):
    sizes = lambda key: [len(m) for m in direct[key][1]]
    print(sizes("plain"), sizes("third"), sizes("normals"), direct["plain"][0])
    assert sizes("plain") == [800, 100, 50] and sizes("normals") == [400, 400, 100, 50] and direct["plain"][0]["too_small"] == 1
    assert len(sizes("third")) >= 3


def test_euclidean_cluster_extraction_and_the_free_function(driven, direct):
    out, err, _ = driven
    assert out["defaults"] == [1, 2 ** 31 - 1, 1]
    assert same_lists(out["ece"], direct["plain"][1]) and same_lists(out["ece_third"], direct["third"][1])
    res = direct["plain"][0]
    assert out["ece_result"] == [res["n_components"], res["too_small"], res["too_large"]]
    assert same_lists(out["normals"], direct["normals"][1]) and same_lists(out["own_normals"], direct["normals"][1])
    assert out["refused"] == [0, 0, 0] and out["normals_refused"] == 0
    assert "[pcl::EuclideanClusterExtraction::extract] The cluster tolerance" in err and "[pcl::EuclideanClusterExtraction::extract] The index" in err
    assert "[pcl::EuclideanClusterExtraction::extract] No input dataset" in err and "[pcl::extractEuclideanClusters] Number of points" in err


def test_scan_cloud_extracts_and_keeps_clusters(driven, direct):
    out, err, _ = driven
    n = len(direct["p"])
    keep = direct["plain"][2] < KEEP
    assert out["scan_ok"] == [1, 1] and same_lists(out["scan_clusters"], direct["plain"][1])
    assert same_lists(out["scan_clusters_normals"], direct["normals"][1])
    assert out["scan_refused"] == [0, 0, 0, 0, n] and "[ScanCloud::extractClusters] The tolerance" in err
    assert out["scan_dropped"] == n - keep.sum() == n - 900
    assert np.array_equal(np.asarray(out["scan_points"], np.uint32).reshape(-1, 3), np.ascontiguousarray(direct["p"][keep, :3]).view(np.uint32))
    assert np.array_equal(np.asarray(out["scan_rich_follow"]), np.nonzero(keep)[0])


def test_object_isolation_in_front_of_save_registered_points(driven, direct):
    out, err, tmp = driven
    n = len(direct["p"])
    kept = int((direct["isolate"][2] < KEEP).sum())
    plain, wrote_direct, written, dropped, by_hand, merged, equal, written_leaf, dropped_leaf, small, read, back, off_again = out["isolation"]
    assert out["isolation_off_by_default"] == 1 and plain == n and wrote_direct == 1
    assert written == merged == kept == 900 and dropped == by_hand == dropped_leaf == n - kept and equal == 1
    assert read == 1 and back == written_leaf == small and 0 < written_leaf < written         # the voxel-grid variant isolates first
    assert off_again == 1
    for name in ("points.pcd", "points.asc"):                                                  # off: byte for byte what it wrote before
        ref = open(str(tmp / "direct" / name), "rb").read()
        assert len(ref) > 0 and open(str(tmp / "off" / name), "rb").read() == ref and open(str(tmp / "off_again" / name), "rb").read() == ref
