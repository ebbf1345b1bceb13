"""GPU test of the C++ layers of the neighbour searches through tests/cxx/radius_driver.cpp (compiled here, as
tests/test_gpu_pfh_cxx.py compiles its driver): every overload of pcl::search::KdTree::radiusSearch / nearestKSearch and both
forms of ScanCloud::radiusSearch on two small clouds give the lists of tests/radius_ref.py and tests/normals_ref.py (passed to
the driver in a file; it reports the mismatching rows), with PCL's return values; setInputCloud twice searches the second cloud;
setSortedResults(false) keeps the sets; a k above MVR_MAX_KNN is refused."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import normals_ref as N
import radius_ref as R
import walk_cases as W
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

NA, NB, K, MAX_NN, RADIUS = 500, 300, 9, 5, 1.7


def csr_bytes(o, idx, d2):
    return o.astype("<u8").tobytes() + idx.astype("<u4").tobytes() + np.ascontiguousarray(d2, np.float32).view("<u4").tobytes()


def knn_csr(q, t, k):
    ki, kd = N.knn_brute(q, t, k)
    ok = ki != N.NONE
    o = np.zeros(len(q) + 1, np.uint64)
    o[1:] = np.cumsum(ok.sum(1))
    return o, ki[ok], kd[ok]


@pytest.fixture(scope="module")
def driven(built, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("radius_cxx")
    exe = str(tmp / "radius_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "radius_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    rng = np.random.default_rng(12)
    a = W.cloud(rng.standard_normal((NA, 3)) * 3 + [0, 0, 900])
    a[50:58] = a[49]                                                      # duplicates: ties the index decides
    b = W.cloud(rng.standard_normal((NB, 3)) * 3 + [0, 0, 900])
    b[:4] = a[49]
    b[10, :3] = [500.0, 0.0, 900.0]                                       # a query with nothing around it
    indices = rng.permutation(NB)[:40].astype(np.int32)
    indices[:3] = (10, 0, 0)                                              # ... listed, and one point listed twice
    cross_capped = R.radius_search(b, a, RADIUS, max_nn=MAX_NN)
    tables = [R.radius_search(a, a, RADIUS), R.radius_search(b[indices], a, RADIUS, max_nn=MAX_NN), knn_csr(b, a, K),
              R.radius_search(a, b, RADIUS), knn_csr(a, a, K), cross_capped]
    assert np.diff(tables[0][0].astype(np.int64)).max() > 20 and np.diff(tables[1][0].astype(np.int64)).tolist()[:3] == [0, MAX_NN, MAX_NN]
    path = str(tmp / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<5Id", NA, NB, len(indices), K, MAX_NN, RADIUS))
        f.write(a.astype("<f4").tobytes() + b.astype("<f4").tobytes() + indices.astype("<i4").tobytes())
        for t in tables:
            f.write(csr_bytes(*t))
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


def test_radius_search_overloads(driven):
    out, err = driven
    assert out["input_is_a"] == 1 and out["sorted_default"] == 1
    assert out["radius_batch"] == 0 and out["radius_batch_indices_max_nn"] == 0
    assert out["radius_single"] == [0, 0]                                 # the lists, and the return values
    assert out["unsorted"] == [0, 0, 0]


def test_nearest_k_search_overloads_and_refusals(driven):
    out, err = driven
    assert out["knn_batch"] == 0 and out["knn_single"] == [0, 0]
    assert out["no_input"] == [0, 0, 0, 1] and "No input dataset was given" in err
    assert out["refused"] == [0, 0, 0, 0, 0, 0]
    assert "k = 65 is outside 1..64" in err and "k = 0 is outside" in err and "is outside the cloud" in err and "must be finite and > 0" in err


def test_set_input_cloud_twice_and_the_ignored_tree(driven):
    out, err = driven
    assert out["second_input"] == [0, 1] and out["copy"] == [0, 0] and out["normals"] == NB


def test_scan_cloud_radius_search(driven):
    out, err = driven
    assert out["scan"] == [0, 0, 0, 0, 1, 0] and "[ScanCloud::radiusSearch] The radius" in err
