"""GPU test of the C++ layers of the ISS keypoints through tests/cxx/iss_driver.cpp (compiled here, as
tests/test_gpu_fpfh_cxx.py compiles its driver), on the recovery case of tests/align_cases.py:
  * pcl::ISSKeypoint3D through PCL's call order and ScanCloud::detectKeypoints return the indices of the C-ABI call
    (Context.iss_keypoints);
  * ScanCloud::alignPrerejective with use_keypoints returns, bit for bit, what mvr_align_prerejective returns when it is called
    directly with descriptor tables whose non-keypoint rows were overwritten with NaN in Python; the aligner's k-NN table has one
    row per source keypoint -- its draws (rule A2) depend on that row count, and its trace equals align_ref's replay over the
    keypoints alone.

No threshold on the quality of the recovery is fixed here.  The worst-point distance of the best pose from the true one, with
and without keypoints at equal iterations and seed, is printed.  NOT measured on a GPU when this was written."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import align_cases as AC
import align_ref as AR
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

F64 = np.float64
# 2.5 and 1.5 leaves of the 4 mm voxel grid of the recovery case: about 28 and 10 neighbours per ball; the numpy reference gives
# 246 keypoints of 3 097 source points and 212 of 3 150 target points, every ratio 2e-4 from its threshold
ISS = dict(salient_radius=10.0, non_max_radius=6.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5)


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


def worst_point(s, T):
    inv = np.linalg.inv(AC.REC_POSE.astype(F64))
    x = s[:, :3].astype(F64) @ T[:3, :3].astype(F64).T + T[:3, 3].astype(F64)
    y = s[:, :3].astype(F64) @ inv[:3, :3].T + inv[:3, 3]
    return float(np.linalg.norm(x - y, axis=1).max())


@pytest.fixture(scope="module")
def direct(mvr):
    """the two downsampled clouds of the recovery case, their keypoints, and what the aligner returns for the masked tables"""
    s_raw, t_raw = AC.recovery_view(mvr)
    pts, feat, key = [], [], []
    with mvr.Context(0) as ctx:
        for slot, raw in ((0, s_raw), (1, t_raw)):
            ctx.upload(slot, raw)
            ctx.voxel_grid(slot, slot, AC.REC_LEAF)
            ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS)
            pts.append(ctx.download(slot))
            feat.append(ctx.fpfh(slot, AC.REC_FPFH_RADIUS))
            key.append(ctx.iss_keypoints(-1, slot, return_index=True, **ISS)[1])
        masked = []
        for f, k in zip(feat, key):
            m = np.full_like(f, np.nan)
            m[k] = f[k]
            masked.append(m)
        plain = ctx.align_prerejective(0, 1, feat[0], feat[1], **AC.REC_PARAMS)
        plain_ms = ctx.stat("prerej_match_ms")
        res, tr = ctx.align_prerejective(0, 1, masked[0], masked[1], return_trace=True, **AC.REC_PARAMS)
        match_ms = ctx.stat("prerej_match_ms")
        el = AR.eligible(pts[0], masked[0])
        idx, _ = ctx.feature_knn(masked[0][el], masked[1], AC.REC_PARAMS["k"])
    print("recovery with keypoints: %d of %d source and %d of %d target points; converged %d at iteration %d, %d inliers, error %.4f, rejected %d, "
          "scored %d, worst displacement %.3f mm, matching %.2f ms | all points: converged %d at iteration %d, %d inliers, error %.4f, rejected %d, "
          "scored %d, worst displacement %.3f mm, matching %.2f ms"
          % (len(key[0]), len(pts[0]), len(key[1]), len(pts[1]), res["converged"], res["best_iteration"], res["inliers"], res["error"], res["rejected"],
             res["scored"], worst_point(pts[0], res["T"]), match_ms, plain["converged"], plain["best_iteration"], plain["inliers"], plain["error"],
             plain["rejected"], plain["scored"], worst_point(pts[0], plain["T"]), plain_ms))
    return dict(s=pts[0], t=pts[1], key=key, masked=masked, res=res, trace=tr, plain=plain, elig=el, knn=idx)


@pytest.fixture(scope="module")
def driven(built, direct, tmp_path_factory):
    built.build_hip()
    tmp = tmp_path_factory.mktemp("iss_cxx")
    exe = str(tmp / "iss_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "iss_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    files = []
    for name, p in (("source", direct["s"]), ("target", direct["t"])):
        files.append(str(tmp / (name + ".f32")))
        np.ascontiguousarray(p, np.float32).tofile(files[-1])
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    a = AC.REC_PARAMS
    args = [repr(ISS["salient_radius"]), repr(ISS["non_max_radius"]), repr(ISS["gamma_21"]), repr(ISS["gamma_32"]), str(ISS["min_neighbors"]),
            repr(AC.REC_NORMAL_RADIUS), repr(AC.REC_FPFH_RADIUS), str(a["max_iterations"]), str(a["nr_samples"]), str(a["k"]), repr(a["similarity"]),
            repr(a["max_dist"]), repr(a["inlier_fraction"]), str(a["seed"])]
    r = subprocess.run([exe] + files + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


def cm_bits(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(16).view(np.uint32)


def test_iss_keypoint3d_shim(driven, direct):
    out, err = driven
    key = direct["key"][0]
    assert 50 < len(key) < len(direct["s"]) // 4
    assert np.array_equal(np.asarray(out["shim_index"], np.uint32), key)
    assert np.array_equal(np.asarray(out["shim_points"], np.uint32).reshape(-1, 3), np.ascontiguousarray(direct["s"][key.astype(np.int64), :3]).view(np.uint32))
    assert np.array_equal(np.asarray(out["default_index"], np.uint32), key) and out["in_place_size"] == len(key)      # ISS holds PCL's defaults
    assert out["refused"] == [0, 0, 0, 0]
    assert "No input dataset given" in err and "must be finite and > 0" in err and err.count("The border estimation") == 2


def test_scan_cloud_detect_keypoints(driven, direct):
    out, err = driven
    assert out["scan_ok"] == 1 and out["scan_untouched"] == 1 and out["scan_refused"] == [0, 0]
    assert np.array_equal(np.asarray(out["scan_index"], np.uint32), direct["key"][0])
    assert np.array_equal(np.asarray(out["target_index"], np.uint32), direct["key"][1])
    assert "[ScanCloud::detectKeypoints] The radii" in err


def test_align_prerejective_on_keypoints(driven, direct):
    out, err = driven
    res, plain = direct["res"], direct["plain"]
    assert out["off_by_default"] == 1 and out["key_refused"] == 0
    # bit for bit the aligner's own answer to the masked tables
    assert np.array_equal(np.asarray(out["key_T"], np.uint32), cm_bits(res["T"]))
    assert (out["key_ok"], out["key_inliers"], out["key_best"], out["key_rejected"], out["key_scored"]) == \
           (int(res["converged"]), res["inliers"], res["best_iteration"], res["rejected"], res["scored"])
    # and with use_keypoints off, today's path
    assert np.array_equal(np.asarray(out["all_T"], np.uint32), cm_bits(plain["T"]))
    assert (out["all_ok"], out["all_inliers"], out["all_best"]) == (int(plain["converged"]), plain["inliers"], plain["best_iteration"])


def test_the_matcher_sees_one_row_per_source_keypoint(direct):
    """A1 packs the eligible rows: the masked source table has exactly the keypoints' rows left, the trace samples nothing else,
    and it equals the replay whose draws take ne = the number of source keypoints (another row count gives other draws)"""
    key, tr = direct["key"], direct["trace"]
    assert np.array_equal(direct["elig"], key[0])
    m = AC.REC_REPLAY
    st, src, tgt = AR.replay(direct["s"], direct["t"], direct["elig"], direct["knn"], m, 3, AC.REC_PARAMS["seed"], AC.REC_PARAMS["similarity"])
    assert np.array_equal(tr["status"][:m], st) and np.array_equal(tr["src"][:m], src) and np.array_equal(tr["tgt"][:m], tgt)
    live = tr["status"] != 2
    assert live.any() and np.isin(tr["src"][live], key[0]).all() and np.isin(tr["tgt"][live], key[1]).all()
