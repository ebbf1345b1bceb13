"""GPU test of the C++ layer of the Normal Distributions Transform through tests/cxx/ndt_driver.cpp (compiled here, as
tests/test_gpu_gicp_cxx.py compiles its driver), on the `centred` pair of tests/ndt_cases.py:
  * pcl::NormalDistributionsTransform has PCL's defaults and PCL's names; align(out) and align(out, guess) return what
    Context.ndt_align returns, within the parity bars; the getters say what the stats say; `out` is the output slot;
  * a target without a cell leaves the guess as the final transformation, not converged;
  * ScanCloud::alignNDT rotates about the centre of the target's bounding box and returns that align's pose."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import ndt_cases as NC
import ndt_ref as R
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

ROT_TOL, TRANS_TOL = 1e-5, 1e-4          # tests/test_gpu_parity.py:17


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def direct(mvr):
    case = NC.centred("res5")
    guess = R.pose_matrix(0.5 * NC.P_STAR).astype(np.float32)
    out = dict(case=case, guess=guess)
    p = mvr.ndt_params(**case["prm"])
    t = case["tgt"][:, :3].astype(np.float64)
    centre = 0.5 * (t.min(0) + t.max(0))
    with mvr.Context(0) as ctx:
        ctx.upload(0, case["src"])
        ctx.upload(1, case["tgt"])
        out["plain"] = ctx.ndt_align(0, 1, 2, p)
        out["plain_out"] = ctx.download(2)
        out["fitness"] = ctx.fitness(0, 1, out["plain"][0])
        out["guess_run"] = ctx.ndt_align(0, 1, 2, p, guess.astype(np.float64))
        out["scan"] = ctx.ndt_align(0, 1, -1, mvr.ndt_params(origin=tuple(centre), **case["prm"]))
    return out


@pytest.fixture(scope="module")
def ndt_exe(built, tmp_path_factory):
    built.build_hip()
    exe = str(tmp_path_factory.mktemp("ndt_cxx_exe") / "ndt_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "ndt_driver.cpp"),
                        "-o", exe, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def drive(exe, tmp, case, guess):
    files = []
    for key in ("src", "tgt"):
        files.append(str(tmp / (key + ".f32")))
        np.ascontiguousarray(case[key], np.float32).tofile(files[-1])
    files.append(str(tmp / "guess.f32"))
    np.ascontiguousarray(guess.T).reshape(16).tofile(files[-1])
    prm = case["prm"]
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe] + files + [repr(prm["resolution"]), repr(prm["step_size"]), repr(prm["transformation_epsilon"])],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


@pytest.fixture(scope="module")
def driven(ndt_exe, direct, tmp_path_factory):
    return drive(ndt_exe, tmp_path_factory.mktemp("ndt_cxx"), direct["case"], direct["guess"])


def from_words(words):
    return np.asarray(words, np.uint32).view(np.float32).reshape(4, 4).T.astype(np.float64)


def within_bars(A, B, what):
    dr, dt = np.abs(A[:3, :3] - B[:3, :3]).max(), np.abs(A[:3, 3] - B[:3, 3]).max()
    print("%s: rotation within %.2g, translation within %.2g" % (what, dr, dt))
    assert dr <= ROT_TOL and dt <= TRANS_TOL, (what, dr, dt)


def test_class_defaults_and_setters(driven):
    out, _ = driven
    assert out["defaults"] == [1, 1, 1, 1, 35, 6, 0, 0] and out["setters"] == [1, 1, 1, 1]


def test_align_and_getters(driven, direct, mvr):
    out, _ = driven
    T, X, st, rc = direct["plain"]
    assert rc == 0 and st["stop"] == "STEP"
    within_bars(from_words(out["T"]), T.astype(np.float64), "align(out)")
    assert out["api"] == [1, st["iterations"], st["evaluations"], len(direct["case"]["src"]), mvr.NDT_STOPS.index(st["stop"])]
    assert out["score"] == st["score"] and abs(out["probability"] - st["score"] / len(direct["case"]["src"])) <= 1e-15 * st["score"]
    assert abs(out["fitness"] - direct["fitness"]) <= 1e-4 * direct["fitness"]
    got = np.asarray(out["out"], np.uint32).view(np.float32).reshape(-1, 2)
    assert np.array_equal(got, direct["plain_out"][::97][:, [0, 2]])
    assert NC.residual(from_words(out["T"]), direct["case"]) <= 2 * NC.residual(X, direct["case"])


def test_align_with_a_guess(driven, direct, mvr):
    out, err = driven
    T, X, st, rc = direct["guess_run"]
    assert rc == 0
    within_bars(from_words(out["guess_T"]), T.astype(np.float64), "align(out, guess)")
    assert out["guess_api"] == [int(st["converged"]), st["iterations"], st["evaluations"], len(direct["case"]["src"]), mvr.NDT_STOPS.index(st["stop"])]
    # no cell: the guess comes back, nothing converged, and the class says why on stderr
    assert np.array_equal(from_words(out["none_T"]), direct["guess"].astype(np.float64))
    assert out["none_api"] == [0, 0, mvr.NDT_STOPS.index("NO_OVERLAP")] and "overlaps no cell" in err


def test_scan_cloud_align_ndt(driven, direct):
    out, _ = driven
    T, X, st, rc = direct["scan"]
    assert rc == 0 and out["scan_ok"][:2] == [1, st["iterations"]]
    pose = np.asarray(out["scan_pose"], np.float64).reshape(4, 4).T        # RowMatrixd: the row-vector convention
    within_bars(pose, T.astype(np.float64), "ScanCloud::alignNDT")
    case = direct["case"]
    t = case["tgt"][:, :3].astype(np.float64)
    prm = R.params(origin=tuple(0.5 * (t.min(0) + t.max(0))), **case["prm"])
    ref = R.align(case["src"], R.build_cells(case["tgt"], prm), prm)
    assert NC.residual(pose, case) <= 2 * NC.residual(ref["X"], case)


def test_flat_stop_through_the_class(ndt_exe, mvr, tmp_path_factory):
    """the one-cell case `flat-0` of tests/ndt_cases.py (the source's one point on the cell's mean: g = 0): the class reports
    what Context.ndt_align reports -- not converged, 0 iterations, 1 evaluation, stop FLAT, the final transformation the
    guess (here I) and `out` the source --, and so does ScanCloud::alignNDT, which turns about that same point"""
    case = [c for c in NC.branch_cases() if c["name"] == "flat-0"][0]
    flat = mvr.NDT_STOPS.index("FLAT")
    prm = dict(case["prm"], origin=(0.0, 0.0, 0.0), min_points_per_voxel=6)          # what the class sets
    with mvr.Context(0) as ctx:
        ctx.upload(0, case["src"])
        ctx.upload(1, case["tgt"])
        T, X, st, rc = ctx.ndt_align(0, 1, -1, mvr.ndt_params(**prm))
    assert rc == 0 and (st["stop"], st["converged"], st["iterations"], st["evaluations"]) == ("FLAT", False, 0, 1) and np.array_equal(X, np.eye(4))
    out, _ = drive(ndt_exe, tmp_path_factory.mktemp("ndt_cxx_flat"), case, np.eye(4, dtype=np.float32))
    assert out["api"] == [0, 0, 1, 1, flat] and out["guess_api"] == [0, 0, 1, 1, flat]
    assert np.array_equal(from_words(out["T"]), np.eye(4)) and np.array_equal(from_words(out["guess_T"]), np.eye(4))
    assert out["score"] == st["score"] and out["probability"] == st["score"]
    assert np.array_equal(np.asarray(out["out"], np.uint32).view(np.float32), case["src"][0, [0, 2]])
    assert out["none_api"] == [0, 0, mvr.NDT_STOPS.index("NO_OVERLAP")]
    assert out["scan_ok"][1:] == [0, flat] and np.array_equal(np.asarray(out["scan_pose"]).reshape(4, 4), np.eye(4))
