"""GPU test of the C++ layers of the surface reconstruction through tests/cxx/mc_driver.cpp (compiled here, as
tests/test_gpu_shot_cxx.py compiles its driver): pcl::MarchingCubesHoppe with PCL's members in PCL's order of calls on the sphere
of tests/mc_cases.py, the mesh written as mesh.ply and read back, against the arrays of the Python path (Context.
marching_cubes_hoppe) bit for bit; ScanCloud::reconstructMesh; and Registrator::saveRegisteredMesh on three synthetic views that
stand on a platter, with the platter removal on."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

import mc_cases as Cs
import mc_ref as R
from mc_cases import read_ply

pytestmark = pytest.mark.gpu
F32 = np.float32
RES, EXTEND = 24, 0.2
VIEWS, POINTS, CONFIG, MERGED_RES = 3, 2000, 1, 20


@pytest.fixture(scope="module")
def exe(built, tmp_path_factory):
    built.build_hip()
    out = str(tmp_path_factory.mktemp("mc_cxx") / "mc_driver")
    pkg = os.path.join(ROOT, PKG)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", "mc_driver.cpp"),
                        "-o", out, "-L" + pkg, "-lmvr_hip", "-Wl,-rpath," + pkg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return out


def drive(exe, *args):
    env = dict(os.environ)
    env.pop("MVR_RCCL_LIB", None)
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout), r.stderr


@pytest.fixture(scope="module")
def ctx():
    mvr = importlib.import_module(PKG)
    c = mvr.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("weld", [0, 1])
def test_marching_cubes_hoppe_members_and_mesh_file(exe, ctx, tmp_path, weld):
    p, n = Cs.sphere()
    np.concatenate([p, n], 1).astype(F32).tofile(tmp_path / "cloud.bin")
    out, err = drive(exe, "shim", tmp_path / "cloud.bin", RES, EXTEND, weld, tmp_path)
    assert out["defaults"] == [32, 32, 32, 0, 0, -1, 0] and out["no_input"] == [0, 0] and "No input dataset given" in err
    assert out["res"] == [RES] * 3 and out["read_back"] == 1 and out["overload"] == 1
    assert out["refused"] == [0, 0] and "grid resolution below 2" in err
    ctx.upload(0, p)
    ctx.upload_normals(0, n)
    v, t = ctx.marching_cubes_hoppe(0, (RES,) * 3, percentage_extend_grid=EXTEND, weld=bool(weld))
    assert out["mesh"] == [len(v), len(t)] and len(t) > 1000
    for name in ("mesh.ply", "scan.ply"):
        fv, ff = read_ply(tmp_path / name)
        assert R.same_bits(fv, v) and np.array_equal(np.array(ff, np.uint32), t), name
    assert out["scan"] == [1, len(v), len(t)]
    if weld:
        assert R.closed_and_oriented(t) and R.euler(len(v), t) == 2
    # voxel_size 10 on a box of 1.2 * ~100 mm: about 13 vertices per axis; 1e-4: refused; no normals: refused
    by_voxel = len(ctx.marching_cubes_hoppe(0, [int(np.ceil(float(e) * (1.0 + EXTEND) / 10.0)) + 1 for e in (p.max(0).astype(np.float64) - p.min(0))],
                                            percentage_extend_grid=EXTEND)[1])
    assert out["by_voxel"] == [1, by_voxel] and out["too_fine"] == [0, 0] and out["bare"] == [0, 0]
    assert "above the limit" in err and "has no normals" in err


def test_save_registered_mesh_with_platter_removal(exe, ctx, tmp_path):
    for sub in ("off", "bare"):
        os.mkdir(tmp_path / sub)
    out, err = drive(exe, "registered", VIEWS, POINTS, CONFIG, MERGED_RES, tmp_path)
    platter = out["platter_points"]
    n_points, taken, taken_mesh = out["points"]
    assert platter == VIEWS * (POINTS // 4) and taken == taken_mesh and platter * 0.9 <= taken <= platter * 1.1
    assert n_points == VIEWS * (POINTS + POINTS // 4) - taken
    merged = np.fromfile(tmp_path / "merged.bin", F32).reshape(-1, 6)
    assert len(merged) == n_points
    ctx.upload(1, merged[:, :3].copy())
    ctx.upload_normals(1, merged[:, 3:].copy())
    v, t = ctx.marching_cubes_hoppe(1, (MERGED_RES,) * 3, percentage_extend_grid=0.1, weld=True)
    fv, ff = read_ply(tmp_path / "mesh.ply")
    assert out["on"] == [len(t), len(v), len(t)] and len(t) > 100
    assert R.same_bits(fv, v) and np.array_equal(np.array(ff, np.uint32), t)
    assert os.path.exists(tmp_path / "points.pcd")                                   # mesh.ply lies beside it
    # without the removal the platter is part of the surface: another mesh
    assert out["off"][0] == out["off"][1] > 0 and os.path.exists(tmp_path / "off" / "mesh.ply")
    assert read_ply(tmp_path / "off" / "mesh.ply")[0].shape != fv.shape
    # a merge without normals writes nothing
    assert out["bare"] == 0 and os.listdir(tmp_path / "bare") == []
