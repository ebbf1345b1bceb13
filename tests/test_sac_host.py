"""CPU tests of the plane segmentation that need no device: the draws of rule P2 against a frozen table and against the
independent statement of rule A2 in tests/align_ref.py, the numpy reference (tests/sac_ref.py) against the constructed answers
of tests/sac_cases.py and the iteration counts the loop of P7 must give, the measured bars of the refinement, the declarations,
the exported symbols, the argument refusals, and the resources of the kernels of csrc/mvr_sac.hip."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref as AR
import sac_cases as SC
import sac_ref as R
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ P2

def test_draws_against_a_frozen_table_and_rule_a2():
    assert [R.draw(0, 0, 0, 1 << 32), R.draw(1, 2, 3, 1000), R.draw((1 << 64) - 1, 5, 2, 6001)] == [3793791033, 529, 1976]
    got = [R.sample_positions(7, t, nv) for t in range(4) for nv in (3, 65, 6001)]
    assert got == [[1, 0, 2], [25, 1, 58], [2339, 100, 5405], [2, 0, 1], [57, 20, 40], [5278, 1958, 3715], [1, 0, 2], [24, 18, 37],
                   [2299, 1695, 3346], [2, 1, 0], [54, 41, 43], [5072, 3862, 4023]]
    # the other statement of A2 (numpy uint64 arithmetic, written for the prerejective alignment)
    t = np.arange(3000)
    for seed in (0, 1, 12345, (1 << 64) - 1):
        for j, m in ((0, 6001), (1, 6000), (2, 5999), (0, 3), (2, 1)):
            assert AR.draw(seed, t, j, m).tolist() == [R.draw(seed, int(i), j, m) for i in t]
        for i in (0, 1, 999):
            assert AR.sample_positions(seed, i, 65, 3) == R.sample_positions(seed, i, 65)


@pytest.mark.parametrize("nv", [3, 4, 5, 65, 6001])
def test_samples_are_distinct_and_in_range(nv):
    for t in range(10000):
        s = R.sample_positions(1, t, nv)
        assert len(set(s)) == 3 and min(s) >= 0 and max(s) < nv, (t, s)


def test_draw_order_would_repeat_a_sample():
    """why P2 says 'in ascending order of their value': the same correction applied in the order drawn gives repeats"""
    assert sum(len(set(R.sample_positions_in_draw_order(1, t, 5))) < 3 for t in range(10000)) > 100


# ------------------------------------------------------------------ the reference on the cases

@pytest.mark.parametrize("name,seed", SC.RUNS, ids=SC.IDS)
def test_every_stop_decision_keeps_its_margin(name, seed):
    p, kw, r = SC.reference(name, seed)      # (asserts the margin itself)
    assert r["min_margin"] >= R.K_MARGIN
    assert r["attempts"] == r["iterations"] + r["skipped"] == len(r["trace"]["status"])
    assert not r["mask"][~r["valid"]].any() and r["found"] == (name in SC.FOUND)


# the points a case puts on the plane that must win; at a threshold of 4-5 sigma of the noise all but 1 % of them are inliers,
# and only the other plane's points along the line where the two planes meet can join them
ON_PLANE = {"platter": (3001, 0), "mostly_object": (1001, 0), "far": (3001, 0), "small": (25, 0), "two_planes": (2458, 40),
            "right_angle": (900, 20), "perpendicular": (600, 20)}


@pytest.mark.parametrize("name", sorted(ON_PLANE))
def test_reference_recovers_the_constructed_plane(name):
    p, kw, r = SC.reference(name)
    want, extra = ON_PLANE[name]
    got = int(r["mask"].sum())
    nrm = r["coefficients"][:3].astype(F64)
    ang = R.angle_between(nrm, SC.plane_of(name))
    ang = min(ang, math.pi - ang)
    print("%s: %d inliers of %d on the plane, normal %.2e rad off, %d iterations" % (name, got, want, ang, r["iterations"]))
    assert 0.99 * want <= got <= want + extra
    assert ang < 5e-3      # noise of 0.1 mm over a disc of 60 mm and hundreds of points: well below 0.1 / 60
    assert abs(np.linalg.norm(nrm) - 1) < 1e-6


def test_lattice_has_its_closed_form():
    p, kw, r = SC.reference("lattice")
    co = r["ransac_coefficients"]
    assert co[0] == 0 and co[1] == 0 and abs(co[2]) == 1 and co[3] == 0          # integers: n = (0, 0, +-len) / len exactly
    assert np.array_equal(r["ransac_mask"], p[:, 2] == 0) and r["ransac_mask"].sum() == 196
    assert np.array_equal(r["mask"], p[:, 2] == 0)
    assert np.abs(np.abs(r["coefficients"]) - [0, 0, 1, 0]).max() < 1e-6


def test_the_larger_plane_wins_unless_the_axis_says_otherwise():
    p, kw, r = SC.reference("right_angle")
    q, kq, s = SC.reference("perpendicular")
    assert np.array_equal(p, q) and abs(r["coefficients"][0]) > 0.999 and abs(s["coefficients"][2]) > 0.999
    assert r["mask"].sum() > s["mask"].sum() > 0
    st = s["trace"]["status"]
    assert (st == R.INVALID).sum() >= 10 and (s["trace"]["inliers"][st == R.INVALID] == 0).all() and (r["trace"]["status"] == R.COUNTED).all()
    assert s["iterations"] == len(st)                                            # an invalid model is a counted iteration


def test_iteration_counts():
    for seed in (1, 2, 3):
        r = SC.reference("platter", seed)[2]
        assert 35 <= r["iterations"] <= 56 and 2950 <= r["mask"].sum() <= 3001
    r = SC.reference("mostly_object")[2]
    assert 900 <= r["iterations"] <= 1001 and r["attempts"] > 3 * 256            # many chunks, whatever their size
    r = SC.reference("mostly_object_50")[2]
    assert r["iterations"] == 51 and r["k"] > 51                                 # PCL's off-by-one: max_iterations + 1
    r = SC.reference("collinear")[2]
    assert (r["found"], r["iterations"], r["skipped"], r["attempts"]) == (False, 0, 100, 100) and (r["trace"]["status"] == R.SKIPPED).all()
    for name in ("n0", "n1", "n2", "all_invalid"):
        r = SC.reference(name)[2]
        assert (r["found"], r["attempts"], r["k"]) == (False, 0, 1.0) and not r["mask"].any()
    r = SC.reference("n3")[2]
    assert r["found"] and r["attempts"] == 1 and r["mask"].all()
    r = SC.reference("duplicates")[2]
    assert r["skipped"] >= 1 and r["found"]                                      # an attempt drew two copies of one point
    p, _, r = SC.reference("invalid_mixed")
    assert 0 < (~r["valid"]).sum() and r["nv"] < len(p) and np.isin(r["trace"]["sample"], np.nonzero(r["valid"])[0]).all()


def test_the_fma_case_is_one_where_fma_matters():
    """tests/test_gpu_sac.py::test_fma_distance would pass with fma_dist ignored on a case where the two chains agree"""
    plain, fma = SC.reference(SC.FMA_CASE, 1, False, False)[2], SC.reference(SC.FMA_CASE, 1, True, False)[2]
    assert same_trace_shape(plain, fma)
    differ = int((plain["trace"]["inliers"] != fma["trace"]["inliers"]).sum())
    print("%s: fma changes %d of %d counts, %d mask entries" % (SC.FMA_CASE, differ, plain["attempts"], (plain["ransac_mask"] != fma["ransac_mask"]).sum()))
    assert differ >= 1 and (plain["ransac_mask"] != fma["ransac_mask"]).any()
    q = SC.reference("mostly_object", 1, True, False)[2]
    assert q["attempts"] > 3 * 256 and fma["min_margin"] >= R.K_MARGIN and q["min_margin"] >= R.K_MARGIN


def same_trace_shape(a, b):
    return a["attempts"] == b["attempts"] and np.array_equal(a["trace"]["sample"], b["trace"]["sample"]) and np.array_equal(
        a["trace"]["coefficients"].view(np.uint32), b["trace"]["coefficients"].view(np.uint32))


def test_far_frame_gives_the_same_plane():
    a, b = SC.reference("platter")[2], SC.reference("far")[2]
    assert np.array_equal(a["trace"]["sample"], b["trace"]["sample"])            # the draws do not look at the coordinates
    assert R.angle_between(a["coefficients"][:3], b["coefficients"][:3]) < 1e-4 and b["mask"].sum() >= 2990


# ------------------------------------------------------------------ P10's bar

def _fits(name):
    p, kw, r = SC.reference(name)
    q = p[r["trace"]["sample"][r["best_attempt"]][0]]
    m, co = r["ransac_mask"], r["ransac_coefficients"]
    return R.eigh_fit(p, m, q, co), R.svd_fit(p, m, co), R.jacobi_fit(p, m, q, co)


def test_refinement_bars_are_the_measured_spread():
    ang = dd = 0.0
    for name in SC.REFINED:
        e, s, _ = _fits(name)
        a, d = R.angle_between(e[0], s[0]), abs(e[1] - s[1])
        print("%-16s eigh against svd: %.2e rad, d %.2e" % (name, a, d))
        ang, dd = max(ang, a), max(dd, d)
    print("largest: %.3e rad, %.3e; bars %.3e, %.3e" % (ang, dd, R.REFINE_ANGLE_BAR, R.REFINE_D_BAR))
    # the constants are not below the measurement; the ceiling only says that they are bars of f64 rounding, not of f32
    assert 4 * ang <= R.REFINE_ANGLE_BAR <= 1e-12 and 4 * dd <= R.REFINE_D_BAR <= 1e-9


@pytest.mark.parametrize("name", SC.REFINED)
def test_the_jacobi_route_stays_within_the_bars(name):
    e, _, j = _fits(name)
    assert R.angle_between(e[0], j[0]) <= R.REFINE_ANGLE_BAR and abs(e[1] - j[1]) <= R.REFINE_D_BAR


# ------------------------------------------------------------------ the C-ABI

def test_header_declares_the_entries_and_the_rules():
    h = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    assert re.search(r"\bint\s+mvr_cloud_segment_plane\(mvr_ctx \*ctx, int dst_slot[^;]*const mvr_sac_params \*p,\s*mvr_sac_result \*result", h)
    assert re.search(r"\bint\s+mvr_cloud_extract_indices\(mvr_ctx \*ctx, int dst_slot, int src_slot, const uint32_t \*index", h)
    assert "} mvr_sac_params;" in h and "} mvr_sac_result;" in h and "} mvr_sac_trace;" in h
    for rule in ["P%d." % k for k in range(1, 13)]:
        assert " " + rule + " " in h, rule
    assert h.count("DEVIATION", h.index(" P1. "), h.index(" P12. ")) >= 4 and '"sac_chunk"' in h


def test_library_exports_the_entries(mvr):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    for sym in ("mvr_cloud_segment_plane", "mvr_cloud_extract_indices"):
        assert sym in mvr.SIGNATURES and re.search(r" T %s$" % sym, r.stdout, re.M), sym
    assert (C.sizeof(mvr.SacParams), C.sizeof(mvr.SacResult), C.sizeof(mvr.SacTrace)) == (88, 72, 48)
    assert [f[0] for f in mvr.SacParams._fields_] == ["model", "threshold", "max_iterations", "probability", "optimize", "axis", "eps_angle",
                                                      "seed", "negative", "fma_dist"]
    assert [f[0] for f in mvr.SacResult._fields_] == ["found", "inliers", "ransac_inliers", "iterations", "attempts", "skipped", "best_attempt",
                                                      "k", "coefficients", "ransac_coefficients"]
    assert [f[0] for f in mvr.SacTrace._fields_] == ["status", "sample", "coefficients", "inliers", "k"]
    assert mvr.SAC_MODELS == {"plane": R.PLANE, "perpendicular_plane": R.PERPENDICULAR}
    assert hasattr(mvr.Context, "segment_plane") and hasattr(mvr.Context, "extract_indices")


def test_bad_arguments_are_refused_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                                  # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    res = mvr.SacResult(found=9, inliers=9)
    n_out = C.c_size_t(9)
    idx, flag = (C.c_uint32 * 1)(9), (C.c_uint8 * 1)(9)
    tr = (mvr.SacTrace * 1)()
    tr[0].status = 9
    good = dict(model=0, threshold=0.5, max_iterations=100, probability=0.99, optimize=1, axis=(0.0, 0.0, 1.0), eps_angle=0.1, seed=1,
                negative=0, fma_dist=0)

    def call(c, dst, src, with_res=True, **kw):
        a = dict(good, **kw)
        p = None if a.pop("null", False) else C.byref(mvr.SacParams(a["model"], a["threshold"], a["max_iterations"], a["probability"], a["optimize"],
                                                                    (C.c_double * 3)(*a["axis"]), a["eps_angle"], a["seed"], a["negative"], a["fma_dist"]))
        return L.mvr_cloud_segment_plane(c, dst, src, p, C.byref(res) if with_res else None, C.byref(n_out), idx, flag, tr, 1)

    assert call(None, 1, 0) == mvr.E_ARG and call(ctx, 1, 0, null=True) == mvr.E_ARG and call(ctx, 1, 0, with_res=False) == mvr.E_ARG
    for s in (-1, mvr.MAX_SLOTS, 1 << 20):
        assert call(ctx, 1, s) == mvr.E_ARG
    for d in (-2, mvr.MAX_SLOTS, 1 << 20):
        assert call(ctx, d, 0) == mvr.E_ARG
    for m in (-1, 2, 16):
        assert call(ctx, 1, 0, model=m) == mvr.E_ARG
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(ctx, 1, 0, threshold=bad) == mvr.E_ARG
    for bad in (0, -5, (1 << 24) + 1):
        assert call(ctx, 1, 0, max_iterations=bad) == mvr.E_ARG
    for bad in (0.0, 1.0, -0.1, 1.5, math.nan, math.inf):
        assert call(ctx, 1, 0, probability=bad) == mvr.E_ARG
    for bad in ((0.0, 0.0, 0.0), (math.nan, 0.0, 1.0), (0.0, math.inf, 1.0)):
        assert call(ctx, 1, 0, model=1, axis=bad) == mvr.E_ARG
    for bad in (0.0, -0.1, float(np.nextafter(math.pi / 2, 2.0)), 3.0, math.nan, math.inf):
        assert call(ctx, 1, 0, model=1, eps_angle=bad) == mvr.E_ARG
    one = (C.c_uint32 * 1)(0)
    assert L.mvr_cloud_extract_indices(None, 1, 0, one, 1, 0, C.byref(n_out)) == mvr.E_ARG
    assert L.mvr_cloud_extract_indices(ctx, 1, 0, None, 1, 0, C.byref(n_out)) == mvr.E_ARG
    for d, s in ((-1, 0), (1, -1), (mvr.MAX_SLOTS, 0), (1, mvr.MAX_SLOTS)):
        assert L.mvr_cloud_extract_indices(ctx, d, s, one, 1, 0, C.byref(n_out)) == mvr.E_ARG
    assert res.found == 9 and res.inliers == 9 and n_out.value == 9 and idx[0] == 9 and flag[0] == 9 and tr[0].status == 9
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the kernels' resources

def test_sac_kernels_use_no_scratch(built, tmp_path):
    assert "mvr_sac.hip" in built.HIP_SOURCES
    src = os.path.join(ROOT, PKG, "csrc", "mvr_sac.hip")
    r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "mvr_sac.o"),
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
    use = [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
            int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
           for b in blocks]
    print(use)
    for kernel, times in (("sac_hypotheses_kernel", 1), ("sac_flag_kernel", 2), ("sac_moments_kernel", 1), ("sac_fit_kernel", 1)):
        assert sum(kernel in n for n, _, _, _ in use) == times, (kernel, use)
    # the shared counting kernel (mvr_ransac.h) over this file's model: (1, 2, 4 registers) x fma
    count = sorted(l for n, _, _, l in use if "19ransac_count_kernel" in n and "PlaneModel" in n)
    assert len(count) == sum("count_kernel" in n for n, _, _, _ in use) == 6, use
    assert all(s == 0 for _, _, s, _ in use), use
    assert count == [256, 256, 512, 512, 1024, 1024]  # one counter per attempt of the chunk
    assert all(v <= 64 for _, v, _, _ in use)


def test_one_ransac_scaffold_shared():
    """the draws, the counting kernel, the replay of the loop and f32_at_least are mvr_ransac.h's, for both chunked RANSACs; the mark
    kernel of mvr_cloud_extract_indices is the filter tail's (launch_mark, mvr_denoise.hip), for the cluster extraction too"""
    csrc = os.path.join(ROOT, PKG, "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in os.listdir(csrc) if name.endswith((".hip", ".h", ".cpp"))}
    for name in ("mvr_sac.hip", "mvr_reject_sac.hip"):
        s = text[name]
        assert '#include "mvr_ransac.h"' in s and "float f32_at_least(" not in s, name
        assert not re.search(r"__global__[^;{]*count_kernel\s*\(", s), name
        assert "prerej_draw(" not in s and "ransac_draw3(" in s and ".replay(" in s and "ransac_launch_count<" in s, name
    for needle in ("float f32_at_least(", "void ransac_draw3(", "void replay(", r"ransac_count_kernel("):
        assert [name for name, s in text.items() if needle in s] == ["mvr_ransac.h"], needle
    assert "cl_mark_kernel" not in text["mvr_cluster.hip"] and "sac_mark_kernel" not in text["mvr_sac.hip"]
    assert "launch_mark(" in text["mvr_cluster.hip"] and "launch_mark(" in text["mvr_sac.hip"]
