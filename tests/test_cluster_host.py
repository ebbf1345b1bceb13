"""CPU tests of the Euclidean cluster extraction's yardstick and surface: tests/cluster_ref.py against the hand-counted answers
of tests/cluster_cases.py and against scipy's radius graph (a kd-tree in f64 -- another route to the same components wherever
no pair lies within rounding of the tolerance), then the header's rules, the exported symbols, the binding's structures and
the argument refusals of rule E8, which need no GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import cluster_cases as CC
import cluster_ref as R
from conftest import PKG, ROOT

F32 = np.float32


def test_every_case_has_a_name(mvr):
    assert sorted(CC.names()) == sorted(CC.cases(mvr))


@pytest.mark.parametrize("name", CC.names())
def test_reference_gives_the_hand_counted_answers(mvr, name):
    case = CC.cases(mvr)[name]
    for fma in (False, True):
        ref = CC.reference(case, fma)
        res, lists, lab = ref["result"], ref["lists"], ref["labels"]
        n = len(case.pts)
        act = R.active_mask(n, case.kw.get("index"), case.kw.get("negative", False))
        # what holds of any answer (E5 - E7)
        sizes = [len(m) for m in lists]
        assert sizes == sorted(sizes, reverse=True) and res["n_clusters"] == len(lists) and res["n_clustered"] == sum(sizes)
        assert all(np.all(np.diff(m.astype(np.int64)) > 0) for m in lists)
        firsts = [int(m[0]) for m in lists]
        assert all(a < b for a, b, sa, sb in zip(firsts, firsts[1:], sizes, sizes[1:]) if sa == sb)
        assert np.array_equal(ref["offsets"], np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32))
        assert res["n_active"] == act.sum() and np.all(lab[~act] == R.NONE)
        assert res["n_components"] == res["n_clusters"] + res["too_small"] + res["too_large"]
        assert res["largest"] == (sizes[0] if sizes else 0)
        for k, m in enumerate(lists):
            assert np.all(lab[m] == k)
        assert (lab != R.NONE).sum() == sum(sizes)
        if case.expect is not None:
            want, small, large = case.expect
            assert sizes == sorted(want, reverse=True) and (res["too_small"], res["too_large"]) == (small, large), (name, fma, res)


def test_tie_rule_and_keep_on_the_twelve_blobs(mvr):
    case = CC.cases(mvr)["twelve_equal_blobs"]
    ref = R.clusters(case.pts, case.tolerance, keep=3)
    firsts = [int(m[0]) for m in ref["lists"]]
    assert firsts == sorted(firsts) and firsts[0] == 0
    assert np.array_equal(ref["kept"], np.sort(np.concatenate(ref["lists"][:3])))
    assert len(R.clusters(case.pts, case.tolerance, keep=99)["kept"]) == 240


@pytest.mark.parametrize("name", ["bounding_box_faces", "non_finite", "walk_size_257_several", "walk_planar_sheet_fraction", "two_snakes",
                                  "walk_two_far_clusters_fraction"])
def test_reference_agrees_with_scipys_radius_graph(mvr, name):
    case = CC.cases(mvr)[name]
    P = case.pts[:, :3].astype(np.float64)
    fin = np.isfinite(P).all(axis=1)
    ids = np.nonzero(fin)[0]
    tree = cKDTree(P[fin])
    r = case.tolerance
    near = tree.query_pairs(r * (1.0 + 1.0e-6), output_type="ndarray")
    d = np.linalg.norm(P[ids[near[:, 0]]] - P[ids[near[:, 1]]], axis=1)
    assert not np.any(np.abs(d - r) <= 1.0e-6 * r), "a pair within rounding of the tolerance: the f64 graph is no referee here"
    pairs = near[d <= r]
    g = coo_matrix((np.ones(len(pairs), np.int8), (ids[pairs[:, 0]], ids[pairs[:, 1]])), shape=(len(P), len(P)))
    _, lab = connected_components(g, directed=False)
    i, j = R.link_pairs(case.pts, r)
    root = R.roots_of(len(P), i, j)
    assert len(i) == len(pairs)
    # the same partition: labels map one to one
    assert len(set(zip(lab.tolist(), root.tolist()))) == len(set(lab.tolist())) == len(set(root.tolist()))


def test_dot_and_r2_follow_the_rules():
    assert R.r2_of(0.5) == F32(0.25) and R.r2_of(1.0e30) == np.finfo(F32).max and R.r2_of(1.0e-30) == 0
    assert R.dot_f64(F32([1, 0, 0]), F32([0, 1, 0])) == 0.0 and not (0.0 > math.cos(math.pi / 2))
    assert R.dot_f64(F32([0, 0, 1]), F32([0, 0, -1])) == -1.0 == math.cos(math.pi)
    assert np.isnan(R.dot_f64(F32([np.inf, 0, 1]), F32([0, 0, 1])))


# ------------------------------------------------------------------ the C-ABI

def test_header_declares_the_entry_and_the_rules():
    h = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    assert re.search(r"\bint\s+mvr_cloud_euclidean_clusters\(mvr_ctx \*ctx, int dst_slot[^;]*const mvr_cluster_params \*p,\s*const uint32_t \*index, "
                     r"size_t index_count,[^)]*mvr_cluster_result \*result, size_t \*n_out,[^)]*uint32_t \*cluster_offset, size_t offset_cap,"
                     r"[^)]*uint32_t \*cluster_index[^)]*uint32_t \*label[^)]*\);", h)
    assert re.search(r"\bvoid\s+mvr_cluster_default_params\(mvr_cluster_params \*p\);", h)
    assert "} mvr_cluster_params;" in h and "} mvr_cluster_result;" in h
    for rule in ["E%d." % k for k in range(1, 9)]:
        assert " " + rule + " " in h, rule
    assert h.count("DEVIATION", h.index(" E1. "), h.index(" E8. ")) >= 2
    sac = h[h.index(" P12. "):h.index("} mvr_sac_params;")]
    assert "Out of scope" in sac and "cluster" not in sac


def test_library_exports_the_entries(mvr):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    for sym in ("mvr_cloud_euclidean_clusters", "mvr_cluster_default_params"):
        assert sym in mvr.SIGNATURES and re.search(r" T %s$" % sym, r.stdout, re.M), sym
    assert (C.sizeof(mvr.ClusterParams), C.sizeof(mvr.ClusterResult)) == (48, 28)
    assert [f[0] for f in mvr.ClusterParams._fields_] == ["tolerance", "min_size", "max_size", "use_normals", "eps_angle", "negative", "keep",
                                                          "fma_dist"]
    assert [f[0] for f in mvr.ClusterResult._fields_] == ["n_active", "n_components", "n_clusters", "n_clustered", "largest", "too_small",
                                                          "too_large"]
    assert hasattr(mvr.Context, "euclidean_clusters")
    p = mvr.ClusterParams(9.0, 9, 9, 9, 9.0, 9, 9, 9)
    mvr._lib.mvr_cluster_default_params(C.byref(p))
    assert (p.tolerance, p.min_size, p.max_size, p.use_normals, p.eps_angle, p.negative, p.keep, p.fma_dist) == (0.0, 1, 2 ** 31 - 1, 0, 0.0, 0, 1, 0)
    mvr._lib.mvr_cluster_default_params(None)


def test_bad_arguments_are_refused_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                                  # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    res = mvr.ClusterResult(9, 9, 9, 9, 9, 9, 9)
    n_out = C.c_size_t(9)
    off, cidx, lab, one = (C.c_uint32 * 2)(9, 9), (C.c_uint32 * 1)(9), (C.c_uint32 * 1)(9), (C.c_uint32 * 1)(0)
    good = dict(tolerance=1.0, min_size=1, max_size=100, use_normals=0, eps_angle=0.0, negative=0, keep=1, fma_dist=0)

    def call(c, dst, src, with_res=True, null=False, index=None, count=0, **kw):
        a = dict(good, **kw)
        p = None if null else C.byref(mvr.ClusterParams(a["tolerance"], a["min_size"], a["max_size"], a["use_normals"], a["eps_angle"],
                                                        a["negative"], a["keep"], a["fma_dist"]))
        return L.mvr_cloud_euclidean_clusters(c, dst, src, p, index, count, C.byref(res) if with_res else None, C.byref(n_out), off, 2, cidx, lab)

    assert call(None, 1, 0) == mvr.E_ARG and call(ctx, 1, 0, null=True) == mvr.E_ARG and call(ctx, 1, 0, with_res=False) == mvr.E_ARG
    for s in (-1, mvr.MAX_SLOTS, 1 << 20):
        assert call(ctx, 1, s) == mvr.E_ARG
    for d in (-2, mvr.MAX_SLOTS, 1 << 20):
        assert call(ctx, d, 0) == mvr.E_ARG
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(ctx, -1, 0, tolerance=bad) == mvr.E_ARG
    assert call(ctx, 1, 0, keep=0) == mvr.E_ARG
    for bad in (0.0, -0.1, float(np.nextafter(math.pi, 4.0)), 4.0, math.nan, math.inf):
        assert call(ctx, -1, 0, use_normals=1, eps_angle=bad) == mvr.E_ARG
    assert call(ctx, -1, 0, index=None, count=1) == mvr.E_ARG
    assert tuple(getattr(res, f[0]) for f in mvr.ClusterResult._fields_) == (9,) * 7 and n_out.value == 9
    assert (off[0], off[1], cidx[0], lab[0], one[0]) == (9, 9, 9, 9, 0)
    assert fake.raw == b"\0" * 256


# ------------------------------------------------------------------ the kernels' resources

def test_cluster_kernels_use_no_scratch(built, tmp_path):
    assert "mvr_cluster.hip" in built.HIP_SOURCES
    src = os.path.join(ROOT, PKG, "csrc", "mvr_cluster.hip")
    assert '#include "mvr_union_find.h"' in open(src).read()
    den = open(os.path.join(ROOT, PKG, "csrc", "mvr_denoise.hip")).read()
    assert '#include "mvr_union_find.h"' in den and "uint32_t uf_find(" not in den      # one union-find, shared
    def usage(path):
        r = subprocess.run([built.HIPCC] + built.HIP_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", path, "-o", str(tmp_path / "device.o"),
                            "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        blocks = re.split(r"(?=remark: Function Name: )", r.stdout)[1:]
        return [(re.search(r"Function Name: (\S+)", b).group(1), int(re.search(r" VGPRs: (\d+)", b).group(1)),
                 int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))) for b in blocks]

    use = usage(src)
    own = [u for u in use if "cl_" in u[0] and "_kernel" in u[0]]
    # E1's marks are launch_mark of the filter tail (mvr_denoise.hip), shared with mvr_cloud_extract_indices: one mark kernel
    assert "mark_index_kernel" in den and not any("mark" in n for n, _, _ in use), use
    own += [u for u in usage(os.path.join(ROOT, PKG, "csrc", "mvr_denoise.hip")) if "mark_index_kernel" in u[0]]
    print(own)
    assert sum("cl_link_kernel" in n for n, _, _ in own) == 4                            # (fma) x (plain, normals)
    for kernel in ("mark_index_kernel", "cl_jump_kernel", "cl_label_kernel", "cl_root_key_kernel", "cl_rank_kernel", "cl_point_key_kernel",
                   "cl_offsets_kernel"):
        assert sum(kernel in n for n, _, _ in own) == 1, kernel
    assert all(s == 0 and v <= 64 for _, v, s in own), own                               # no spills; 8 waves per SIMD
