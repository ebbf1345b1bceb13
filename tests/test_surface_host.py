"""Host tests of the reference of the features over a search surface (tests/surface_ref.py), of the cases the GPU tests run
(tests/surface_cases.py) and of what mvr_cloud_estimate_normals_at, mvr_cloud_fpfh_at and mvr_cloud_pfh_at refuse before they
touch a GPU."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fpfh_cases as FC
import fpfh_ref as R
import normals_ref as NR
import pfh_cases as PC
import pfh_ref as PR
import surface_cases as SC
import surface_ref as SR
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64
NAMES = ("mvr_cloud_estimate_normals_at", "mvr_cloud_fpfh_at", "mvr_cloud_pfh_at")


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


# ------------------------------------------------------------------ the reference against the references it generalises

def test_a_query_at_a_surface_point_has_the_neighbourhood_of_that_point():
    p, nrm, radius = FC.duplicates()
    q, m, bad = FC.with_invalid(p, nrm)
    idx = SC.subset_with_repeats(len(q))
    for fma in (False, True):
        I, J, d2 = SR.hoods_radius(q[idx], q, m, radius, fma)
        fI, fJ = R.pairs(q, m, radius, fma)
        valid = R.valid_mask(q, m)
        for r in (0, 5, len(idx) - 1):
            if valid[idx[r]]:
                assert np.array_equal(np.sort(J[I == r]), fJ[fI == idx[r]])
        # the weighting on a given table: the rows of fpfh_ref.fpfh_from_spfh
        C_ = R.spfh_counts(q, m, radius, fma, sets=(fI, fJ))
        S = R.spfh_from_counts(C_["full"], C_["n"], C_["valid"])
        want = R.fpfh_from_spfh(q, S, fI, fJ, valid, fma)[idx]
        got = SR.fpfh_from_spfh(len(idx), S, I, J, d2)
        v = valid[idx]
        assert np.allclose(got[v], want[v], rtol=1e-6, atol=1e-6)      # (the sums run in another order)
        # the pair counts: those of pfh_ref on the same neighbourhoods
        ref = PR.counts(q, m, PR.hoods_radius(q, m, radius, fma), np.unique(idx[v]))
        mine = SR.pfh_counts(len(idx), q, m, I, J, d2)
        pos = np.searchsorted(ref["queries"], idx[v])
        for key in ("n", "sure", "maybe", "slack", "full"):
            assert np.array_equal(mine[key][v], ref[key][pos]), key


def test_normals_reference_at_surface_points_is_the_whole_cloud_reference():
    p, _, radius = FC.box()
    idx = SC.subset_with_repeats(len(p))
    flat, offs = NR.radius_sets(p, radius)
    want, wc, _ = NR.normals_from_sets(p, flat, offs)
    I, J, _ = SR.hoods_radius(p[idx], p, None, radius)
    got, gc, _ = SR.normals_from_sets(p[idx], p, I, J)
    assert NR.angle_between(got, want[idx], unsigned=True).max() <= 1e-6 and np.abs(gc - wc[idx]).max() <= 1e-6
    kl, _ = NR.knn_brute(p, p, SC.K)
    want, wc, _ = NR.normals_from_lists(p, kl)
    got, gc, _ = SR.normals_from_lists(p[idx], p, SC.K)
    assert np.array_equal(got.view(np.uint32), want[idx].view(np.uint32)) and np.array_equal(gc.view(np.uint32), wc[idx].view(np.uint32))


def test_degenerate_queries_of_the_reference():
    p, nrm, radius = FC.box()
    nrm = nrm.copy()
    nrm[7, 1] = np.nan
    q = SC.degenerate(p, 7)
    I, J, d2 = SR.hoods_radius(q, p, nrm, radius)
    n = SR.neighbor_count(3, I)
    assert n[0] == 0 and n[1] == 0 and n[2] > 0 and 7 not in J
    S = np.zeros((len(p), 33), F32)
    f = SR.fpfh_from_spfh(3, S, I, J, d2)
    assert np.isnan(f[:2]).all() and (f[2] == 0).all()
    c = SR.pfh_counts(3, p, nrm, I, J, d2)
    assert list(c["n"][:2]) == [0, 0] and c["m"][2] == n[2] * (n[2] - 1) // 2
    rows = PR.rows_from_counts(c["full"], c["n"], np.ones(3, bool))
    assert np.isnan(rows[:2]).all() and np.isfinite(rows[2]).all()
    # k mode: the far query has its k neighbours, the NaN query none
    I, J, d2 = SR.hoods_knn(q, p, nrm, SC.K)
    assert list(SR.neighbor_count(3, I)) == [SC.K, 0, SC.K - 1]


# ------------------------------------------------------------------ the cases: the share of slack pairs

@pytest.mark.parametrize("name", SC.LARGE)
def test_slack_share_of_the_off_surface_cases(name, mvr):
    p, nrm, radius = SC.surface(name, mvr, lambda pts, r: FC.ref_normals(pts, r))
    q = SC.off_surface(p)
    assert len(q) == min(SC.SUBSET, len(p)) and np.isfinite(q[:, :3]).all()
    I, J, d2 = SR.hoods_radius(q, p, nrm, radius)
    rows = SC.reference_rows(name, len(q))
    c = SR.pfh_counts(len(q), p, nrm, I, J, d2, rows)
    share = c["slack"].sum() / max(c["pairs"], 1)
    print("%s: %d queries, %d pairs, slack share %.4f" % (name, len(q), c["pairs"], share))
    assert c["pairs"] > 1000 and share < PC.SLACK_CAP
    I, J, d2 = SR.hoods_knn(q, p, nrm, SC.K)
    c = SR.pfh_counts(len(q), p, nrm, I, J, d2)
    assert c["slack"].sum() / max(c["pairs"], 1) < PC.SLACK_CAP


# ------------------------------------------------------------------ the C-ABI and the wrapper

def test_library_exports_the_new_symbols(mvr):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, PKG, "libmvr_hip.so")], stdout=subprocess.PIPE, text=True, check=True)
    hdr = open(os.path.join(ROOT, "include", "mvr_hip.h")).read()
    for name in NAMES:
        assert name in mvr.SIGNATURES and re.search(r" T %s$" % name, r.stdout, re.M), name
        assert re.search(r"\b%s\(mvr_ctx \*ctx, int q_slot, const uint32_t \*indices, size_t n_indices, int surface_slot," % name, hdr)
    for name in ("estimate_normals_at", "fpfh_at", "pfh_at"):
        assert hasattr(mvr.Context, name)
    for q in range(1, 9):
        assert re.search(r"^ \*  Q%d\. " % q, hdr, re.M), q


def test_refusals_before_touching_the_gpu(mvr):
    L = mvr._lib
    fake = C.create_string_buffer(256)                                    # a context that is not one: any use of it would crash
    ctx = C.cast(fake, C.c_void_p)
    out, cnt = (C.c_float * 125)(*[9.0] * 125), (C.c_uint32 * 125)(*[9] * 125)
    idx = (C.c_uint32 * 2)(0, 1)
    fp, pp = mvr.FpfhParams(2.5, 0), mvr.PfhParams(2.5, 0, 0)
    npar = mvr.NormalParams(0, 2.5, (C.c_float * 3)(), 0)
    f, h, g = L.mvr_cloud_fpfh_at, L.mvr_cloud_pfh_at, L.mvr_cloud_estimate_normals_at
    assert f(None, 0, idx, 2, 1, C.byref(fp), out, cnt) == mvr.E_ARG
    assert h(None, 0, idx, 2, 1, C.byref(pp), out, cnt, cnt) == mvr.E_ARG
    assert g(None, 0, idx, 2, 1, C.byref(npar), 0, out, out) == mvr.E_ARG
    assert f(ctx, 0, idx, 2, 1, None, out, cnt) == mvr.E_ARG
    assert h(ctx, 0, idx, 2, 1, None, out, cnt, cnt) == mvr.E_ARG
    assert g(ctx, 0, idx, 2, 1, None, 0, out, out) == mvr.E_ARG
    for a, b in ((-1, 0), (0, -1), (mvr.MAX_SLOTS, 0), (0, mvr.MAX_SLOTS), (1 << 20, 1)):
        assert f(ctx, a, idx, 2, b, C.byref(fp), out, cnt) == mvr.E_ARG
        assert h(ctx, a, idx, 2, b, C.byref(pp), out, cnt, cnt) == mvr.E_ARG
        assert g(ctx, a, idx, 2, b, C.byref(npar), 0, out, out) == mvr.E_ARG
    for radius in (0.0, -1.0, math.nan, math.inf):
        assert f(ctx, 0, idx, 2, 1, C.byref(mvr.FpfhParams(radius, 0)), out, cnt) == mvr.E_ARG
    for radius, k in [(0.0, 0), (2.5, 16), (-1.0, 0), (math.nan, 0), (math.inf, 0), (0.0, -1), (0.0, 65)]:
        assert h(ctx, 0, idx, 2, 1, C.byref(mvr.PfhParams(radius, k, 0)), out, cnt, cnt) == mvr.E_ARG, (radius, k)
        assert g(ctx, 0, idx, 2, 1, C.byref(mvr.NormalParams(k, radius, (C.c_float * 3)(), 0)), 0, out, out) == mvr.E_ARG, (radius, k)
    assert g(ctx, 0, idx, 2, 1, C.byref(mvr.NormalParams(0, 2.5, (C.c_float * 3)(math.nan, 0.0, 0.0), 0)), 0, out, out) == mvr.E_ARG
    assert g(ctx, 0, idx, 2, 1, C.byref(npar), 1, out, out) == mvr.E_ARG                       # Q6: store_in_slot with indices
    assert list(out) == [9.0] * 125 and list(cnt) == [9] * 125
    assert fake.raw == b"\0" * 256


def test_wrapper_refuses_its_arguments_itself(mvr):
    c = mvr.Context.__new__(mvr.Context)                                   # no device: the checks come before any use of it
    for kw in (dict(), dict(radius=2.5, k=16)):
        with pytest.raises(ValueError):
            c.pfh_at(0, 1, **kw)
    c.size = lambda slot: 10
    for bad in (np.zeros((2, 2), np.uint32), np.array([0.5, 1.0]), np.array([-1, 2]), np.array([1 << 32])):
        with pytest.raises(ValueError):
            c._at_rows(0, bad)
    a, ptr, rows = c._at_rows(0, [3, 1, 3])
    assert a.dtype == np.uint32 and rows == 3 and ptr is not None
    assert c._at_rows(0, None) == (None, None, 10)
    assert c._at_rows(0, np.zeros(0, np.int64))[1:] != (None, 0) and c._at_rows(0, np.zeros(0, np.int64))[2] == 0
