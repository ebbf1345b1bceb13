"""CPU tests of the correspondence rejectors: the numpy reference (tests/reject_ref.py) against plain loops, the conditions the
cases of tests/reject_cases.py promise, the arguments that are refused before any device is touched, and the layout of the three
structs against the Python bindings.  No GPU compute here."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import reject_cases as RC
import reject_ref as R
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def cases(mvr):
    return RC.build(mvr)


@pytest.fixture(scope="module")
def found(cases):
    """(case, reciprocal) -> the correspondences of an exhaustive search"""
    return {(name, rec): R.brute_correspondences(c["src"], c["tgt"], c["max_dist"], rec) for name, c in cases.items() for rec in (0, 1)}


def test_case_names(cases):
    assert tuple(cases) == RC.NAMES
    sizes = sorted({len(c["src"]) for c in cases.values()})
    assert {1, 2, 3, 65, 257, 6001, 20011} <= set(sizes)


def test_reference_against_plain_loops(cases, found):
    for name in ("lattice", "shared_target", "rand_65", "synth_257"):
        q, m, d = found[(name, 0)]
        n = len(q)
        assert n > 40
        # R3: the upper median is what sorting gives at position n / 2
        keep, thr = R.stage(q, m, d, ("median", 1.5))
        med = R.naive_median(d)
        assert float(thr) == med and np.array_equal(keep, d.astype(np.float64) <= med * 1.5)
        # R4: exactly nv, the smallest by (d2 bits, query)
        for ratio, minc in ((0.5, 0), (0.31, 0), (0.01, 9)):
            nv = R.trimmed_count(ratio, n, minc)
            keep, thr = R.stage(q, m, d, ("trimmed", ratio, minc))
            assert keep.sum() == nv == max(int(np.floor(ratio * n)), minc)
            assert q[keep].tolist() == R.naive_trimmed(q, d, nv) and float(thr) == float(d[keep].max())
        # R6: per target the smallest (d2 bits, query)
        keep, _ = R.stage(q, m, d, ("one_to_one",))
        assert q[keep].tolist() == R.naive_one_to_one(q, m, d) and len(set(m[keep].tolist())) == keep.sum() == len(set(m.tolist()))


def test_the_lattice_has_ties_at_both_cuts(cases, found):
    q, m, d = found[("lattice", 0)]
    values, counts = np.unique(d, return_counts=True)
    assert len(values) == 4 and counts.min() >= 150
    keep, thr = R.stage(q, m, d, ("trimmed", 0.6))
    equal = d == thr
    assert 0 < (keep & equal).sum() < equal.sum()                         # the cut falls inside a run of equal distances ...
    assert q[keep & equal].max() < q[~keep & equal].min()                 # ... and the lower query indices stay (R4's deviation)
    _, med = R.stage(q, m, d, ("median", 1.0))
    assert (d == med).sum() >= 150


def test_shared_targets_and_exact_dots(cases, found):
    q, m, d = found[("shared_target", 0)]
    assert len(q) >= 10 * len(set(m.tolist()))
    # equal distances to one target: the lower query index wins
    keep, _ = R.stage(q, m, d, ("one_to_one",))
    ties = 0
    for j in set(m.tolist()):
        g = np.nonzero(m == j)[0]
        best = R.bits(d[g]).min()
        tied = g[R.bits(d[g]) == best]
        ties += len(tied) > 1
        assert keep[tied[0]] and not keep[tied[1:]].any()
    assert ties >= 1
    c = cases["rand_257_palette"]
    q, m, d = found[("rand_257_palette", 0)]
    dots = R.dot_f32(c["snrm"][q], c["tnrm"][m])
    assert np.isnan(dots).sum() >= 10 and (dots == np.float32(0.6)).sum() >= 10
    keep, _ = R.stage(q, m, d, ("surface_normal", RC.DOT_EDGE), c["snrm"], c["tnrm"])
    assert not keep[np.isnan(dots)].any() and not keep[dots == np.float32(0.6)].any() and keep[dots == np.float32(0.8)].all()


def test_every_stage_rejects_and_keeps(cases, found):
    """the condition of tests/reject_cases.py"""
    checked = 0
    for name, c in cases.items():
        if name.startswith("degenerate"):
            continue
        for chain, recs in c["chains"]:
            for rec in recs:
                q, m, d = found[(name, rec)]
                _, _, _, stages = R.apply_chain(q, m, d, chain, c.get("snrm"), c.get("tnrm"))
                for k, s in enumerate(stages):
                    assert 3 <= s["n_out"] < s["n_in"], (name, chain, rec, k, s)
                checked += len(stages)
    assert checked >= 60
    kinds = {r[0] for c in cases.values() for chain, _ in c["chains"] for r in chain}
    assert kinds == set(R.KINDS)
    assert any(len(chain) == 8 for c in cases.values() for chain, _ in c["chains"])


def test_degenerate_cases_are_what_they_say(cases, found):
    q, m, d = found[("degenerate_keep_all", 0)]
    for chain, _ in cases["degenerate_keep_all"]["chains"]:
        _, _, _, st = R.apply_chain(q, m, d, chain)
        assert all(s["n_out"] == s["n_in"] == len(q) for s in st)
    q, m, d = found[("degenerate_empty_after", 0)]
    for chain, _ in cases["degenerate_empty_after"]["chains"]:
        _, _, _, st = R.apply_chain(q, m, d, chain)
        assert st[0]["n_out"] == 0 and all(s["n_in"] == 0 and float(s["threshold"]) == 0.0 for s in st[1:])
    assert len(found[("degenerate_no_match", 0)][0]) == 0
    assert R.trimmed_count(7.5e9, 300) == 0xFFFFFFFF and R.trimmed_count(0.2, 300, 100000) == 100000


def test_null_context_and_chain_length_are_refused(mvr):
    lib = mvr._lib
    one = (mvr.Rejector * 1)(mvr.rejector("median", 2.0))
    cnt = C.c_size_t(77)
    for n_chain in (0, 1, -1, mvr.MAX_REJECTORS + 1):
        assert lib.mvr_correspondences_rejected(None, 0, 1, 4.0, 1, 0, one, n_chain, None, None, None, 0, C.byref(cnt), None) == mvr.E_ARG
        assert lib.mvr_reject_correspondences(None, 0, 1, None, None, None, 0, one, n_chain, None, None, None, 0, C.byref(cnt), None) == mvr.E_ARG
        T = np.full(16, 5.0, np.float32)
        p = mvr.icp_params()
        assert lib.mvr_icp_align_rejected(None, 0, 1, 2, C.byref(p), one, n_chain, T.ctypes.data_as(C.POINTER(C.c_float)), None, None, 0) == mvr.E_ARG
        assert cnt.value == 77 and (T == 5.0).all()                       # nothing written


def test_struct_layout_equals_the_bindings(mvr, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mvr_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(mvr_rejector), offsetof(mvr_rejector, value),\n'
                   '         offsetof(mvr_rejector, min_correspondences), sizeof(mvr_rejector_stage), offsetof(mvr_rejector_stage, threshold),\n'
                   '         sizeof(mvr_icp_iter_trace), offsetof(mvr_icp_iter_trace, n_corr), offsetof(mvr_icp_iter_trace, mse),\n'
                   '         offsetof(mvr_icp_iter_trace, tr), MVR_MAX_REJECTORS);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    Rj, St, Tr = mvr.Rejector, mvr.RejectorStage, mvr.IcpIterTrace
    assert got == [C.sizeof(Rj), Rj.value.offset, Rj.min_correspondences.offset, C.sizeof(St), St.threshold.offset, C.sizeof(Tr), Tr.n_corr.offset,
                   Tr.mse.offset, Tr.tr.offset, mvr.MAX_REJECTORS]
    assert [mvr.REJ_DISTANCE, mvr.REJ_MEDIAN, mvr.REJ_TRIMMED, mvr.REJ_SURFACE_NORMAL, mvr.REJ_ONE_TO_ONE] == [0, 1, 2, 3, 4]
    r = mvr.rejector("trimmed", 0.8, 12)
    assert (r.kind, r.value, r.min_correspondences) == (mvr.REJ_TRIMMED, 0.8, 12)
