"""GPU tests of the ISS keypoints (mvr_cloud_iss_keypoints; rules K1-K8 in include/mvr_hip.h) against the numpy reference of
tests/iss_ref.py on the inputs of tests/iss_cases.py.

Two correct implementations differ by the order of the sums and the rounding of the eigen-solver, so nothing here is a tolerance
on a flag.  The counts are exact on every case.  The saliency is within GAP / 4 relative of the reference wherever the reference
is salient and exactly 0 wherever the reference is DECIDEDLY not salient (iss_ref.decided: no rounding can change it; on the
rank-deficient sets -- collinear, the planar lattice -- e3 is rounding itself and only the counts and the suppression are
compared).  The keypoints equal, exactly and on every case, the non-maximum suppression recomputed on the host from the GPU's
OWN saliencies over the reference's neighbour sets.  Where tests/test_iss_host.py has shown the input to keep every ratio GAP
from its threshold and every pair of neighbouring saliencies GAP apart (view, view_tight, box, non_finite), the keypoints and
the downloaded points equal the reference's exactly.

NOT measured on a GPU when this was written: no device was available.  The comparisons below were run once against a stand-in
context whose detector is the numpy reference, so they are known to hold for a correct implementation.  The same holds for the
targets of the walk cases (iss_cases.WALK) and for the four grid resolutions, added later."""
import importlib

import numpy as np
import pytest

import fpfh_cases as FC
import iss_cases as IC
import iss_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

RUNS = [(n, False) for n in IC.NAMES] + [(n, True) for n in IC.FMA_CASES]
IDS = ["%s%s" % (n, "-fma" if f else "") for n, f in RUNS]


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def ctx(mvr):
    c = mvr.Context(0)
    yield c
    c.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def detect(ctx, c, dst, src, fma=False):
    n_out, idx, sal, sc, nc = ctx.iss_keypoints(dst, src, fma=fma, return_index=True, return_saliency=True, return_counts=True, **IC.params(c))
    assert n_out == len(idx) and sal.shape == sc.shape == nc.shape == (len(c["p"]),)
    return dict(index=idx, saliency=sal, salient_count=sc, nms_count=nc)


_gpu = {}


def gpu_run(name, fma, mvr, ctx):
    """(case, reference, the GPU's result into slot 1 with the downloaded keypoints), once per case"""
    if (name, fma) not in _gpu:
        c, ref = IC.reference(name, mvr, fma)
        ctx.upload(0, c["p"])
        g = detect(ctx, c, 1, 0, fma)
        g["points"] = ctx.download(1)
        assert same_bits(ctx.download(0), c["p"])                       # the source is left as it was
        _gpu[(name, fma)] = (c, ref, g)
    return _gpu[(name, fma)]


def check_counts(c, ref, g):
    assert np.array_equal(g["salient_count"], ref["salient_count"])
    ball = np.diff(ref["sets"][1][1]).astype(np.uint32)
    assert np.array_equal(g["nms_count"], np.where(g["saliency"] != 0, ball, 0))      # K5: 0 for a point that is not salient
    d = R.decided(ref)
    assert np.array_equal(g["nms_count"][d], ref["nms_count"][d])
    assert (g["salient_count"][~ref["valid"]] == 0).all() and (g["saliency"][~ref["valid"]] == 0).all()


def check_saliency(c, ref, g, name, fma):
    s = ref["salient"]
    rel = np.abs(g["saliency"][s] - ref["saliency"][s]) / ref["saliency"][s]
    off = R.decided(ref) & ~s
    print("%s fma=%d: %d salient, largest relative difference of a saliency %.2e; %d of %d points decidedly not salient, %d undecided"
          % (name, fma, s.sum(), rel.max(initial=0.0), off.sum(), len(s), (~R.decided(ref)).sum()))
    assert rel.max(initial=0.0) <= R.GAP / 4
    assert (bits(g["saliency"][off]) == 0).all()                        # +0.0 exactly
    assert np.isfinite(g["saliency"]).all() and (g["saliency"] >= 0).all()


def check_suppression(c, ref, g):
    flat, offs = ref["sets"][1]
    cnt, key = R.nms(g["saliency"], flat, offs, c["min_neighbors"])
    assert np.array_equal(g["index"], np.nonzero(key)[0].astype(np.uint32))
    assert np.array_equal(g["nms_count"], cnt)
    out = c["p"][g["index"].astype(np.int64)].copy()
    out[:, 3] = 1.0
    assert same_bits(g["points"], out)                                 # K6: ascending original index, w = 1


@pytest.mark.parametrize("name,fma", RUNS, ids=IDS)
def test_counts_are_exact(name, fma, mvr, ctx):
    check_counts(*gpu_run(name, fma, mvr, ctx))


@pytest.mark.parametrize("name,fma", RUNS, ids=IDS)
def test_saliency_against_the_reference(name, fma, mvr, ctx):
    check_saliency(*gpu_run(name, fma, mvr, ctx), name, fma)


@pytest.mark.parametrize("name,fma", RUNS, ids=IDS)
def test_keypoints_are_the_suppression_of_the_gpus_own_saliencies(name, fma, mvr, ctx):
    """no tolerance, on the degenerate and tie-ridden sets too"""
    check_suppression(*gpu_run(name, fma, mvr, ctx))


@pytest.mark.parametrize("name", ["box", "view_tight", "patch_far_1e6"])
def test_results_do_not_depend_on_the_grid_resolution(name, mvr, ctx):
    """seq_cell_points 4 (the default), 1, 64 and 4096 change the cell edge of every grid built afterwards (the cloud is uploaded
    again after each tune): the three checks above hold at each, and on the exact cases the keypoints are the reference's --
    hence the same at every resolution.  The f64 sums of the scatter run in walk order: identical saliency bits are not promised"""
    c, ref, base = gpu_run(name, False, mvr, ctx)
    try:
        for cp in (4, 1, 64, 4096):
            ctx.tune(seq_cell_points=cp)
            ctx.upload(8, c["p"])
            g = detect(ctx, c, 9, 8)
            g["points"] = ctx.download(9)
            check_counts(c, ref, g)
            check_saliency(c, ref, g, "%s seq_cell_points=%d" % (name, cp), False)
            check_suppression(c, ref, g)
            assert same_bits(g["salient_count"], base["salient_count"]) and same_bits(g["nms_count"], base["nms_count"]), (name, cp)
            if c["exact"]:
                assert np.array_equal(g["index"], ref["index"]) and same_bits(g["points"], base["points"]), (name, cp)
            print("%s seq_cell_points=%d: %d of %d saliencies differ in a bit from the default resolution's, %d keypoints"
                  % (name, cp, int((bits(g["saliency"]) != bits(base["saliency"])).sum()), len(g["saliency"]), len(g["index"])))
    finally:
        ctx.tune(seq_cell_points=4)


@pytest.mark.parametrize("name,fma", [r for r in RUNS if r[0] in IC.EXACT], ids=[i for i, r in zip(IDS, RUNS) if r[0] in IC.EXACT])
def test_keypoints_equal_the_references(name, fma, mvr, ctx):
    c, ref, g = gpu_run(name, fma, mvr, ctx)
    assert np.array_equal(g["saliency"] != 0, ref["salient"])
    assert np.array_equal(g["index"], ref["index"]) and len(ref["index"]) > 100
    out = c["p"][ref["index"].astype(np.int64)].copy()
    out[:, 3] = 1.0
    assert same_bits(g["points"], out)


def test_exact_copies_get_the_same_bits_and_the_same_flag(mvr, ctx):
    for fma in (False, True):
        c, ref, g = gpu_run("duplicates", fma, mvr, ctx)
        p = c["p"]
        flag = np.zeros(len(p), bool)
        flag[g["index"]] = True
        a, b = np.arange(3, len(p), 5)[:len(p[4::5])], np.arange(4, len(p), 5)
        twins = (p[a, :3] == p[b, :3]).all(1)
        assert twins.sum() >= 280
        assert np.array_equal(bits(g["saliency"][a[twins]]), bits(g["saliency"][b[twins]])) and np.array_equal(flag[a[twins]], flag[b[twins]])
        zero = np.nonzero((p[:, :3] == p[0, :3]).all(1))[0]
        assert len(zero) >= 11 and len(set(bits(g["saliency"][zero]).tolist())) == 1 and len(set(flag[zero].tolist())) == 1
        assert (g["saliency"][a[twins]] != 0).sum() > 200 and flag[a[twins]].sum() > 10      # kept twins: equal saliencies, both kept


def test_in_place_no_destination_and_normals(mvr, ctx):
    c, ref, g = gpu_run("box", False, mvr, ctx)
    nr = FC.box()[1]
    # dst == -1: the host arrays alone, no slot touched
    ctx.upload(2, c["p"])
    ctx.upload_normals(2, nr)
    ctx.upload(3, c["p"][:7])
    h = detect(ctx, c, -1, 2)
    assert all(same_bits(h[k], g[k]) for k in ("index", "saliency", "salient_count", "nms_count"))
    assert same_bits(ctx.download(2), c["p"]) and same_bits(ctx.download_normals(2), nr) and same_bits(ctx.download(3), c["p"][:7])
    assert ctx.iss_keypoints(-1, 2, **IC.params(c)) == len(g["index"])  # every host array NULL
    # into another slot: normals follow their points
    h = detect(ctx, c, 3, 2)
    assert same_bits(h["index"], g["index"]) and same_bits(ctx.download(3), g["points"])
    assert same_bits(ctx.download_normals(3), nr[g["index"].astype(np.int64)])
    # in place
    h = detect(ctx, c, 2, 2)
    assert same_bits(h["index"], g["index"]) and same_bits(h["saliency"], g["saliency"])
    assert same_bits(ctx.download(2), g["points"]) and same_bits(ctx.download_normals(2), nr[g["index"].astype(np.int64)])
    # the output is a new point set: it is searched as one
    n2 = ctx.iss_keypoints(2, 2, **IC.params(c))
    assert n2 == ctx.size(2) < len(g["index"])
    # a source without normals leaves none
    assert len(ctx.download_normals(1)) == 0


def test_two_runs_give_the_same_bits(mvr, ctx):
    for name, fma in (("view", False), ("duplicates", True), ("huge_coordinates", False)):
        c, ref, g = gpu_run(name, fma, mvr, ctx)
        ctx.upload(4, c["p"])
        h = detect(ctx, c, 5, 4, fma)
        assert all(same_bits(h[k], g[k]) for k in ("index", "saliency", "salient_count", "nms_count"))
        assert same_bits(ctx.download(5), g["points"])


def test_empty_and_refused(mvr, ctx):
    c = IC.case("tiny_0", mvr)
    ctx.upload(6, c["p"])
    ctx.upload(7, IC.case("tiny_5", mvr)["p"])
    assert ctx.iss_keypoints(7, 6, **IC.params(c)) == 0 and ctx.size(7) == 0      # an empty cloud: MVR_OK, an empty output
    with pytest.raises(mvr.MvrError):
        ctx.iss_keypoints(7, 6, 0.0, 1.0)
    with pytest.raises(mvr.MvrError):
        ctx.iss_keypoints(7, 6, 1.0, 1.0, min_neighbors=-1)
    # min_neighbors = 0 makes no point of an empty ball a keypoint: a lone point's scatter is all zero
    p5 = IC.case("tiny_5", mvr)
    ctx.upload(6, p5["p"])
    n, sal = ctx.iss_keypoints(-1, 6, p5["salient_radius"], p5["non_max_radius"], min_neighbors=0, return_saliency=True)
    assert n == 0 and (bits(sal) == 0).all()
