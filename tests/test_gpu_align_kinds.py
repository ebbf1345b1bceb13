"""The kinds of align share one scratch cloud (ICP's input_transformed: CurSource in csrc/mvr_align.hip): the current
source moves into it in the second iteration, with its normals where the kind moves them.  Nothing one align leaves there may
reach the next: on ONE context the sequence plain, rejected (distance + surface-normal chain), GICP, point-to-plane, sharded
(a world of one), plain again -- in that order and reversed, into a third slot and in place (on a copy of the source) -- must
give, call by call, what the same call gives on a fresh context: T, iterations, state, n_corr, mse, the output points, and the
output normals where the kind writes them, bit for bit.  A second sequence puts a source WITHOUT normals between two aligns that
moved normals through the scratch cloud (the rejected align moves them only if the source has them).

The clouds are two 3 000-point synthetic views with estimated normals, the source a little off its prior; the criteria are set so
that every kind runs at least 3 iterations (asserted), or the scratch cloud would not be used at all.  No tolerance: equality."""
import importlib

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

N = 3000
MAX_D = 8.0
SRC, TGT, OUT, WORK, BARE = 0, 1, 2, 3, 4      # BARE: the source's points without normals, in reverse order
KINDS = ["plain", "rejected", "gicp", "p2plane", "sharded", "plain"]


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def scene(mvr):
    """(source points, source normals, target points, target normals): view 1 under its prior and a small extra motion, view 0"""
    sp = mvr.synth_params(n_views=12, config_id=1)
    piv, ax = mvr.synth_prior(sp)
    prior = mvr.axis_rotation(piv, ax, mvr.turntable_angle(1, 12))
    off = np.array(mvr.axis_rotation(piv, ax, np.deg2rad(0.4)))
    off[:3, 3] += (0.6, -0.4, 0.5)
    with mvr.Context(0) as ctx:
        ctx.upload(TGT, mvr.synth_view(sp, 0, N))
        ctx.upload(SRC, mvr.synth_view(sp, 1, N))
        ctx.transform(SRC, SRC, mvr.mat4d_mul(off, prior))
        ctx.estimate_normals([SRC, TGT], k=12)
        return ctx.download(SRC), ctx.download_normals(SRC), ctx.download(TGT), ctx.download_normals(TGT)


def fresh(mvr, scene, mode):
    s, sn, t, tn = scene
    ctx = mvr.Context(0)
    ctx.tune(nn_mode=0 if mode == "brute" else 1)
    ctx.upload(SRC, s); ctx.upload_normals(SRC, sn)
    ctx.upload(TGT, t); ctx.upload_normals(TGT, tn)
    ctx.upload(BARE, s[::-1])                     # (back to front: an ordering left over from SRC would be a wrong one)
    return ctx


def run(mvr, ctx, kind, in_place, src=SRC):
    """one align of `src` against TGT -> everything it returns and writes, as bit patterns"""
    bare = src == BARE
    if in_place:                                  # (the slot an align in place moved is no source for the next one)
        ctx.copy(WORK, src)
        src = out = WORK
    else:
        out = OUT
    icp = dict(max_dist=MAX_D, max_iter=4, teps=1e-12, feps=-1e300)
    gp = mvr.gicp_params(max_corr_dist=MAX_D, max_iterations=3, transformation_epsilon=1e-12, rotation_epsilon=1e-12)
    if kind == "plain":
        T, st, rc = ctx.icp_align(src, TGT, out, mvr.icp_params(**icp))
    elif kind == "p2plane":
        T, st, rc = ctx.icp_align(src, TGT, out, mvr.icp_params(point_to_plane=True, **icp))
    elif kind == "rejected":
        T, st, rc = ctx.icp_align_rejected(src, TGT, out, mvr.icp_params(**icp), [mvr.rejector("distance", 6.0), mvr.rejector("surface_normal", 0.5)])
    elif kind == "rejected_bare":                 # (no surface-normal stage: the source has no normals)
        T, st, rc = ctx.icp_align_rejected(src, TGT, out, mvr.icp_params(**icp), [mvr.rejector("distance", 6.0)])
    elif kind == "gicp":
        T, st, rc = ctx.icp_align_gicp(src, TGT, out, gp, [mvr.rejector("distance", 6.0)])
    else:
        assert kind == "sharded"
        T, st, rc = ctx.seq_align_sharded(src, TGT, out, mvr.icp_params(**icp), (0.0, 0.0, 900.0))
    assert rc == 0 and st["iterations"] >= 3, (kind, rc, st)
    got = dict(T=T.view(np.uint32).copy(), iterations=st["iterations"], state=st["state"], n_corr=st["n_corr"],
               mse=np.float64(st["mse"]).view(np.uint64), points=ctx.download(out).view(np.uint32))
    if kind != "sharded" and not bare:            # (every other kind rotates the source's normals into the output)
        got["normals"] = ctx.download_normals(out).view(np.uint32)
        assert len(got["normals"]) == N
    return got


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


@pytest.fixture(scope="module")
def reference(mvr, scene):
    """every call on a context of its own, once"""
    ref = {}
    for mode in ("culled", "brute"):
        for in_place in (False, True):
            for kind, src in [(k, SRC) for k in set(KINDS)] + [("plain", BARE), ("rejected_bare", BARE)]:
                with fresh(mvr, scene, mode) as ctx:
                    ref[mode, in_place, kind, src] = run(mvr, ctx, kind, in_place, src)
    return ref


@pytest.mark.parametrize("mode", ["culled", "brute"])
@pytest.mark.parametrize("in_place", [False, True], ids=["third-slot", "in-place"])
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_every_kind_after_every_other(mvr, scene, reference, mode, in_place, order):
    with fresh(mvr, scene, mode) as ctx:
        for k, kind in enumerate(KINDS if order == "forward" else KINDS[::-1]):
            same(run(mvr, ctx, kind, in_place), reference[mode, in_place, kind, SRC], "call %d: %s" % (k, kind))


@pytest.mark.parametrize("mode", ["culled", "brute"])
@pytest.mark.parametrize("in_place", [False, True], ids=["third-slot", "in-place"])
def test_source_without_normals_between_two_with(mvr, scene, reference, mode, in_place):
    seq = [("rejected", SRC), ("rejected_bare", BARE), ("gicp", SRC), ("plain", BARE), ("rejected", SRC), ("rejected_bare", BARE), ("p2plane", SRC)]
    with fresh(mvr, scene, mode) as ctx:
        for k, (kind, src) in enumerate(seq):
            same(run(mvr, ctx, kind, in_place, src), reference[mode, in_place, kind, src], "call %d: %s" % (k, kind))
