"""Lean posing (tune key lean_pose, stat key lean_passes): a pass of the ring run that is queued ahead of its poses and whose
searches all walk the grid writes only the grid-ordered coordinates and the pose records of its posed copies; every kernel
of such a pass poses its own queries from the raw Hilbert-ordered copy.  Nothing of that may show: poses, edge tables and
every array a later call reads are the bytes lean_pose = 0 gives."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V, N, MAX_D = 12, 20000, 4.0


def _ring(mvr, n=N):
    sp = mvr.synth_params(V, 3)
    scans = [mvr.synth_view(sp, v, n) for v in range(V)]
    piv, ax = mvr.synth_prior(sp)
    poses0 = [np.eye(4)] + [mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, V)) for v in range(1, V)]
    return scans, poses0, np.array(sp.pivot), [(i, (i + 1) % V) for i in range(V)]


def _six_passes(mvr, scans, poses0, origin, edges, fma=False, **knobs):
    """six passes from the prior in one native call; (bytes of the results, passes posed lean, passes queued ahead)"""
    with mvr.Context(0) as ctx:
        ctx.tune(**knobs)
        for v in range(V):
            ctx.upload(V + v, scans[v])
        poses, info = ctx.ring_step(list(range(V)), [V + v for v in range(V)], edges, [p.copy() for p in poses0], MAX_D, origin,
                                    steps=6, fma=fma)
        posed = [ctx.download(v).tobytes() for v in range(V)]
        return (np.asarray(poses).tobytes(), info["rows"].tobytes(), posed), ctx.stat("lean_passes"), ctx.stat("piped_passes")


@pytest.mark.parametrize("knobs,fma", [(dict(), False), (dict(grid_stage=0), False), (dict(), True)],
                         ids=["default", "grid_stage=0", "fma"])
def test_lean_passes_give_the_same_bits(mvr, knobs, fma):
    scans, poses0, origin, edges = _ring(mvr)
    full, n_full, _ = _six_passes(mvr, scans, poses0, origin, edges, fma=fma, lean_pose=0, **knobs)
    lean, n_lean, piped = _six_passes(mvr, scans, poses0, origin, edges, fma=fma, lean_pose=1, **knobs)
    print("lean_passes %g of %g queued passes (lean_pose=0: %g)" % (n_lean, piped, n_full))
    assert n_full == 0
    assert n_lean > 0 and n_lean <= piped          # the comparison is not empty: passes WERE posed lean
    assert lean == full


@pytest.mark.parametrize("knobs", [dict(pipeline=0), dict(grid_sets=0), dict(cull_list=0)], ids=lambda k: ",".join("%s=%s" % kv for kv in k.items()))
def test_routes_that_read_the_posed_copy_are_never_lean(mvr, knobs):
    """not queued ahead, or the listed sets on the culled kernels: posed fully every pass -- no lean launch, so no flush either"""
    scans, poses0, origin, edges = _ring(mvr)
    full, n_full, _ = _six_passes(mvr, scans, poses0, origin, edges, lean_pose=0, **knobs)
    lean, n_lean, _ = _six_passes(mvr, scans, poses0, origin, edges, lean_pose=1, **knobs)
    assert n_full == 0 and n_lean == 0
    assert lean == full
    ref, _, _ = _six_passes(mvr, scans, poses0, origin, edges, lean_pose=0)
    assert lean[:2] == ref[:2]


def _after_a_ring_run(mvr, lean_pose, what):
    scans, poses0, origin, edges = _ring(mvr)
    out = []
    with mvr.Context(0) as ctx:
        ctx.tune(lean_pose=lean_pose)
        for v in range(V):
            ctx.upload(V + v, scans[v])
        poses, info = ctx.ring_step(list(range(V)), [V + v for v in range(V)], edges, [p.copy() for p in poses0], MAX_D, origin, steps=6)
        n_lean = ctx.stat("lean_passes")
        out.append(np.asarray(poses).tobytes())
        if what == "correspondences":
            out += [a.tobytes() for a in ctx.correspondences(0, 1, MAX_D)]
            out += [a.tobytes() for a in ctx.correspondences(5, 4, MAX_D, reciprocal=False)]
        elif what == "fitness":
            out.append(np.float64(ctx.fitness(2, 3, np.eye(4), max_range=MAX_D * MAX_D)).tobytes())
        elif what == "voxel_grid":
            n_out, vmap = ctx.voxel_grid(2 * V, 3, 2.0, return_map=True)
            out += [np.int64(n_out).tobytes(), vmap.tobytes(), ctx.download(2 * V).tobytes()]
        elif what == "estimate_normals":
            curv = ctx.estimate_normals([1, 2], k=10, curvature=True)
            out += [c.tobytes() for c in curv] + [ctx.download_normals(1).tobytes(), ctx.download_normals(2).tobytes()]
        elif what == "seq_run":
            T, S, O = 2 * V, 2 * V + 1, 2 * V + 2
            sposes, log = ctx.seq_run([V + v for v in range(V)], T, S, O, mvr.icp_params(max_dist=8.0, max_iter=20), poses0, repeat=1)
            out += [np.asarray(sposes).tobytes(), ctx.download(T).tobytes()] + [np.asarray(r["T"]).tobytes() for r in log]
        elif what == "restart":
            # the run goes on from poses that are 2 mm and more off what the seeds belong to (back at the prior, one view turned
            # a little further), twice: inside the call nothing is seeded where the keys say
            again = [p.copy() for p in poses0]
            again[3] = again[3] @ mvr.axis_rotation(np.zeros(3), np.array([0.0, 0.0, 1.0]), 0.01)
            for _ in range(2):
                p2, i2 = ctx.ring_step(list(range(V)), [V + v for v in range(V)], edges, [p.copy() for p in again], MAX_D, origin, steps=4)
                out += [np.asarray(p2).tobytes(), i2["rows"].tobytes()]
            assert ctx.stat("lean_passes") <= ctx.stat("piped_passes")
        out += [ctx.download(v).tobytes() for v in range(V)]          # every posed slot, after the call too
    return out, n_lean


@pytest.mark.parametrize("what", ["download", "correspondences", "fitness", "voxel_grid", "estimate_normals", "seq_run", "restart"])
def test_what_follows_a_lean_run_reads_current_arrays(mvr, what):
    """After a ring run with lean passes returns, every posed slot downloads as with lean_pose = 0, and so does whatever a one-pair
    search, a fitness score, a voxel grid, a normal estimation or a sequential run on the same context reads or writes next.
    "restart": the registration goes on from poses far from the seeds' (the prior again, one view turned further).  Which passes
    are lean is decided from what the host knows (same pairs as the pass before, grids valid, stragglers on the grid): such a
    restart pass keeps the grid route -- it launches no culled kernel -- and is lean like the others, so the test bounds the
    count by the queued passes instead of excluding it."""
    full, n_full = _after_a_ring_run(mvr, 0, what)
    lean, n_lean = _after_a_ring_run(mvr, 1, what)
    assert n_full == 0 and n_lean > 0
    assert len(lean) == len(full)
    for k, (a, b) in enumerate(zip(lean, full)):
        assert a == b, (what, k)
