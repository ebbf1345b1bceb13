"""Slot state on the GPU: one feature's output slot as the next feature's cached input (tests/slot_model.py).

One long-lived Context runs a sequence of public calls -- every entry that writes a slot, every entry that builds cached state
on one.  After EVERY step the checker (slot_model.Checker)
  * replays the call in a fresh Context that got the step's input slots from the model's host copies (points, normals, the
    segment table through set_global_base / append_range) and compares return values and every written slot bit for bit;
  * compares every slot the call did not write with the model, bit for bit;
  * searches the slots the step touched, and one it did not, on the long-lived context against the independent references: nn
    both ways and correspondences (both reciprocal settings) against the oracle, knn at k = 1 and 17 against
    normals_ref.knn_brute (the rule of tests/test_gpu_walk_fuzz.py), radius_outlier_removal with return_index into the filter
    destination against outlier_ref.radius, and the keys of nn_forward_keys against the model's global numbering.
A stale ordering, sorted copy, box, pose, grid, seed, pair record or segment table shows as a wrong neighbour in the step that
left it stale; that this checker notices one is proven on the CPU (tests/test_slot_model_host.py).

The named scenarios (the coverage matrix: every kind of cached state x every mutator x destination / source, and the
hand-written ones) run with the culled searches and again with nn_mode = 0; the seeded random sequences with the culled ones.
Every entry is bit-reproducible across contexts (slot_model.NOT_BIT_REPRODUCIBLE is empty) once the clean room gives a slot the
ORDERING it has on the long-lived context: f64 sums (the moment rows, GICP's objective, an iteration's residual) are added in the
order of the source set's Hilbert ordering, and a posed copy inherits the ordering of the cloud it was posed from, built from
that cloud's coordinates.  The clean room rebuilds it that way (slot_model.Slot.recipe).  A return value's wall time and
evaluation count (slot_model.VOLATILE) are not results.

Measured on an MI355X: a named scenario takes 0.2 s (median; 0.5 s at most), a random sequence 0.7 to 1.7 s, the file 30 s
with the first import of torch; a fresh context costs about 1 ms, the clean rooms a tenth of a sequence's time.

Found by the shard scenarios: the output slot of an align kept the segment table of the shard it had been (DESIGN.md section 22;
fixed by finish_align_out in csrc/mvr_align.hip)."""
import importlib
import time

import numpy as np
import pytest

import slot_model as M
from conftest import PKG

pytestmark = pytest.mark.gpu

SCENARIOS = M.named_scenarios()
_stop = []                                     # a HIP error ends the file's run: nothing more is started on the GPU after it


@pytest.fixture(scope="module")
def mvr(built):
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def env(mvr, orc):
    return M.Env(mvr, orc)


def export_keys(ctx, s, t):
    """nn_forward_keys of slot s in slot t, through a torch device buffer as tests/test_gpu_seq.py holds it"""
    import torch
    n = ctx.size(s)
    buf = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    ctx.nn_forward_keys(s, t, 1e9, buf.data_ptr())
    ctx.sync()
    return buf.cpu().numpy()[:n]


class GpuChecker(M.Checker):
    grid_launches = None

    def finish(self, ctx):
        ctx.prof_enable(False)
        self.grid_launches = ctx.prof_get(self.env.mvr.K_NN_GRID)[0]


def checker(mvr, env, mode, **kw):
    def make(clean=False):
        ctx = mvr.Context(0)
        if mode == "brute":
            ctx.tune(nn_mode=0)
        if not clean:
            ctx.prof_reset()
            ctx.prof_enable(1)
        return ctx
    return GpuChecker(make, env, export_keys=export_keys, **kw)


def guarded(mvr, what, run):
    if _stop:
        pytest.fail("not run: %s ended in a HIP error, and nothing more is started on the GPU after one" % _stop[0])
    t0 = time.perf_counter()
    try:
        c = run()
    except mvr.MvrError as e:
        if e.status == mvr.E_HIP:
            _stop.append(what)
        raise
    print("[slot-state] %s: %.2f s, %.2f s of it in the clean rooms, %d steps" % (what, time.perf_counter() - t0, c.t_clean, len(c.seq)))
    return c


@pytest.mark.parametrize("name", sorted(SCENARIOS))
@pytest.mark.parametrize("mode", ["culled", "brute"])
def test_named_scenario(mvr, env, mode, name):
    seq = SCENARIOS[name]
    c = guarded(mvr, "%s-%s" % (mode, name), lambda: checker(mvr, env, mode).run(seq))
    # ... and the scenario did what it was built for
    aligns = [a for n, a in seq if n in M.ALIGNS]
    assert len(c.align_iterations) == len(aligns)
    if name == "dst-icp_align":                   # the reference's settings end in one iteration; with the criteria off the source moves (the scratch cloud)
        assert c.align_iterations[:2] == [1, 1] and c.align_iterations[2] >= 2, c.align_iterations
    if name == "posed-scan-align":
        assert c.align_iterations[0] == 1 and c.align_iterations[1] >= 2, c.align_iterations
    if name in M.POSED_SCAN:                      # the posed scans were searched over their grids where grids are used at all
        assert (c.grid_launches > 0) == (mode == "culled"), (name, mode, c.grid_launches)
    if name == "extend-1025+700":
        # mvr_cloud_append extended the ordering in place (extend_point_set): it is there right after the append, without a
        # search, and its head is the old ordering -- 1 025 is no multiple of the tile, so the last old tile is refreshed
        (k1, before1, after1), (k2, before2, after2) = c.order_log
        if mode == "culled":
            assert before1 is not None and len(before1) == 1025 and after1 is not None and len(after1) == 1725
            assert np.array_equal(after1[:1025], before1) and np.array_equal(np.sort(after1), np.arange(1725))
            assert before2 is not None and after2 is not None and len(after2) == 1982 and np.array_equal(after2[:1725], before2)
        else:
            assert after1 is None and after2 is None
    if name == "append-shared-ordering":          # the ordering is shared with a copy: the append must not extend it
        (k1, before1, after1), = c.order_log
        assert after1 is None and (before1 is not None) == (mode == "culled")
    if name.startswith("shard-"):
        assert c.model[M.X].segs == [] and c.model[M.Y].segs == [(0, 3000, 123456)] and c.model[M.S].segs == [(0, 3000, 123456)]


@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_sequence(mvr, env, seed):
    c = guarded(mvr, "random-%d" % seed, lambda: checker(mvr, env, "culled").run_random(seed))
    assert len(c.seq) == len(M.RANDOM_PROLOGUE) + M.RANDOM_STEPS
    print("[slot-state] random-%d ran %s" % (seed, " ".join(n for n, _ in c.seq[len(M.RANDOM_PROLOGUE):])))


@pytest.mark.parametrize("name", ["extend-1025+700", "append-pairs", "append-shared-ordering", "posed-scan-align", "posed-scan-ring", "shrunk-by-a-filter",
                                  "target-shrinks-between-aligns", "upload-sizes", "dst-append", "src-append", "dst-icp_align", "src-icp_align_rejected",
                                  "dst-voxel_grid", "dst-transform_batch"])
def test_named_scenario_without_the_checkers_searches(mvr, env, name):
    """the same sequences with no search after the steps: a mutator then meets slots that have no ordering yet, or an ordering
    but no sorted copy, boxes or model grid (append's extension with a source that was never searched); every slot is searched
    after the last step, and the clean rooms compare every step as before"""
    guarded(mvr, "bare-%s" % name, lambda: checker(mvr, env, "culled", searches=False).run(SCENARIOS[name]))
