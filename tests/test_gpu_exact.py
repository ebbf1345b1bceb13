"""GPU tests that close the exactness gaps of the grid search named by the round-2 review: the posed and the canonical
frame far apart, the grid path against the ORACLE's correspondence lists on every edge, and slot state that an in-place
align must invalidate (registrator.cpp:920's aliased align(*source_)).  Bar: bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ring(mvr, V, N):
    sp = mvr.synth_params(V, 3)
    scans = [mvr.synth_view(sp, v, N) for v in range(V)]
    piv, ax = mvr.synth_prior(sp)
    poses0 = [np.eye(4)] + [mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, V)) for v in range(1, V)]
    return sp, scans, poses0, np.array(sp.pivot), [(i, (i + 1) % V) for i in range(V)]


def _shift(d):
    T = np.eye(4)
    T[:3, 3] = d
    return T


@pytest.mark.parametrize("case", ["raw_far_1e5", "raw_far_1e6", "posed_far_1e5", "posed_far_1e6", "both_far"])
def test_grid_search_with_the_two_frames_far_apart(mvr, case):
    """The cell arithmetic of the grid search runs in the target's CANONICAL (upload) frame, the distances in the POSED
    frame.  Raw scans kept 1e5 .. 1e6 mm from the origin (ulp 8e-3 .. 6e-2 mm) with poses that bring them next to it, and
    the converse, and both far: ring_search 1 == ring_search 0, bit for bit, over five passes.  (The ball's margin once
    scaled with the posed coordinates only: ADVICE r2.)"""
    V, N, max_d = 8, 12000, 4.0
    sp, scans, poses0, origin, edges = _ring(mvr, V, N)
    far = {"raw_far_1e5": 1.0e5, "raw_far_1e6": 1.0e6, "posed_far_1e5": 1.0e5, "posed_far_1e6": 1.0e6, "both_far": 3.0e5}[case]
    D = np.array([0.61, -0.52, 0.6]) * far
    if case.startswith("raw_far"):
        raw = [(s + np.array([*D, 0.0], np.float32)).astype(np.float32) for s in scans]          # canonical frame far away ...
        poses = [p @ _shift(-D) for p in poses0]                                                  # ... posed frame as usual
        org = origin
    elif case.startswith("posed_far"):
        raw = scans
        poses = [_shift(D) @ p for p in poses0]
        org = origin + D
    else:
        raw = [(s + np.array([*D, 0.0], np.float32)).astype(np.float32) for s in scans]
        poses = [_shift(-2.0 * D) @ p @ _shift(-D) for p in poses0]                                 # both far, on opposite sides
        org = origin - 2.0 * D
    for s in raw:
        s[:, 3] = 1.0
    runs = []
    for mode in (0, 1):
        with mvr.Context(0) as ctx:
            ctx.tune(ring_search=mode)
            for v in range(V):
                ctx.upload(V + v, raw[v])
            P, log = [p.copy() for p in poses], []
            ctx.prof_reset(); ctx.prof_enable(1)
            for _ in range(5):
                P, info = ctx.ring_step(list(range(V)), [V + v for v in range(V)], edges, P, max_d, org)
                log.append((np.asarray(P).tobytes(), info["rows"].tobytes()))
            ctx.prof_enable(False)
            assert (ctx.prof_get(mvr.K_NN_GRID)[0] > 0) == (mode == 1)          # the grid kernels did run in mode 1
            assert sum(info["pair_n"]) > 1000, (case, info["pair_n"])
            runs.append(log)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a == b, (case, k)


def test_grid_path_equals_the_oracle_lists_on_every_edge(mvr, orc):
    """Not only grid == culled: the (query, match, d2) lists the fused pass leaves behind -- read back from its keys by
    mvr_pair_batch_correspondences -- equal the oracle's determineReciprocalCorrespondences on EVERY edge of the 12 x 20k
    ring, in an unseeded pass (culled kernel), the first seeded pass and a well seeded one (grid walk + stragglers)."""
    V, N, max_d = 12, 20000, 4.0
    sp, scans, poses0, origin, edges = _ring(mvr, V, N)
    with mvr.Context(0) as ctx:
        for v in range(V):
            ctx.upload(V + v, scans[v])
        P = [p.copy() for p in poses0]
        ctx.prof_reset(); ctx.prof_enable(1)
        for it in range(4):
            P_in = [np.array(p) for p in P]
            P, info = ctx.ring_step(list(range(V)), [V + v for v in range(V)], edges, P, max_d, origin)
            if it == 2:
                continue                                  # (three of the four passes are enough oracle time)
            clouds = [orc.transform_f64(P_in[v], scans[v]) for v in range(V)]
            for e, (s, t) in enumerate(edges):
                cc = orc.correspondences(clouds[s], clouds[t], max_d, kdtree=True)
                q, m, d = ctx.pair_batch_correspondences(e, N)
                assert len(q) == len(cc) == int(info["rows"][e, 0]), (it, e, len(q), len(cc))
                assert np.array_equal(q, cc["query"]) and np.array_equal(m, cc["match"]), (it, e)
                assert np.array_equal(d.view(np.uint32), cc["dist2"].view(np.uint32)), (it, e)
        ctx.prof_enable(False)
        assert ctx.prof_get(mvr.K_NN_GRID)[0] > 0 and ctx.prof_get(mvr.K_NN_WIDE)[0] > 0


def test_batch_correspondences_refuse_a_stale_pair(mvr):
    V, N = 4, 3000
    sp, scans, poses0, origin, edges = _ring(mvr, V, N)
    with mvr.Context(0) as ctx:
        for v in range(V):
            ctx.upload(V + v, scans[v])
        with pytest.raises(mvr.MvrError):
            ctx.pair_batch_correspondences(0, N)            # no batch yet
        ctx.ring_step(list(range(V)), [V + v for v in range(V)], edges, poses0, 4.0, origin)
        q, m, d = ctx.pair_batch_correspondences(1, N)
        assert len(q) > 100 and np.all(np.diff(q) > 0)
        with pytest.raises(mvr.MvrError):
            ctx.pair_batch_correspondences(V, N)            # no such pair
        ctx.upload(1, scans[1])                             # the source of pair 1 is another point set now
        with pytest.raises(mvr.MvrError):
            ctx.pair_batch_correspondences(1, N)


@pytest.mark.parametrize("how", ["align_in_place", "transform_in_place", "append"])
def test_slot_state_after_in_place_changes_between_passes(mvr, how):
    """mvr_icp_align with out == src (the aliased align(*source_) of registrator.cpp:920) rewrote a posed
    slot's points but left its pose / grid bookkeeping in place; the next fused pass then re-derived the grid-ordered
    coordinates from the stale pose and searched the wrong points.  Ring passes, an in-place change of a posed slot,
    then a batch over the slots AS THEY ARE: ring_search 1 == ring_search 0, and equal to one-pair calls."""
    V, N, max_d = 6, 9000, 4.0
    sp, scans, poses0, origin, edges = _ring(mvr, V, N)
    runs = []
    for mode in (0, 1):
        with mvr.Context(0) as ctx:
            ctx.tune(ring_search=mode)
            for v in range(V):
                ctx.upload(V + v, scans[v])
            P = [p.copy() for p in poses0]
            for _ in range(3):
                P, info = ctx.ring_step(list(range(V)), [V + v for v in range(V)], edges, P, max_d, origin)
            if how == "align_in_place":
                T, st, rc = ctx.icp_align(3, 4, 3, mvr.icp_params(max_dist=max_d, max_iter=3, teps=0.0, feps=-1e300))
                assert rc == 0 and st["iterations"] >= 1 and np.abs(T - np.eye(4)).max() > 1e-7
                ctx.copy(2 * V + 1, 3)                      # a copy of the moved slot: must not inherit a stale pose either
            elif how == "transform_in_place":
                ctx.transform(3, 3, mvr.axis_rotation(np.array(sp.pivot), np.array(sp.axis), 3e-3))
            else:
                ctx.append(3, 2)                            # slot 3 grows by slot 2's points: another point set
            rows = ctx.pair_moments2_batch(edges, max_d, origin)
            single = [ctx.pair_moments2(s, t, max_d, origin) for s, t in edges]
            for k, (a, b) in enumerate(zip(single, rows)):
                assert bytes(a) == bytes(b), (how, mode, k)
            # ... and the passes after it (seeded by that batch)
            rows2 = ctx.pair_moments2_batch(edges, max_d, origin)
            runs.append(b"".join(bytes(r) for r in rows) + b"".join(bytes(r) for r in rows2))
            assert sum(r.n for r in rows) > 1000
    assert runs[0] == runs[1], how


def _sequential(mvr, ctx, scans, poses0, params, repeat, V, hook=None):
    """the sequential driver (registrator.cpp:526-588) over the C-ABI: view 0 posed, then 1, V-1, 2, ... each aligned to
    the growing model and appended"""
    RAW, TARGET, SOURCE, OUT = 16, 0, 1, 2
    order = []
    for i in range(1, V // 2):
        order += [i, V - i]
    order.append(V // 2)
    poses, log = [p.copy() for p in poses0], []
    for r in range(repeat):
        ctx.transform(TARGET, RAW + 0, poses[0])
        ctx.reserve(TARGET, sum(len(s) for s in scans))
        for k, v in enumerate(order):
            ctx.transform(SOURCE, RAW + v, poses[v])
            T, st, rc = ctx.icp_align(SOURCE, TARGET, OUT, params)
            poses[v] = mvr.mat4d_mul(T.astype(np.float64), poses[v])
            if hook:
                hook(ctx, r, k)
            ctx.append(TARGET, OUT)
            log.append((v, st["n_corr"], st["iterations"], st["state"], st["mse"], T.tobytes()))
    return poses, log, ctx.download(TARGET)


@pytest.mark.parametrize("case", ["reference_settings", "two_sweeps", "three_iterations", "ragged_sizes", "wide_radius"])
def test_sequential_align_over_the_source_grid_equals_the_culled_search(mvr, orc, case):
    """mvr_icp_align of a posed scan against the growing model of the sequential mode: with the reverse searches walking the
    source scan's cell grid (seq_search 1, the default) the same transformations, counts, residuals and merged cloud, bit for
    bit, as with the culled kernel both ways (seq_search 0) -- with the reference's settings, over two sweeps (the grids are
    reused, the model is rebuilt), with aligns that iterate (only their first iteration can use the grid), with scans of
    different sizes and with a radius ten times as wide (wide balls leave the thread-per-query walk).  The forward
    searches' seeds, the iteration row's two ways to the host and the native driver change nothing either.  The tune keys of
    the forward searches that were removed (seq_search 2 and 3 and their knobs; the ring walk's grid_lanes, seed_delta_um and
    rim_cert_um; grid_index 0, the round-3 grid build) are refused, grid_index 1 and 2 accepted.  The first align's
    correspondences equal the oracle's."""
    V, N, max_d = 8, 9000, 4.0
    sp = mvr.synth_params(V, 3)
    sizes = [N] * V if case != "ragged_sizes" else [N - 613 * v for v in range(V)]
    scans = [mvr.synth_view(sp, v, sizes[v]) for v in range(V)]
    piv, ax = mvr.synth_prior(sp)
    poses0 = [np.eye(4)] + [mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, V)) for v in range(1, V)]
    kw = dict(max_dist=max_d, max_iter=1000)
    if case == "three_iterations":
        kw = dict(max_dist=max_d, max_iter=3, teps=0.0, feps=-1e300)
    if case == "wide_radius":
        kw = dict(max_dist=40.0, max_iter=1000)
    params = mvr.icp_params(**kw)
    runs = []
    for mode in (0, 1):  # culled both ways; reverse over the source's grid (default)
        with mvr.Context(0) as ctx:
            ctx.tune(seq_search=mode)
            for v in range(V):
                ctx.upload(16 + v, scans[v])
            ctx.prof_reset(); ctx.prof_enable(1)
            poses, log, merged = _sequential(mvr, ctx, scans, poses0, params, 2 if case == "two_sweeps" else 1, V)
            ctx.prof_enable(False)
            assert (ctx.prof_get(mvr.K_NN_GRID)[0] > 0) == (mode >= 1), (case, mode)
            runs.append((np.asarray(poses).tobytes(), log, merged.tobytes()))
    for r in runs[1:]:
        assert runs[0][1] == r[1], case
        assert runs[0][0] == r[0] and runs[0][2] == r[2], case
    # ... the same without the seeds one align of a scan leaves for the next (seq_seed: the forward searches of a sweep start from
    # the matches of the sweep before) -- three sweeps, so that seeds left by seeded searches are used as well
    seeded = []
    # (last arm: the iteration's row fetched by a copy and a synchronise instead of stored to the host by the sums launch itself, align_spin 0)
    for seed, mode, spin in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with mvr.Context(0) as ctx:
            ctx.tune(seq_seed=seed, seq_search=mode, align_spin=spin, lazy_super=spin)
            for v in range(V):
                ctx.upload(16 + v, scans[v])
            poses, log, merged = _sequential(mvr, ctx, scans, poses0, params, 3, V)
            seeded.append((np.asarray(poses).tobytes(), log, merged.tobytes()))
    for r in seeded[1:]:
        assert seeded[0][1] == r[1], case
        assert seeded[0][0] == r[0] and seeded[0][2] == r[2], case
    # ... and the native driver of the same loop (mvr_seq_run: one call for the three sweeps), with and without the model's tail
    # refreshed by the launch that poses the next source (seq_rider)
    for rider in (0, 1):
        with mvr.Context(0) as ctx:
            ctx.tune(seq_rider=rider)
            for v in range(V):
                ctx.upload(16 + v, scans[v])
            nposes, nlog = ctx.seq_run([16 + v for v in range(V)], 0, 1, 2, params, poses0, repeat=3)
            nmerged = ctx.download(0)
        assert np.asarray(nposes).tobytes() == seeded[0][0] and nmerged.tobytes() == seeded[0][2], (case, rider)
    assert [(e["view"], e["n_corr"], e["iterations"], e["state"], e["mse"], np.asarray(e["T"], np.float32).tobytes()) for e in nlog] == \
           [(l[0], l[1], l[2], l[3], l[4], l[5]) for l in seeded[0][1]], case
    # ... and against the oracle: the first align's correspondences, one by one
    with mvr.Context(0) as ctx:
        for gone in (dict(seq_search=2), dict(seq_search=3), dict(seq_model_tail=0), dict(parts_lanes=4), dict(parts_max_rows=8),
                     dict(grid_lanes=4), dict(seed_delta_um=50), dict(rim_cert_um=200), dict(grid_index=0)):
            with pytest.raises(mvr.MvrError) as refused:
                ctx.tune(**gone)
            assert refused.value.status == mvr.E_ARG, gone
        for kept in (1, 2):      # (the two forms of the cell-start table that remain; 2 is the default)
            ctx.tune(grid_index=kept)
        for v in range(V):
            ctx.upload(16 + v, scans[v])
        ctx.transform(0, 16, poses0[0]); ctx.transform(1, 17, poses0[1])
        T, st, rc = ctx.icp_align(1, 0, 2, params)
    a, b = orc.transform_f64(poses0[1], scans[1]), orc.transform_f64(poses0[0], scans[0])
    cc = orc.correspondences(a, b, kw["max_dist"], kdtree=True)
    if case != "three_iterations":
        assert st["n_corr"] == len(cc), (case, st["n_corr"], len(cc))
