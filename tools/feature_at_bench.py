"""Timing of the descriptors at query points over a search surface (mvr_cloud_fpfh_at, mvr_cloud_pfh_at) on synthetic turntable
views, beside the existing whole-cloud calls (mvr_cloud_fpfh, mvr_cloud_pfh) on the same slot in the same process.  No ratio has a
bar; what the numbers are read for: a keypoint set must cost less than the whole cloud, every point through the _at entry must
cost what the whole-cloud call costs (within the spread reported here), and the descriptor phase of a coarse alignment on
keypoints must cost less than the whole-cloud descriptors it replaces.

Writes ONE JSON line to --out (default profiles/feature_at_bench.json) and prints it.  A time is milliseconds of a warm call with
every output NULL (the kernels, the synchronisations and the few bytes read back between them), measured with HIP events
(torch.cuda.Event on the stream the context enqueues on) around the call: [median, min, max] of --reps calls.
  <cloud> = 1x200k: one 200k view; 12x200k: the twelve views posed by their turntable prior and concatenated (2.4 M; PFH at
  5 mm on it only with --full); normals from radius 2.5 mm.
  <work>  = fpfh_r2.5, fpfh_r5, pfh_r2.5, pfh_r5, pfh_k16
  <set>   = iss: the cloud's ISS keypoints (salient / non-maximum radius 6 x / 4 x the measured point spacing, as
            tools/iss_bench.py); p1 / p10: a seeded random 1 % / 10 % of the points; all: every point, as an index list.
  <cloud>_<work>_full                 the existing call
  <cloud>_<work>_none                 the _at entry with indices NULL on the same slot: it forwards to the existing call
  <cloud>_<work>_<set>                the _at entry with that index list; <cloud>_<set>_queries / _share: its size
  <cloud>_<work>_<set>_nosort         the same with tune key at_sort = 0 (iss and p1)
  <cloud>_fpfh_r*_<set>_stages        [mark, select, spfh, weight] ms of one call with tune key at_clock = 1 (events on the stream
                                      between the stages), and _marked_share = SPFH rows computed / surface points
  align_*                             the recovery pair of tests/align_cases.py (a 60k view moved by 70 degrees, both voxel-
                                      downsampled at 4 mm, descriptors at 20 mm, ISS at 10 / 6 mm): the descriptor phase of a coarse
                                      alignment on keypoints, host tables out, wall ms: _full = the whole-cloud call on both clouds
                                      (what the alignment did before it computed at the keypoints), _at = the keypoints alone;
                                      _iss = the detector on both clouds, which either path runs; _align_fpfh / _align_pfh = the
                                      aligner (20 000 iterations) on the tables, NaN but for the keypoints' rows, which are the same
                                      bits from either path; _whole_* = detector + descriptors + aligner.  The _full flow is the
                                      parent's: its code is in this build unchanged, so both are timed in one process on one device
Usage: python tools/feature_at_bench.py [--reps 7] [--n 200000] [--views 12] [--full] [--out profiles/feature_at_bench.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_at_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    mvr = importlib.import_module("multi-view-registration_amd")
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = mvr.synth_params(a.views, 3)
    piv, ax = mvr.synth_prior(sp)
    views = [mvr.synth_view(sp, v, a.n) for v in range(a.views)]
    out = {"n": a.n, "views": a.views, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    def save():                                                  # after every section: a run cut short leaves what it measured
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")

    def timed(call, reps=None):
        call()                                                   # warm: code objects, arena, buffers, the slot's grid
        ev = []
        for _ in range(reps or a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        return [round(float(np.median(ev)), 4), round(float(min(ev)), 4), round(float(max(ev)), 4)]

    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        L, h = mvr._lib, ctx._h
        posed = []
        for v, p in enumerate(views):
            ctx.upload(2, p)
            ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(2))
        ctx.upload(0, views[0])                                  # slot 0: one view; slot 1: the merged object
        ctx.upload(1, np.concatenate(posed))
        for s in (0, 1):
            ctx.estimate_normals(s, radius=2.5)

        def full(slot, work):
            kind, radius, k = work
            if kind == "fpfh":
                p = mvr.FpfhParams(float(radius), 0)
                rc = L.mvr_cloud_fpfh(h, slot, C.byref(p), None, None, None)
            else:
                p = mvr.PfhParams(float(radius or 0.0), int(k or 0), 0)
                rc = L.mvr_cloud_pfh(h, slot, C.byref(p), None, None, None)
            assert rc == mvr.OK, rc

        def at(slot, work, idx):
            kind, radius, k = work
            ptr = idx.ctypes.data_as(C.POINTER(C.c_uint32)) if idx is not None else None
            n = len(idx) if idx is not None else 0
            if kind == "fpfh":
                p = mvr.FpfhParams(float(radius), 0)
                rc = L.mvr_cloud_fpfh_at(h, slot, ptr, n, slot, C.byref(p), None, None)
            else:
                p = mvr.PfhParams(float(radius or 0.0), int(k or 0), 0)
                rc = L.mvr_cloud_pfh_at(h, slot, ptr, n, slot, C.byref(p), None, None, None)
            assert rc == mvr.OK, rc

        WORK = [("fpfh_r2.5", ("fpfh", 2.5, None)), ("fpfh_r5", ("fpfh", 5.0, None)), ("pfh_r2.5", ("pfh", 2.5, None)),
                ("pfh_r5", ("pfh", 5.0, None)), ("pfh_k16", ("pfh", None, 16))]
        rng = np.random.default_rng(7)
        for slot, tag in ((0, "1x%dk" % (a.n // 1000)), (1, "%dx%dk" % (a.views, a.n // 1000))):
            n = ctx.size(slot)
            _, d2 = ctx.knn(slot, slot, 2)
            spacing = float(np.sqrt(np.median(d2[:, 1])))
            key = ctx.iss_keypoints(-1, slot, 6.0 * spacing, 4.0 * spacing, return_index=True)[1]
            sets = [("iss", np.ascontiguousarray(key, np.uint32)), ("p1", rng.permutation(n)[:n // 100].astype(np.uint32)),
                    ("p10", rng.permutation(n)[:n // 10].astype(np.uint32)), ("all", np.arange(n, dtype=np.uint32))]
            for sname, idx in sets:
                out["%s_%s_queries" % (tag, sname)] = int(len(idx))
                out["%s_%s_share" % (tag, sname)] = round(len(idx) / n, 5)
            for wname, work in WORK:
                if slot == 1 and wname == "pfh_r5" and not a.full:
                    continue
                nm = "%s_%s" % (tag, wname)
                t0 = time.perf_counter()
                full(slot, work)
                reps = 1 if time.perf_counter() - t0 > 5.0 else a.reps
                out[nm + "_full"] = timed(lambda: full(slot, work), reps)
                out[nm + "_none"] = timed(lambda: at(slot, work, None), reps)
                for sname, idx in sets:
                    out["%s_%s" % (nm, sname)] = timed(lambda: at(slot, work, idx), reps)
                    if sname in ("iss", "p1"):
                        ctx.tune(at_sort=0)
                        out["%s_%s_nosort" % (nm, sname)] = timed(lambda: at(slot, work, idx), reps)
                        ctx.tune(at_sort=1)
                    if work[0] == "fpfh":
                        ctx.tune(at_clock=1)
                        at(slot, work, idx)
                        ctx.tune(at_clock=0)
                        out["%s_%s_stages" % (nm, sname)] = [round(ctx.stat("fpfh_at_%s_ms" % s), 4) for s in ("mark", "select", "spfh", "weight")]
                        out["%s_%s_marked_share" % (nm, sname)] = round(ctx.stat("fpfh_at_marked") / n, 5)
                save()

        # the descriptor phase of a coarse alignment on keypoints
        import align_cases as AC
        s_raw, t_raw = AC.recovery_view(mvr)
        for slot, raw in ((3, s_raw), (4, t_raw)):
            ctx.upload(slot, raw)
            ctx.voxel_grid(slot, slot, AC.REC_LEAF)
            ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS)
        keys = {}

        def iss():
            for slot in (3, 4):
                keys[slot] = ctx.iss_keypoints(-1, slot, 10.0, 6.0, return_index=True)[1]

        def wall(call):
            call()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()                                           # (every call ends in a synchronise: the tables are on the host)
                ts.append((time.perf_counter() - t0) * 1e3)
            return [round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)]

        out["align_iss"] = wall(iss)
        out["align_points"] = [ctx.size(3), ctx.size(4)]
        out["align_keypoints"] = [int(len(keys[3])), int(len(keys[4]))]
        r = AC.REC_FPFH_RADIUS
        out["align_fpfh_full"] = wall(lambda: [ctx.fpfh(s, r) for s in (3, 4)])
        out["align_fpfh_at"] = wall(lambda: [ctx.fpfh_at(s, s, r, indices=keys[s]) for s in (3, 4)])
        out["align_pfh_full"] = wall(lambda: [ctx.pfh(s, radius=r) for s in (3, 4)])
        out["align_pfh_at"] = wall(lambda: [ctx.pfh_at(s, s, indices=keys[s], radius=r) for s in (3, 4)])
        for name, rows in (("fpfh", lambda s: ctx.fpfh_at(s, s, r, indices=keys[s])), ("pfh", lambda s: ctx.pfh_at(s, s, indices=keys[s], radius=r))):
            tabs = []
            for s in (3, 4):
                got = rows(s)
                m = np.full((ctx.size(s), got.shape[1]), np.nan, np.float32)
                m[keys[s]] = got
                tabs.append(m)
            out["align_align_" + name] = wall(lambda: ctx.align_prerejective(3, 4, tabs[0], tabs[1], **AC.REC_PARAMS))
            for flow in ("full", "at"):
                out["align_whole_%s_%s" % (name, flow)] = round(out["align_iss"][0] + out["align_%s_%s" % (name, flow)][0] + out["align_align_" + name][0], 4)
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
