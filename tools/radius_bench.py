"""Timing of the radius search (mvr_radius_search) on synthetic turntable views, beside what walks the same ball without lists
(mvr_cloud_radius_outlier_removal with counts, radius-mode mvr_cloud_estimate_normals) and beside mvr_knn at the same k for the
capped rows, all on the same slots in the same process.  Nothing here has a bar.

Writes ONE JSON line to --out (default profiles/radius_bench.json) and prints it.  Milliseconds are the median of --reps warm calls
(the first call, which builds the slot's grid and grows the buffers, is not counted).  Per workload <w> = 1x200k_r2.5, 1x200k_r5
(one 200k view against itself) and 12x200k_r2.5 (the twelve views posed by their turntable prior and concatenated, 2.4 M):
  <w>_rows / _entries / _mean_row / _max_row / _long_rows    the result's shape
  <w>_count                      the count-only call (offsets and total to the host), wall
  <w>_sorted / <w>_unsorted      the whole call as Context.radius_search's second half makes it (lists to pageable host arrays),
                                 wall; *_device = the library's own phase clocks count + fill (the offsets' copy inside, those of idx / d2 not),
                                 *_copy the copies of idx / d2 home
  <w>_sorted_mrows_per_s / _mentries_per_s                   from *_device
  <w>_max16 / _max64             max_nn = 16 / 64, *_device likewise;  <w>_knn16 / _knn64: mvr_knn at that k, wall (its lists
                                 go home too: n * k * 8 bytes)
  <w>_ror_counts                 radius_outlier_removal(min_neighbors = 1, return_counts): the same walk, no lists
  <w>_normals                    estimate_normals(radius): the same walk, a covariance per point
A workload whose total exceeds MVR_RADIUS_MAX_TOTAL records "<w>_refused" and its count alone.
Usage: python tools/radius_bench.py [--reps 5] [--n 200000] [--views 12] [--out profiles/radius_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radius_bench.json"))
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

    def timed(call, reps, stats=()):
        call()                                                   # warm: code objects, arena, buffers, the slot's grid
        wall, st = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            st.append([ctx.stat(s) for s in stats])
        med = lambda v: round(float(np.median(v)), 4)
        return (med(wall),) + tuple(med([r[i] for r in st]) for i in range(len(stats)))

    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        posed = []
        for v, p in enumerate(views):
            ctx.upload(2, p)
            ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(2))
        ctx.upload(0, views[0])                                  # slot 0: one view; slot 1: the merged object
        ctx.upload(1, np.concatenate(posed))
        del posed

        def workload(tag, slot, radius):
            w = "%s_r%g" % (tag, radius)
            n = ctx.size(slot)
            offsets, total = ctx.radius_search(slot, slot, radius, count_only=True)
            lens = np.diff(offsets.astype(np.int64))
            out[w + "_rows"], out[w + "_entries"] = int(n), int(total)
            out[w + "_mean_row"], out[w + "_max_row"] = round(float(lens.mean()), 2), int(lens.max())
            out[w + "_long_rows"] = int(ctx.stat("radius_long_rows"))
            out[w + "_count"] = timed(lambda: ctx.radius_search(slot, slot, radius, count_only=True), a.reps)[0]
            out[w + "_ror_counts"] = timed(lambda: ctx.radius_outlier_removal(3, slot, radius, 1, return_counts=True), a.reps)[0]
            out[w + "_normals"] = timed(lambda: ctx.estimate_normals(slot, radius=radius), a.reps)[0]
            save()
            idx, d2 = np.empty(max(total, 1), np.uint32), np.empty(max(total, 1), np.float32)
            tot = C.c_size_t(0)

            def full(max_nn, sorted_):
                p = mvr.RadiusParams(float(radius), int(max_nn), int(sorted_), 0)
                rc = mvr._lib.mvr_radius_search(ctx._h, slot, slot, C.byref(p), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                idx.ctypes.data_as(C.POINTER(C.c_uint32)), d2.ctypes.data_as(C.POINTER(C.c_float)), len(idx), C.byref(tot))
                return rc

            if total > mvr.RADIUS_MAX_TOTAL:
                out[w + "_refused"] = True
                assert full(0, 1) == mvr.E_ARG
            else:
                phases = ("radius_count_ms", "radius_fill_ms", "radius_copy_ms")
                for name, max_nn, sorted_ in (("sorted", 0, 1), ("unsorted", 0, 0)):
                    t = timed(lambda: full(max_nn, sorted_), a.reps, phases)
                    out[w + "_" + name], out[w + "_%s_device" % name], out[w + "_%s_copy" % name] = t[0], round(t[1] + t[2], 4), t[3]
                    out[w + "_%s_fill" % name] = t[2]
                dev = out[w + "_sorted_device"] * 1e-3
                out[w + "_sorted_mrows_per_s"], out[w + "_sorted_mentries_per_s"] = round(n / dev / 1e6, 3), round(total / dev / 1e6, 2)
                save()
            for k in (16, 64):
                t = timed(lambda: full(k, 1), a.reps, ("radius_count_ms", "radius_fill_ms", "radius_copy_ms"))
                out[w + "_max%d" % k], out[w + "_max%d_device" % k], out[w + "_max%d_entries" % k] = t[0], round(t[1] + t[2], 4), int(tot.value)
                out[w + "_knn%d" % k] = timed(lambda: ctx.knn(slot, slot, k), a.reps)[0]
            save()

        tag1, tagm = "1x%dk" % (a.n // 1000), "%dx%dk" % (a.views, a.n // 1000)
        workload(tag1, 0, 2.5)
        workload(tag1, 0, 5.0)
        workload(tagm, 1, 2.5)                                   # the long one last
        out["complete"] = True
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
