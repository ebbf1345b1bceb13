"""Timing of the moving-least-squares smoothing (mvr_cloud_mls) on synthetic turntable views, beside the radius-mode normal
estimation at the same radius on the same cloud in the same process -- normals_radius_kernel is the first walk of the MLS
kernel alone, the natural yardstick.

Prints ONE JSON line: milliseconds per warm call, measured with HIP events (torch.cuda.Event on the stream the context enqueues
on) around the call, median of --reps calls, for
  mls_1x200k_r1_o1 / _r1_o2 / _r2.5_o1 / _r2.5_o2    ctx.mls of one 200k view (radius in mm, polynomial order), normals computed
  normals_1x200k_r1 / _r2.5                          ctx.estimate_normals(radius=...) of the same slot
  mls_12x200k_r2.5_o2, normals_12x200k_r2.5          the twelve views posed by their turntable prior and concatenated (2.4 M points)
and, per mls entry, the output count (<name>_out), the wall time (<name>_wall) and the ratio to the normals call at the same
radius (<name>_per_normals).  A warm call reads the source slot and writes another, so every repetition sees the same input and
the source keeps its grid.  Both calls include their launches' tail: the MLS call its selection, gather and read-back, the
normals call its synchronisation; the kernels alone are in a rocprofv3 --kernel-trace --stats run of this tool (--kernels runs
each call --reps times in turn and times nothing; add --output-format csv for the csv tables).
Usage: python tools/mls_bench.py [--reps 10] [--n 200000] [--views 12] [--kernels]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    mvr = importlib.import_module("multi-view-registration_amd")
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = mvr.synth_params(a.views, 3)
    piv, ax = mvr.synth_prior(sp)
    views = [mvr.synth_view(sp, v, a.n) for v in range(a.views)]
    out = {"n": a.n, "views": a.views, "reps": a.reps}
    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        ctx.upload(0, views[0])
        posed = []
        for v, p in enumerate(views):                        # slot 1: the merged object
            ctx.upload(2, p)
            ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(2))
        ctx.upload(1, np.concatenate(posed))
        one, merged = "1x%dk" % (a.n // 1000), "%dx%dk" % (a.views, a.n // 1000)
        jobs = []
        for r in (1.0, 2.5):
            jobs.append(("normals_%s_r%g" % (one, r), lambda r=r: ctx.estimate_normals(0, radius=r), None))
            for o in (1, 2):
                jobs.append(("mls_%s_r%g_o%d" % (one, r, o), lambda r=r, o=o: ctx.mls(3, 0, r, order=o, compute_normals=True), "normals_%s_r%g" % (one, r)))
        jobs.append(("normals_%s_r2.5" % merged, lambda: ctx.estimate_normals(1, radius=2.5), None))
        jobs.append(("mls_%s_r2.5_o2" % merged, lambda: ctx.mls(3, 1, 2.5, order=2, compute_normals=True), "normals_%s_r2.5" % merged))
        if a.kernels:
            for name, call, _ in jobs:
                for _ in range(a.reps):
                    call()
            print(json.dumps({"kernels": True, "n": a.n, "views": a.views, "reps": a.reps}))
            return
        for name, call, base in jobs:
            res = call()                                     # warm: code objects, arena, buffers, the source's grid
            ev, wall = [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                ev.append(e0.elapsed_time(e1))
            out[name] = round(float(np.median(ev)), 4)
            out[name + "_wall"] = round(float(np.median(wall)), 4)
            if base:
                out[name + "_out"] = int(res)
                out[name + "_per_normals"] = round(out[name] / out[base], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
