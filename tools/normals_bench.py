"""Timing of the k-NN search and the normal estimation (mvr_knn, mvr_cloud_estimate_normals) on synthetic turntable views.

Prints ONE JSON line: milliseconds per warm call, measured with HIP events (torch.cuda.Event on the stream the context
enqueues on) around the call, median of --reps calls, for
  knn_k16_1x200k         ctx.knn(s, s, 16) of one 200k view against itself (lists copied to the host: 25.6 MB)
  normals_k16_1x200k     ctx.estimate_normals(s, k=16)
  normals_r1_1x200k      ctx.estimate_normals(s, radius=1.0)
  knn_k16_12x200k        twelve knn calls, one per view
  normals_k16_12x200k    ONE estimate_normals call over the twelve views
  normals_r1_12x200k     the same, radius 1.0 mm
Usage: python tools/normals_bench.py [--reps 10] [--n 200000] [--views 12]
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
    a = ap.parse_args()
    import numpy as np
    import torch
    mvr = importlib.import_module("multi-view-registration_amd")
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = mvr.synth_params(a.views, 2)
    views = [mvr.synth_view(sp, v, a.n) for v in range(a.views)]
    out = {"n": a.n, "views": a.views, "reps": a.reps}
    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        for v, p in enumerate(views):
            ctx.upload(v, p)
        slots = list(range(a.views))

        def timed(name, fn):
            fn()                                          # warm: grids, code objects, buffers
            ev, wall = [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                ev.append(e0.elapsed_time(e1))
            out[name] = round(float(np.median(ev)), 4)
            out[name + "_wall"] = round(float(np.median(wall)), 4)

        timed("knn_k16_1x200k", lambda: ctx.knn(0, 0, 16))
        timed("normals_k16_1x200k", lambda: ctx.estimate_normals(0, k=16))
        timed("normals_r1_1x200k", lambda: ctx.estimate_normals(0, radius=1.0))
        timed("knn_k16_12x200k", lambda: [ctx.knn(s, s, 16) for s in slots])
        timed("normals_k16_12x200k", lambda: ctx.estimate_normals(slots, k=16))
        timed("normals_r1_12x200k", lambda: ctx.estimate_normals(slots, radius=1.0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
