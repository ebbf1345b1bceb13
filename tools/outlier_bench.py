"""Timing of the two outlier filters (mvr_cloud_statistical_outlier_removal, mvr_cloud_radius_outlier_removal) on synthetic
turntable views.

Prints ONE JSON line: milliseconds per warm call, measured with HIP events (torch.cuda.Event on the stream the context
enqueues on) around the call, median of --reps calls, for
  sor_1x200k_k8 / _k16 / _k50     ctx.statistical_outlier_removal of one 200k view plus 2 000 injected outliers, stddev_mul 1
  ror_1x200k_r0.45                ctx.radius_outlier_removal of the same cloud, radius 0.45 mm, 2 neighbours
  sor_12x200k_k8 / _k16 / _k50    the twelve views posed by their turntable prior and concatenated (2.4 M points)
  ror_12x200k_r0.45
and, per entry, the output count (<name>_out), the wall time (<name>_wall), the time of a call that also has to build the
cloud's grid (<name>_cold: the filter run in place on a fresh copy of the slot) and, with --numpy, the CPU time of the numpy /
kd-tree reference (<name>_numpy_ms, tests/outlier_ref.py, one call: a courtesy figure).  A warm call reads the source slot and
writes another, so every repetition sees the same input and the source keeps its grid.
With --kernels the tool instead runs the searches whose kernels are to be compared under a profiler, --reps times each, in turn:
knn(s, s, 16), knn(s, s, 17), knn(s, s, 51) and the statistical filter at mean_k 16 and 50 on the 200k cloud (knn counts the
query itself, the filter does not: mean_k 16 is the work of knn 17, mean_k 50 that of knn 51); --clean takes the view without
the injected outliers.  Nothing is timed or printed but a line that says so.
Usage: python tools/outlier_bench.py [--reps 10] [--n 200000] [--views 12] [--numpy] [--kernels [--clean]]
"""
import argparse
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--clean", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import outlier_ref
    mvr = importlib.import_module("multi-view-registration_amd")
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = mvr.synth_params(a.views, 2)
    piv, ax = mvr.synth_prior(sp)
    views = [mvr.synth_view(sp, v, a.n) for v in range(a.views)]
    rng = np.random.default_rng(7)
    lo, hi = views[0][:, :3].min(0) - 5.0, views[0][:, :3].max(0) + 5.0
    o = np.ones((a.n // 100, 4), np.float32)
    o[:, :3] = rng.uniform(lo, hi, (len(o), 3)).astype(np.float32)
    one = np.concatenate([views[0], o])
    one = np.ascontiguousarray(one[rng.permutation(len(one))])
    out = {"n": a.n, "views": a.views, "reps": a.reps}
    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        ctx.upload(0, views[0] if a.kernels and a.clean else one)
        if a.kernels:
            for _ in range(a.reps):
                ctx.knn(0, 0, 16)
                ctx.knn(0, 0, 17)
                ctx.knn(0, 0, 51)
                ctx.statistical_outlier_removal(3, 0, 16, 1.0)
                ctx.statistical_outlier_removal(3, 0, 50, 1.0)
            print(json.dumps({"kernels": True, "clean": a.clean, "n": ctx.size(0), "reps": a.reps}))
            return
        posed = []
        for v, p in enumerate(views):                        # slot 1: the merged object
            ctx.upload(2, p)
            ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(2))
        merged = np.concatenate(posed)
        ctx.upload(1, merged)

        def timed(name, call, src, ref):
            out[name + "_out"] = call(3, src)                # warm: code objects, arena, buffers, the source's grid
            ev, wall, cold = [], [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                call(3, src)
                e1.record(stream)
                e1.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                ev.append(e0.elapsed_time(e1))
            for _ in range(max(1, a.reps // 3)):
                ctx.copy(4, src)                             # a copy carries no grid over
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(4, 4)
                e1.record(stream)
                e1.synchronize()
                cold.append(e0.elapsed_time(e1))
            out[name] = round(float(np.median(ev)), 4)
            out[name + "_wall"] = round(float(np.median(wall)), 4)
            out[name + "_cold"] = round(float(np.median(cold)), 4)
            if a.numpy:
                t0 = time.perf_counter()
                r = ref()
                out[name + "_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                assert len(r["index"]) == out[name + "_out"], (name, len(r["index"]), out[name + "_out"])

        for src, host, tag in ((0, one, "1x%dk" % (a.n // 1000)), (1, merged, "%dx%dk" % (a.views, a.n // 1000))):
            for k in (8, 16, 50):
                timed("sor_%s_k%d" % (tag, k), lambda d, s, k=k: ctx.statistical_outlier_removal(d, s, k, 1.0), src,
                      lambda k=k, host=host: outlier_ref.statistical(host, k, 1.0))
            timed("ror_%s_r0.45" % tag, lambda d, s: ctx.radius_outlier_removal(d, s, 0.45, 2), src,
                  lambda host=host: outlier_ref.radius(host, 0.45, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
