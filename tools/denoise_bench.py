#!/usr/bin/env python3
"""tools/denoise_bench.py [N] [--far-point MM] [--reps R] -- PointCloud::denoise on one N-point scan (200 000) + 2 % outliers:
GPU (mvr_cloud_denoise) vs the CPU oracle, same input, same output (checked).  Prints one JSON line.
--far-point MM adds ONE point MM millimetres along x from the pivot: the grid has 10 bits per axis of the bounding box, so
every cell becomes MM / 1023 wide, the object fits into a few of them and the union pass is close to all pairs."""
import argparse, importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
mvr = importlib.import_module("multi-view-registration_amd")
import oracle as orc      # checker / CPU baseline only

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=200000)
ap.add_argument("--far-point", type=float, default=None, metavar="MM")
ap.add_argument("--reps", type=int, default=6, help="calls, the first of which is not in the median")
args = ap.parse_args()
n = args.n
rng = np.random.default_rng(43)
sp = mvr.synth_params(12, 2)
scan = mvr.synth_view(sp, 3, n)
noise = np.ones((n // 50, 4), np.float32); noise[:, :3] = rng.uniform(-150, 150, (n // 50, 3)) + np.array(sp.pivot)
pts = np.concatenate([scan, noise])[rng.permutation(n + n // 50)]
if args.far_point is not None:
    far = np.ones((1, 4), np.float32); far[0, :3] = np.array(sp.pivot) + [args.far_point, 0.0, 0.0]
    pts = np.concatenate([pts, far])
with mvr.Context(0) as ctx:
    times = []
    for rep in range(max(args.reps, 2)):
        ctx.upload(0, pts); ctx.sync()
        t0 = time.perf_counter()
        keep, ncomp = ctx.denoise(0, 10, 2.5)
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    okeep, _, oncomp = orc.denoise(pts, 10, 2.5)
    cpu = time.perf_counter() - t0
    assert np.array_equal(keep, okeep) and ncomp == oncomp
    print(json.dumps(dict(points=len(pts), far_point_mm=args.far_point, kept=int(len(keep)), components=int(ncomp), gpu_ms=1e3 * float(np.median(times[1:])),
                          gpu_ms_first_call=1e3 * times[0], cpu_oracle_ms=1e3 * cpu, points_per_s_gpu=len(pts) / float(np.median(times[1:])),
                          note="GPU time includes two radix sorts, the union-find pass and the D2H of the kept index list")))
