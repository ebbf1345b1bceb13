"""Timing of the FPFH descriptors (mvr_cloud_fpfh) on synthetic turntable views, beside the radius-mode normal estimation at the
same radius on the same cloud in the same process -- normals_radius_kernel is the bare ball walk both FPFH passes are built on,
the yardstick the moving-least-squares figures use (tools/mls_bench.py).

Prints ONE JSON line: milliseconds per warm call, measured with HIP events (torch.cuda.Event on the stream the context enqueues
on) around the call, median of --reps calls, for
  fpfh_1x200k_r2.5 / _r5, normals_1x200k_r2.5 / _r5     one 200k view whose normals come from radius 2.5 mm
  fpfh_12x200k_r2.5, normals_12x200k_r2.5               the twelve views posed by their turntable prior and concatenated (2.4 M)
Per fpfh entry: <name> is the call that returns the signatures to the host (n * 132 bytes over the bus into pageable memory),
<name>_device the same call with all three outputs NULL -- the four kernels and one synchronisation --, <name>_wall the host
clock around the first, <name>_neighbours the mean n_i, and <name>_device_per_normals the ratio to the normals call.  The
normals call runs on a copy of the cloud in another slot, so the FPFH input keeps the normals of radius 2.5 mm.  The kernels
alone are in a rocprofv3 --kernel-trace --stats run of this tool (--kernels runs each call --reps times in turn and times
nothing).
Usage: python tools/fpfh_bench.py [--reps 10] [--n 200000] [--views 12] [--kernels]
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
        posed = []
        for v, p in enumerate(views):
            ctx.upload(2, p)
            ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(2))
        ctx.upload(0, views[0])                                  # slot 0: one view; slot 1: the merged object
        ctx.upload(1, np.concatenate(posed))
        for s in (0, 1):
            ctx.estimate_normals(s, radius=2.5)
            ctx.copy(s + 4, s)                                   # slots 4, 5: the copies the normals yardstick overwrites

        def device_only(slot, r):
            p = mvr.FpfhParams(float(r), 0)
            rc = mvr._lib.mvr_cloud_fpfh(ctx._h, slot, C.byref(p), None, None, None)
            assert rc == mvr.OK, rc

        one, merged = "1x%dk" % (a.n // 1000), "%dx%dk" % (a.views, a.n // 1000)
        jobs = []
        for tag, slot, radii in ((one, 0, (2.5, 5.0)), (merged, 1, (2.5,))):
            for r in radii:
                nm = "normals_%s_r%g" % (tag, r)
                jobs.append((nm, lambda slot=slot, r=r: ctx.estimate_normals(slot + 4, radius=r), None))
                jobs.append(("fpfh_%s_r%g_device" % (tag, r), lambda slot=slot, r=r: device_only(slot, r), nm))
                jobs.append(("fpfh_%s_r%g" % (tag, r), lambda slot=slot, r=r: ctx.fpfh(slot, r), None))
        if a.kernels:
            for name, call, _ in jobs:
                if not name.endswith("_device"):
                    for _ in range(a.reps):
                        call()
            print(json.dumps({"kernels": True, "n": a.n, "views": a.views, "reps": a.reps}))
            return
        for name, call, base in jobs:
            call()                                               # warm: code objects, arena, buffers, the slot's grid
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
            if name.startswith("fpfh") and not base:
                out[name + "_wall"] = round(float(np.median(wall)), 4)
            if base:
                out[name + "_per_normals"] = round(out[name] / out[base], 3)
        for tag, slot, radii in ((one, 0, (2.5, 5.0)), (merged, 1, (2.5,))):
            for r in radii:
                out["fpfh_%s_r%g_neighbours" % (tag, r)] = round(float(ctx.fpfh(slot, r, return_counts=True)[1].mean()), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
