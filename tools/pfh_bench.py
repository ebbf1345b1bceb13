"""Timing of the PFH descriptors (mvr_cloud_pfh) on synthetic turntable views, beside mvr_cloud_fpfh at the same radius on the same
slot in the same process, of the feature matcher at 33 and at 125 floats per row, and of one whole sample-consensus alignment from
PFH rows beside the one from FPFH rows on the same pair.  FPFH and the 33-float matcher are the comparison: nothing here has a bar.

Writes ONE JSON line to --out (default profiles/pfh_bench.json) and prints it: milliseconds per warm call, measured with HIP
events (torch.cuda.Event on the stream the context enqueues on) around the call, median of --reps calls, for
  pfh_<cloud>_r2.5 / _r5 / _k16 / _k64           <cloud> = 1x200k: one 200k view; 12x200k: the twelve views posed by their
  fpfh_<cloud>_r2.5 / _r5                         turntable prior and concatenated (2.4 M); normals from radius 2.5 mm
Per pfh entry: <name>_device is the call with all three outputs NULL (the kernels, two synchronisations and the 24 bytes read back
between them), <name> the call that returns the signatures to the host (n * 500 bytes into pageable memory; the one view
only), <name>_pairs the sum of m_i, <name>_gpairs_per_s = pairs / device time / 1e9, <name>_neighbours the mean n_i,
<name>_tiled the queries on the tiled path, <name>_per_fpfh the ratio of the device time to FPFH's at that radius.  The merged
object at 5 mm (about 16 times the pairs of 2.5 mm) runs only with --full.
  knn33_<n> / knn125_<n>                          mvr_feature_knn, n query rows in n target rows, k = 2, n = 5k and 50k: host
                                                  tables in, host tables out, as the call is
  align_fpfh / align_pfh                          align_prerejective (20 000 iterations, 3 samples, k = 2) of a 60k view moved by
                                                  70 degrees and voxel-downsampled at 4 mm onto the downsampled view, descriptors at
                                                  20 mm; *_match_ms / *_hypotheses_ms / *_score_ms the library's own phase clocks,
                                                  *_worst_mm the largest displacement from the true pose
Usage: python tools/pfh_bench.py [--reps 5] [--n 200000] [--views 12] [--full] [--out profiles/pfh_bench.json]
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
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfh_bench.json"))
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

    def timed(call, reps):
        call()                                                   # warm: code objects, arena, buffers, the slot's grid
        ev, wall = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        return round(float(np.median(ev)), 4), round(float(np.median(wall)), 4)

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

        def pfh_device(slot, radius, k):
            p = mvr.PfhParams(float(radius or 0.0), int(k or 0), 0)
            rc = mvr._lib.mvr_cloud_pfh(ctx._h, slot, C.byref(p), None, None, None)
            assert rc == mvr.OK, rc

        def fpfh_device(slot, radius):
            p = mvr.FpfhParams(float(radius), 0)
            rc = mvr._lib.mvr_cloud_fpfh(ctx._h, slot, C.byref(p), None, None, None)
            assert rc == mvr.OK, rc

        def save():                                              # after every section: a run cut short leaves what it measured
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(out) + "\n")

        def descriptors(tag, slot, radii):
            for r in radii:
                out["fpfh_%s_r%g_device" % (tag, r)] = timed(lambda: fpfh_device(slot, r), a.reps)[0]
            for mode, radius, k in [("r%g" % r, r, None) for r in radii] + [("k16", None, 16), ("k64", None, 64)]:
                nm = "pfh_%s_%s" % (tag, mode)
                t0 = time.perf_counter()
                pfh_device(slot, radius, k)
                first = time.perf_counter() - t0
                out[nm + "_device"] = timed(lambda: pfh_device(slot, radius, k), 1 if first > 10.0 else a.reps)[0]
                pairs = ctx.stat("pfh_pairs")
                out[nm + "_pairs"] = int(pairs)
                out[nm + "_gpairs_per_s"] = round(pairs / (out[nm + "_device"] * 1e-3) / 1e9, 3)
                out[nm + "_tiled"] = int(ctx.stat("pfh_tiled_queries"))
                if radius is not None:
                    out[nm + "_per_fpfh"] = round(out[nm + "_device"] / out["fpfh_%s_r%g_device" % (tag, radius)], 2)
                if slot == 0:
                    out[nm], out[nm + "_wall"] = timed(lambda: ctx.pfh(slot, radius=radius, k=k), a.reps)
                    out[nm + "_neighbours"] = round(float(ctx.pfh(slot, radius=radius, k=k, return_neighbors=True)[1].mean()), 2)
                save()

        descriptors("1x%dk" % (a.n // 1000), 0, (2.5, 5.0))

        # the matcher: rows like signatures (most of the mass in few bins), host tables in and out
        rng = np.random.default_rng(1)
        for n in (5000, 50000):
            for dim in (33, 125):
                q = (rng.uniform(0, 100, (n, dim)) * rng.uniform(0, 1, (n, dim)) ** 6).astype(np.float32)
                t = (rng.uniform(0, 100, (n, dim)) * rng.uniform(0, 1, (n, dim)) ** 6).astype(np.float32)
                nm = "knn%d_%dk" % (dim, n // 1000)
                out[nm], out[nm + "_wall"] = timed(lambda: ctx.feature_knn(q, t, 2), a.reps)

        # one whole alignment from either descriptor on the same pair
        ang, axis = np.deg2rad(70.0), np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
        Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
        c, shift = np.array([0.0, 0.0, 917.0]), np.array([7.0, -3.0, 11.0])
        tv = mvr.synth_view(mvr.synth_params(12, 3), 0, 60000)
        sv = tv.copy()
        sv[:, :3] = ((tv[:, :3].astype(np.float64) - c) @ R.T + c + shift).astype(np.float32)
        for slot, pts in ((20, sv), (21, tv)):
            ctx.upload(slot, pts)
            ctx.voxel_grid(slot, slot, 4.0)
            ctx.estimate_normals(slot, radius=10.0)
        s = ctx.download(20)
        want = (s[:, :3].astype(np.float64) - shift - c) @ R + c      # the inverse pose: the source back on the target
        prm = dict(max_iterations=20000, nr_samples=3, k=2, similarity=0.9, max_dist=6.0, inlier_fraction=0.25, seed=7)
        out["align_points"] = [int(ctx.size(20)), int(ctx.size(21))]
        for name, make in (("fpfh", lambda slot: ctx.fpfh(slot, 20.0)), ("pfh", lambda slot: ctx.pfh(slot, radius=20.0))):
            out["align_%s_descriptors" % name] = timed(lambda: (make(20), make(21)), a.reps)[0]
            sf, tf = make(20), make(21)
            out["align_" + name], out["align_%s_wall" % name] = timed(lambda: ctx.align_prerejective(20, 21, sf, tf, **prm), a.reps)
            res = ctx.align_prerejective(20, 21, sf, tf, **prm)
            for ph in ("match", "hypotheses", "score"):
                out["align_%s_%s_ms" % (name, ph)] = round(ctx.stat("prerej_%s_ms" % ph), 3)
            x = s[:, :3].astype(np.float64) @ res["T"][:3, :3].astype(np.float64).T + res["T"][:3, 3].astype(np.float64)
            out["align_%s_converged" % name] = bool(res["converged"])
            out["align_%s_scored" % name] = res["scored"]
            out["align_%s_worst_mm" % name] = round(float(np.linalg.norm(x - want, axis=1).max()), 3)
        save()
        descriptors("%dx%dk" % (a.views, a.n // 1000), 1, (2.5, 5.0) if a.full else (2.5,))      # the long one last
        out["complete"] = True
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
