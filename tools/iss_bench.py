"""Timing of the ISS keypoint detector (mvr_cloud_iss_keypoints) on synthetic turntable views, beside the radius-mode normal
estimation at the salient radius on the same cloud in the same process -- normals_radius_kernel is the bare ball walk with the
same f64 moments and the full eigen-solve, the yardstick of the MLS and FPFH figures (tools/mls_bench.py, tools/fpfh_bench.py)
-- and of one coarse alignment with and without keypoints.

Prints ONE JSON line.  Detector: milliseconds per warm call, measured with HIP events (torch.cuda.Event on the stream the context
enqueues on) around the call, median of --reps calls, at a salient / non-maximum radius of 6 x / 4 x the cloud's measured point
spacing (the median distance to the nearest other point, from mvr_knn with k = 2), for
  iss_1x200k, normals_1x200k        one 200k view
  iss_12x200k, normals_12x200k      the twelve views posed by their turntable prior and concatenated (2.4 M)
<name> is the call with no output slot and no host array (dst = -1: the two kernels, the selection and two synchronisations),
<name>_index the call that also returns the indices, <name>_per_normals the ratio to the normals call, <name>_keypoints /
_salient_neighbours / _nms_neighbours what it found.  Alignment: the recovery pair of tests/align_cases.py (one view against its
moved copy, both voxel-downsampled at --leaf), FPFH of both, then mvr_align_prerejective on the full tables and on the tables
whose non-keypoint rows are NaN -- what ScanCloud::alignPrerejective does with use_keypoints; per run the wall milliseconds of
the phases (mvr_ctx_stat prerej_match_ms / prerej_hypotheses_ms / prerej_score_ms), the detector's two calls, and the outcome.
The kernels alone are in a rocprofv3 --kernel-trace --stats run of this tool (--kernels runs each call --reps times in turn and
times nothing).
Usage: python tools/iss_bench.py [--reps 10] [--n 200000] [--views 12] [--leaf 4.0] [--align-n 60000] [--iterations 20000] [--kernels]
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
    ap.add_argument("--leaf", type=float, default=4.0)
    ap.add_argument("--align-n", type=int, default=60000)
    ap.add_argument("--iterations", type=int, default=20000)
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

    def timed(call):
        call()                                                   # warm: code objects, arena, buffers, the slot's grid
        ev = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        return round(float(np.median(ev)), 4)

    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        posed = []
        for v, p in enumerate(views):
            ctx.upload(2, p)
            ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(2))
        ctx.upload(0, views[0])                                  # slot 0: one view; slot 1: the merged object
        ctx.upload(1, np.concatenate(posed))

        def device_only(slot, rs, rn):
            p = mvr.IssParams(float(rs), float(rn), 0.975, 0.975, 5, 0)
            rc = mvr._lib.mvr_cloud_iss_keypoints(ctx._h, -1, slot, C.byref(p), None, None, None, None, None)
            assert rc == mvr.OK, rc

        for tag, slot in (("1x%dk" % (a.n // 1000), 0), ("%dx%dk" % (a.views, a.n // 1000), 1)):
            d2 = ctx.knn(slot, slot, 2)[1][:, 1]
            h = float(np.sqrt(np.median(d2[np.isfinite(d2)].astype(np.float64))))
            rs, rn = 6.0 * h, 4.0 * h
            ctx.copy(slot + 4, slot)                             # slots 4, 5: the copies the normals yardstick writes its normals into
            jobs = (("normals_" + tag, lambda: ctx.estimate_normals(slot + 4, radius=rs)),
                    ("iss_" + tag, lambda: device_only(slot, rs, rn)),
                    ("iss_%s_index" % tag, lambda: ctx.iss_keypoints(-1, slot, rs, rn, return_index=True)))
            if a.kernels:
                for name, call in jobs[:2]:
                    for _ in range(a.reps):
                        call()
                continue
            out["spacing_" + tag] = round(h, 4)
            for name, call in jobs:
                out[name] = timed(call)
            out["iss_%s_per_normals" % tag] = round(out["iss_" + tag] / out["normals_" + tag], 3)
            n_key, sc, nc = ctx.iss_keypoints(-1, slot, rs, rn, return_counts=True)
            out["iss_%s_keypoints" % tag] = int(n_key)
            out["iss_%s_salient_neighbours" % tag] = round(float(sc.mean()), 2)
            out["iss_%s_nms_neighbours" % tag] = round(float(nc[nc > 0].mean()) if (nc > 0).any() else 0.0, 2)
        if a.kernels:
            print(json.dumps({"kernels": True, "n": a.n, "views": a.views, "reps": a.reps}))
            return

        # ---- one coarse alignment, with and without keypoints
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import align_cases as AC
        s_raw, t_raw = AC.recovery_view(mvr, a.align_n)
        scale = a.leaf / AC.REC_LEAF
        pts, feat, key, det_ms = [], [], [], []
        for slot, raw in ((8, s_raw), (9, t_raw)):
            ctx.upload(slot, raw)
            ctx.voxel_grid(slot, slot, a.leaf)
            ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS * scale)
            pts.append(ctx.download(slot))
            feat.append(ctx.fpfh(slot, AC.REC_FPFH_RADIUS * scale))
            ctx.iss_keypoints(-1, slot, 2.5 * a.leaf, 1.5 * a.leaf)
            t0 = time.perf_counter()
            key.append(ctx.iss_keypoints(-1, slot, 2.5 * a.leaf, 1.5 * a.leaf, return_index=True)[1])
            det_ms.append((time.perf_counter() - t0) * 1e3)
        par = dict(AC.REC_PARAMS, max_iterations=a.iterations, max_dist=AC.REC_MAX_DIST * scale)
        inv = np.linalg.inv(AC.REC_POSE.astype(np.float64))
        truth = pts[0][:, :3].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
        al = {"leaf": a.leaf, "iterations": a.iterations, "source_points": len(pts[0]), "target_points": len(pts[1]),
              "source_keypoints": len(key[0]), "target_keypoints": len(key[1]), "detect_wall_ms": [round(v, 3) for v in det_ms]}
        for tag, tables in (("all_points", feat), ("keypoints", [np.where(np.isin(np.arange(len(f)), k)[:, None], f, np.nan).astype(np.float32)
                                                                 for f, k in zip(feat, key)])):
            ctx.align_prerejective(8, 9, tables[0], tables[1], **par)          # warm
            t0 = time.perf_counter()
            res = ctx.align_prerejective(8, 9, tables[0], tables[1], **par)
            wall = (time.perf_counter() - t0) * 1e3
            x = pts[0][:, :3].astype(np.float64) @ res["T"][:3, :3].astype(np.float64).T + res["T"][:3, 3].astype(np.float64)
            al[tag] = {"wall_ms": round(wall, 3), "prerej_match_ms": round(ctx.stat("prerej_match_ms"), 3),
                       "prerej_hypotheses_ms": round(ctx.stat("prerej_hypotheses_ms"), 3), "prerej_score_ms": round(ctx.stat("prerej_score_ms"), 3),
                       "converged": bool(res["converged"]), "best_iteration": res["best_iteration"], "inliers": res["inliers"],
                       "rejected": res["rejected"], "scored": res["scored"],
                       "worst_point_mm": round(float(np.linalg.norm(x - truth, axis=1).max()), 3)}
        out["align"] = al
    print(json.dumps(out))


if __name__ == "__main__":
    main()
