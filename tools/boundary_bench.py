"""Timing of the boundary estimation (mvr_cloud_boundary) and of the ISS keypoint detector with and without its border handling
(mvr_cloud_iss_keypoints_border / mvr_cloud_iss_keypoints) on synthetic turntable views, beside the radius-mode normal
estimation and the FPFH call at the same radius on the same cloud in the same process, and of one coarse alignment three ways:
on the keypoints of the border variant, on the keypoints without a border, on all points.  Follows tools/iss_bench.py.

Prints ONE JSON line.  Milliseconds per warm call, measured with HIP events (torch.cuda.Event on the stream the context
enqueues on) around the call, median of --reps calls (and, for the detector, the smallest and largest of them), for
  <call>_1x200k         one 200k view
  <call>_12x200k        the twelve views posed by their turntable prior and concatenated (2.4 M)
with <call> one of
  boundary_r<mm>        mvr_cloud_boundary with every host array NULL at that radius, threshold pi / 2 (the kernel and one
                        synchronisation); boundary_r<mm>_flags the call that also returns the flags; _share the share of
                        boundary points; _neighbours the mean neighbour count
  normals_r<mm>         mvr_cloud_estimate_normals in radius mode at the same radius (the bare ball walk, f64 moments, eigen-solve)
  fpfh_r<mm>            mvr_cloud_fpfh with every host array NULL at the same radius (two walks)
  iss                   mvr_cloud_iss_keypoints with no output slot and no host array at a salient / non-maximum radius of 6 x /
                        4 x the cloud's measured point spacing (as tools/iss_bench.py); iss_border the border variant at a border
                        radius of 4 x the spacing on the normals of that radius; _keypoints / _border_points what they found
Alignment: the recovery pair of tests/align_cases.py (one view against its moved copy, both voxel-downsampled at --leaf), FPFH of
both, then mvr_align_prerejective on the tables whose rows outside the keypoints are NaN -- the keypoints of the border variant
(border radius 2.5 leaves, the salient radius) and those without a border -- and on the full tables; per run the keypoint
counts, the wall milliseconds of the phases (mvr_ctx_stat prerej_match_ms / prerej_hypotheses_ms / prerej_score_ms), whether it
converged and the worst displacement of a source point from its true place.

--iss-only times the detector without a border alone, through the entry every earlier version of the library has, so that the
same file runs against an older build of the package (--root: the tree whose package is imported).
Usage: python tools/boundary_bench.py [--reps 10] [--n 200000] [--views 12] [--radii 2.5,5] [--leaf 4.0] [--align-n 60000]
                                      [--iterations 20000] [--iss-only] [--root DIR]
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--radii", default="2.5,5")
    ap.add_argument("--leaf", type=float, default=4.0)
    ap.add_argument("--align-n", type=int, default=60000)
    ap.add_argument("--iterations", type=int, default=20000)
    ap.add_argument("--iss-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    mvr = importlib.import_module("multi-view-registration_amd")
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = mvr.synth_params(a.views, 3)
    piv, ax = mvr.synth_prior(sp)
    views = [mvr.synth_view(sp, v, a.n) for v in range(a.views)]
    out = {"n": a.n, "views": a.views, "reps": a.reps, "iss_only": bool(a.iss_only)}
    radii = [float(r) for r in a.radii.split(",")]

    def timed(call, spread=False):
        call()                                                   # warm: code objects, arena, buffers, the slot's grid
        ev = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        med = round(float(np.median(ev)), 4)
        return (med, round(float(min(ev)), 4), round(float(max(ev)), 4)) if spread else med

    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        posed = []
        for v, p in enumerate(views):
            ctx.upload(2, p)
            ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(2))
        ctx.upload(0, views[0])                                  # slot 0: one view; slot 1: the merged object
        ctx.upload(1, np.concatenate(posed))

        def iss_plain(slot, rs, rn):
            p = mvr.IssParams(float(rs), float(rn), 0.975, 0.975, 5, 0)
            rc = mvr._lib.mvr_cloud_iss_keypoints(ctx._h, -1, slot, C.byref(p), None, None, None, None, None)
            assert rc == mvr.OK, rc

        def iss_border(slot, rs, rn, rb):
            p = mvr.IssParams(float(rs), float(rn), 0.975, 0.975, 5, 0)
            b = mvr.IssBorderParams(float(rb), math.pi / 2)
            rc = mvr._lib.mvr_cloud_iss_keypoints_border(ctx._h, -1, slot, C.byref(p), C.byref(b), None, None, None, None, None, None, None)
            assert rc == mvr.OK, rc

        def boundary_only(slot, r):
            p = mvr.BoundaryParams(float(r), math.pi / 2, 0, 0)
            rc = mvr._lib.mvr_cloud_boundary(ctx._h, slot, C.byref(p), None, None, None)
            assert rc == mvr.OK, rc

        def fpfh_only(slot, r):
            p = mvr.FpfhParams(float(r), 0)
            rc = mvr._lib.mvr_cloud_fpfh(ctx._h, slot, C.byref(p), None, None, None)
            assert rc == mvr.OK, rc

        for tag, slot in (("1x%dk" % (a.n // 1000), 0), ("%dx%dk" % (a.views, a.n // 1000), 1)):
            d2 = ctx.knn(slot, slot, 2)[1][:, 1]
            h = float(np.sqrt(np.median(d2[np.isfinite(d2)].astype(np.float64))))
            rs, rn, rb = 6.0 * h, 4.0 * h, 4.0 * h
            out["spacing_" + tag] = round(h, 4)
            out["iss_" + tag], out["iss_%s_min" % tag], out["iss_%s_max" % tag] = timed(lambda: iss_plain(slot, rs, rn), spread=True)
            out["iss_%s_keypoints" % tag] = int(ctx.iss_keypoints(-1, slot, rs, rn))
            if a.iss_only:
                continue
            for r in radii:
                key = "r%g_%s" % (r, tag)
                out["normals_" + key] = timed(lambda: ctx.estimate_normals(slot, radius=r))      # (leaves the slot the normals the next two calls read)
                out["boundary_" + key] = timed(lambda: boundary_only(slot, r))
                out["boundary_%s_flags" % key] = timed(lambda: ctx.boundary(slot, r))
                out["fpfh_" + key] = timed(lambda: fpfh_only(slot, r))
                out["boundary_%s_per_fpfh" % key] = round(out["boundary_" + key] / out["fpfh_" + key], 3)
                out["boundary_%s_per_normals" % key] = round(out["boundary_" + key] / out["normals_" + key], 3)
                flag, cnt = ctx.boundary(slot, r, return_counts=True)
                out["boundary_%s_share" % key] = round(float(flag.mean()), 4)
                out["boundary_%s_neighbours" % key] = round(float(cnt.mean()), 2)
            ctx.estimate_normals(slot, radius=rb)
            out["iss_border_" + tag], out["iss_border_%s_min" % tag], out["iss_border_%s_max" % tag] = timed(lambda: iss_border(slot, rs, rn, rb), spread=True)
            n_key, edge, border = ctx.iss_keypoints(-1, slot, rs, rn, border_radius=rb, return_edges=True)
            out["iss_border_%s_keypoints" % tag] = int(n_key)
            out["iss_border_%s_edge_points" % tag] = int(edge.sum())
            out["iss_border_%s_border_points" % tag] = int(border.sum())
            out["iss_border_%s_per_iss" % tag] = round(out["iss_border_" + tag] / out["iss_" + tag], 3)
        if a.iss_only:
            print(json.dumps(out))
            return

        # ---- one coarse alignment: keypoints with a border, keypoints without, all points
        sys.path.insert(0, os.path.join(root, "tests"))
        import align_cases as AC
        s_raw, t_raw = AC.recovery_view(mvr, a.align_n)
        scale = a.leaf / AC.REC_LEAF
        pts, feat, key, bkey, det_ms = [], [], [], [], []
        for slot, raw in ((8, s_raw), (9, t_raw)):
            ctx.upload(slot, raw)
            ctx.voxel_grid(slot, slot, a.leaf)
            ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS * scale)
            pts.append(ctx.download(slot))
            feat.append(ctx.fpfh(slot, AC.REC_FPFH_RADIUS * scale))
            ms = []
            for kw in (dict(), dict(border_radius=2.5 * a.leaf)):
                ctx.iss_keypoints(-1, slot, 2.5 * a.leaf, 1.5 * a.leaf, **kw)
                t0 = time.perf_counter()
                (key if not kw else bkey).append(ctx.iss_keypoints(-1, slot, 2.5 * a.leaf, 1.5 * a.leaf, return_index=True, **kw)[1])
                ms.append(round((time.perf_counter() - t0) * 1e3, 3))
            det_ms.append(ms)
        par = dict(AC.REC_PARAMS, max_iterations=a.iterations, max_dist=AC.REC_MAX_DIST * scale)
        inv = np.linalg.inv(AC.REC_POSE.astype(np.float64))
        truth = pts[0][:, :3].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
        al = {"leaf": a.leaf, "iterations": a.iterations, "source_points": len(pts[0]), "target_points": len(pts[1]),
              "detect_wall_ms_plain_border": det_ms}

        def masked(keys):
            return [np.where(np.isin(np.arange(len(f)), k)[:, None], f, np.nan).astype(np.float32) for f, k in zip(feat, keys)]

        for tag, tables, keys in (("keypoints_border", masked(bkey), bkey), ("keypoints", masked(key), key), ("all_points", feat, None)):
            ctx.align_prerejective(8, 9, tables[0], tables[1], **par)          # warm
            t0 = time.perf_counter()
            res = ctx.align_prerejective(8, 9, tables[0], tables[1], **par)
            wall = (time.perf_counter() - t0) * 1e3
            x = pts[0][:, :3].astype(np.float64) @ res["T"][:3, :3].astype(np.float64).T + res["T"][:3, 3].astype(np.float64)
            al[tag] = {"source_keypoints": len(keys[0]) if keys else len(pts[0]), "target_keypoints": len(keys[1]) if keys else len(pts[1]),
                       "wall_ms": round(wall, 3), "prerej_match_ms": round(ctx.stat("prerej_match_ms"), 3),
                       "prerej_hypotheses_ms": round(ctx.stat("prerej_hypotheses_ms"), 3), "prerej_score_ms": round(ctx.stat("prerej_score_ms"), 3),
                       "converged": bool(res["converged"]), "best_iteration": res["best_iteration"], "inliers": res["inliers"],
                       "rejected": res["rejected"], "scored": res["scored"],
                       "worst_point_mm": round(float(np.linalg.norm(x - truth, axis=1).max()), 3)}
        out["align"] = al
    print(json.dumps(out))


if __name__ == "__main__":
    main()
