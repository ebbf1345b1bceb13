"""Timing of the Normal Distributions Transform (mvr_ndt_cells, mvr_ndt_sums, mvr_ndt_align) on synthetic turntable views.

Writes ONE JSON line to profiles/ndt_bench.json (and prints it).  Milliseconds per warm call, host clock around calls that end
with their own read-back, median of --reps calls, the alternatives of a comparison taken in alternation, for
  <tag> = pair            view 1 under its turntable prior against view 0 (n points each)
          merged          a second sample of view 1 (another seed) under the same prior against the twelve posed views concatenated
keys <tag>_res<r>_... for the resolutions 2, 5 and 10 (millimetres):
  cells, cells_ms         the kept cells of the target and mvr_ndt_cells without a download (sort, statistics, compaction)
  dense_ms, sparse_ms     mvr_ndt_sums -- the cell build plus ONE evaluation -- through the dense table and through the search of
                          the kept keys ("ndt_dense_max" = 0)
  eval_dense_us, eval_sparse_us   what of that is the evaluation (two launches and the 232-byte read-back): minus cells_ms
  pairs                   counted (point, cell) pairs of that evaluation
  align_ms, align_iterations, align_evaluations, align_stop, align_rms
                          one whole mvr_ndt_align (step_size = resolution / 5, transformation_epsilon 0.01, rotating about the
                          target's centre), and the rms distance to the true pose (mm) it ends at (start_rms: at the prior)
and, per tag, on the same slots beside them:
  svd_ms / gicp_ms, ..._iterations, ..._rms   icp_align (reciprocal SVD, --iterations iterations) and icp_align_gicp (PCL's
                          defaults but max_dist; the 20-NN normals are estimated before the clock starts)
Times only: nothing here is a bar.
Usage: python tools/ndt_bench.py [--reps 10] [--n 200000] [--views 12] [--iterations 10] [--root DIR]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--max-dist", type=float, default=4.0)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import numpy as np
    mvr = importlib.import_module("multi-view-registration_amd")
    sp = mvr.synth_params(a.views, 1)
    piv, ax = mvr.synth_prior(sp)
    out = {"n": a.n, "views": a.views, "reps": a.reps, "max_dist": a.max_dist}

    def timed(calls):
        """the medians of calls taken in alternation"""
        for c in calls:
            c()                                                  # warm: code objects, buffers, the clouds' indices
        t = [[] for _ in calls]
        for _ in range(a.reps):
            for k, c in enumerate(calls):
                t0 = time.perf_counter()
                c()
                t[k].append((time.perf_counter() - t0) * 1e3)
        return [round(float(np.median(x)), 4) for x in t]

    ang = mvr.turntable_angle(1, a.views)
    true_axis = np.array(sp.axis) / np.linalg.norm(np.array(sp.axis))
    T_true = mvr.axis_rotation(np.array(sp.pivot), true_axis, ang) @ np.linalg.inv(mvr.axis_rotation(piv, ax, ang))

    SRC, TGT, ALL, OUT, SRC2 = 0, 1, 2, 3, 4
    with mvr.Context(0) as ctx:
        out["device"] = ctx.device_info()[0]
        posed = []
        for v in range(a.views):
            ctx.upload(OUT, mvr.synth_view(sp, v, a.n))
            ctx.transform(OUT, OUT, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(OUT))
        sp2 = mvr.synth_params(a.views, 1)
        sp2.seed += 1                                            # (the merged object holds view 1 itself: its own points would match at distance 0)
        ctx.upload(OUT, mvr.synth_view(sp2, 1, a.n))
        ctx.transform(OUT, OUT, mvr.axis_rotation(piv, ax, ang))
        sources = {"pair": posed[1], "merged": ctx.download(OUT)}
        centres = {"pair": 0.5 * (posed[0][:, :3].min(0) + posed[0][:, :3].max(0)).astype(np.float64)}
        everything = np.concatenate(posed)
        centres["merged"] = 0.5 * (everything[:, :3].min(0) + everything[:, :3].max(0)).astype(np.float64)
        ctx.upload(SRC, sources["pair"])
        ctx.upload(SRC2, sources["merged"])
        ctx.upload(TGT, posed[0])
        ctx.upload(ALL, everything)
        del posed, everything
        ctx.estimate_normals([SRC, SRC2, TGT, ALL], k=20)

        def rms(T, src):
            P = src[:, :3].astype(np.float64)
            d = (P @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]) - (P @ T_true[:3, :3].T + T_true[:3, 3])
            return round(float(np.sqrt((d * d).sum(1).mean())), 4)

        def sparse_sums(cur, tgt, prm):
            ctx.tune(ndt_dense_max=0)
            try:
                return ctx.ndt_sums(cur, tgt, prm)
            finally:
                ctx.tune(ndt_dense_max=1 << 24)

        n = mvr._sz()
        for tag, tgt, cur in (("pair", TGT, SRC), ("merged", ALL, SRC2)):
            out[tag + "_target_points"] = ctx.size(tgt)
            for res in (2.0, 5.0, 10.0):
                key = "%s_res%g_" % (tag, res)
                prm = mvr.ndt_params(resolution=res, step_size=res / 5.0, transformation_epsilon=0.01, origin=tuple(centres[tag]))
                cells = lambda: mvr._chk(mvr._lib.mvr_ndt_cells(ctx._h, tgt, ctypes.byref(prm), 0, None, None, None, None, ctypes.byref(n)), ctx._h)
                ms = timed([cells, lambda: ctx.ndt_sums(cur, tgt, prm), lambda: sparse_sums(cur, tgt, prm), lambda: ctx.ndt_align(cur, tgt, OUT, prm)])
                out[key + "cells_ms"], out[key + "dense_ms"], out[key + "sparse_ms"], out[key + "align_ms"] = ms
                out[key + "cells"] = int(n.value)
                out[key + "eval_dense_us"], out[key + "eval_sparse_us"] = round((ms[1] - ms[0]) * 1e3, 1), round((ms[2] - ms[0]) * 1e3, 1)
                out[key + "pairs"] = int(ctx.ndt_sums(cur, tgt, prm)[27])
                T, X, st, rc = ctx.ndt_align(cur, tgt, OUT, prm)
                out[key + "align_iterations"], out[key + "align_evaluations"], out[key + "align_stop"] = st["iterations"], st["evaluations"], st["stop"]
                out[key + "align_rms"] = rms(X, sources[tag])
            svd = mvr.icp_params(reciprocal=True, max_dist=a.max_dist, max_iter=a.iterations, teps=0.0, feps=0.0)
            gicp = mvr.gicp_params(max_corr_dist=a.max_dist)
            ms = timed([lambda: ctx.icp_align(cur, tgt, OUT, svd), lambda: ctx.icp_align_gicp(cur, tgt, OUT, gicp)])
            out[tag + "_svd_ms"], out[tag + "_gicp_ms"] = ms
            for name, r in (("svd", ctx.icp_align(cur, tgt, OUT, svd)), ("gicp", ctx.icp_align_gicp(cur, tgt, OUT, gicp))):
                out["%s_%s_iterations" % (tag, name)] = r[1]["iterations"]
                out["%s_%s_rms" % (tag, name)] = rms(r[0], sources[tag])
        out["start_rms"] = rms(np.eye(4), sources["pair"])
    line = json.dumps(out)
    path = a.out or os.path.join(root, "profiles", "ndt_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
