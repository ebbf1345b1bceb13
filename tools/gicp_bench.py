"""Timing of Generalized ICP (mvr_gicp_sums, mvr_gicp_solve, mvr_icp_align_gicp) on synthetic turntable views.

Writes ONE JSON line to profiles/gicp_bench.json (and prints it).  Milliseconds per warm call, host clock around calls that end
with their own read-back, median of --reps calls, the alternatives of a comparison taken in alternation, for
  <tag> = pair            view 1 under its turntable prior against view 0 (n points each, 20-NN normals estimated on the device)
          merged          a second sample of view 1 (another seed) under the same prior against the twelve posed views concatenated
keys <tag>_...:
  list                    the correspondences the optimisation runs on: those of the non-reciprocal search at max_dist
  sums_ms                 mvr_gicp_sums: the list up, ONE evaluation + step pair, the state block back
  list_up_ms              what of that is the list's validation and upload: mvr_pair_moments2_from_corr on the same list,
                          which uploads it the same way and runs one (cheaper) sums launch
  solve_chunk<c>_ms       mvr_gicp_solve, one whole inner optimisation, at inner_chunk = 1, 4 and 0 (all at once)
  solve_evaluations       evaluations of the objective that optimisation took
  pair_us_per_evaluation  (solve_chunk0_ms - sums_ms) / (evaluations - 1): what one more evaluation + step pair costs once the
                          list is up, in microseconds
  gicp_ms / gicp_chunk<c>_ms   one whole icp_align_gicp (PCL's defaults but max_dist) at the default inner_chunk, and at 1 and 4
  svd_ms, plane_ms        icp_align, reciprocal SVD and point-to-plane, at the same max_dist, --iterations iterations each
  *_iterations, *_rms     the iterations each took and the rms distance to the true pose (mm) it ends at (start_rms: at the prior)
                          (the merged object lies under the prior itself, so there nothing moves towards the true pose)
Usage: python tools/gicp_bench.py [--reps 10] [--n 200000] [--views 12] [--iterations 10] [--root DIR]
"""
import argparse
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
    out = {"n": a.n, "views": a.views, "reps": a.reps, "max_dist": a.max_dist, "default_inner_chunk": int(mvr.gicp_params().inner_chunk)}

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
        ctx.upload(SRC, sources["pair"])
        ctx.upload(SRC2, sources["merged"])
        ctx.upload(TGT, posed[0])
        ctx.upload(ALL, np.concatenate(posed))
        del posed
        t0 = time.perf_counter()
        ctx.estimate_normals([SRC, SRC2, TGT, ALL], k=20)
        out["normals_ms"] = round((time.perf_counter() - t0) * 1e3, 3)

        def rms(T, src):
            P = src[:, :3].astype(np.float64)
            d = (P @ T[:3, :3].T.astype(np.float64) + T[:3, 3]) - (P @ T_true[:3, :3].T + T_true[:3, 3])
            return round(float(np.sqrt((d * d).sum(1).mean())), 4)

        for tag, tgt, cur in (("pair", TGT, SRC), ("merged", ALL, SRC2)):
            q, m, _ = ctx.correspondences(cur, tgt, a.max_dist, reciprocal=False)
            out[tag + "_target_points"], out[tag + "_list"] = ctx.size(tgt), len(q)
            prm = {c: mvr.gicp_params(max_corr_dist=a.max_dist, inner_chunk=c) for c in (1, 4, 0)}
            ms = timed([lambda: ctx.gicp_sums(cur, tgt, q, m), lambda: ctx.pair_moments2_from_corr(cur, tgt, q, m, np.zeros(3)),
                        lambda: ctx.gicp_solve(cur, tgt, q, m, prm[1]), lambda: ctx.gicp_solve(cur, tgt, q, m, prm[4]),
                        lambda: ctx.gicp_solve(cur, tgt, q, m, prm[0])])
            out[tag + "_sums_ms"], out[tag + "_list_up_ms"] = ms[0], ms[1]
            out[tag + "_solve_chunk1_ms"], out[tag + "_solve_chunk4_ms"], out[tag + "_solve_chunk0_ms"] = ms[2], ms[3], ms[4]
            info = ctx.gicp_solve(cur, tgt, q, m, prm[0])[1]
            out[tag + "_solve_evaluations"] = info["evaluations"]
            out[tag + "_pair_us_per_evaluation"] = round((ms[4] - ms[0]) * 1e3 / max(1, info["evaluations"] - 1), 2)
            default = mvr.gicp_params(max_corr_dist=a.max_dist)
            svd = mvr.icp_params(reciprocal=True, max_dist=a.max_dist, max_iter=a.iterations, teps=0.0, feps=0.0)
            plane = mvr.icp_params(reciprocal=True, max_dist=a.max_dist, max_iter=a.iterations, teps=0.0, feps=0.0, point_to_plane=True)
            ms = timed([lambda: ctx.icp_align_gicp(cur, tgt, OUT, default), lambda: ctx.icp_align_gicp(cur, tgt, OUT, prm[1]),
                        lambda: ctx.icp_align_gicp(cur, tgt, OUT, prm[4]), lambda: ctx.icp_align_gicp(cur, tgt, OUT, prm[0]),
                        lambda: ctx.icp_align(cur, tgt, OUT, svd), lambda: ctx.icp_align(cur, tgt, OUT, plane)])
            for key, v in zip(("gicp_ms", "gicp_chunk1_ms", "gicp_chunk4_ms", "gicp_chunk0_ms", "svd_ms", "plane_ms"), ms):
                out["%s_%s" % (tag, key)] = v
            runs = {"gicp": ctx.icp_align_gicp(cur, tgt, OUT, default, return_trace=True), "svd": ctx.icp_align(cur, tgt, OUT, svd),
                    "plane": ctx.icp_align(cur, tgt, OUT, plane)}
            for key, r in runs.items():
                out["%s_%s_iterations" % (tag, key)] = r[1]["iterations"]
                out["%s_%s_rms" % (tag, key)] = rms(r[0], sources[tag])
            out[tag + "_gicp_evaluations"] = [t["inner_evals"] for t in runs["gicp"][3]]
            out[tag + "_gicp_n_corr"] = runs["gicp"][1]["n_corr"]
        out["start_rms"] = rms(np.eye(4), sources["pair"])
    line = json.dumps(out)
    path = a.out or os.path.join(root, "profiles", "gicp_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
