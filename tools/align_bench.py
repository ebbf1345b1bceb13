"""Timing of the feature matching (mvr_feature_knn), the pose scoring (mvr_pose_scores) and one whole sample-consensus
alignment (mvr_align_prerejective) on synthetic data.

Prints ONE JSON line.  Milliseconds are per warm call, measured with HIP events (torch.cuda.Event on the stream the context
enqueues on) around the call, median of --reps calls:
  feature_knn_<n>x<n>_k<k>           the k-NN of n random 33-float rows in n others, n = 5k, 50k, 200k, k = 2 and 10 -- the call
                                      as a user makes it: both tables go to the device and the lists come back (for 200k rows
                                      26 MB each way beside 4e10 pairs); <name>_pairs_per_s = n * n / that time, and
                                      <name>_share_of_f32_rate = 99 operations per pair over the non-fused f32 vector rate of the
                                      device (compute units x 64 lanes x clock) -- a report, not a bar
  pose_scores_<ns>_x1000              1 000 poses of a 5k / 20k source (a voxel-downsampled view) against a 200k view, half of
                                      them within a few millimetres of the true pose, half anywhere; <name>_queries_per_s
  align_ms / align_*                  one alignment of a voxel-downsampled pair (a view and the same view moved by 70 degrees),
                                      wall clock, and its split into matching, hypothesis generation and scoring
                                      (mvr_ctx_stat "prerej_match_ms" / "prerej_hypotheses_ms" / "prerej_score_ms")
--kernels runs one alignment and one k-NN of 50k rows and times nothing: the process to put under rocprofv3 --kernel-trace --stats.
Usage: python tools/align_bench.py [--reps 5] [--n 200000] [--kernels]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEAF, NORMAL_RADIUS, FPFH_RADIUS, MAX_DIST = 4.0, 10.0, 20.0, 6.0


def rodrigues(np, axis, ang):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def rigid(np, axis, ang, shift, centre):
    T = np.eye(4)
    T[:3, :3] = rodrigues(np, axis, ang)
    T[:3, 3] = np.asarray(centre) - T[:3, :3] @ np.asarray(centre) + np.asarray(shift)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--iterations", type=int, default=20000)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    mvr = importlib.import_module("multi-view-registration_amd")
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(1)
    view = mvr.synth_view(mvr.synth_params(12, 3), 0, a.n)
    centre = view[:, :3].astype(np.float64).mean(0)
    pose = rigid(np, [0.3, -0.5, 0.81], np.deg2rad(70.0), (7.0, -3.0, 11.0), centre)      # target -> source
    moved = view.copy()
    moved[:, :3] = (view[:, :3].astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)
    out = {"n": a.n, "reps": a.reps}
    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        name, n_cu, mhz = ctx.device_info()
        rate = n_cu * 64 * mhz * 1e6
        out.update(device=name, f32_vector_ops_per_s=rate)

        def timed(call, reps=a.reps):
            call()                                               # warm: code objects, buffers, the slots' grids
            ev = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                ev.append(e0.elapsed_time(e1))
            return float(np.median(ev))

        # the pair of the alignment: slots 0 / 1 downsampled, with normals; their descriptors
        feats = []
        for slot, p in ((0, moved), (1, view)):
            ctx.upload(slot, p)
            ctx.voxel_grid(slot, slot, LEAF)
            ctx.estimate_normals(slot, radius=NORMAL_RADIUS)
            feats.append(ctx.fpfh(slot, FPFH_RADIUS))
        args = dict(max_iterations=a.iterations, nr_samples=3, k=2, similarity=0.9, max_dist=MAX_DIST, inlier_fraction=0.25, seed=7)

        def align():
            return ctx.align_prerejective(0, 1, feats[0], feats[1], **args)

        if a.kernels:
            align()
            q = rng.uniform(0, 100, (50000, 33)).astype(np.float32)
            ctx.feature_knn(q, q[::-1].copy(), 10)
            print(json.dumps({"kernels": True, "n": a.n}))
            return
        for n in (5000, 50000, 200000):
            q, t = rng.uniform(0, 100, (n, 33)).astype(np.float32), rng.uniform(0, 100, (n, 33)).astype(np.float32)
            for k in (2, 10):
                nm = "feature_knn_%dkx%dk_k%d" % (n // 1000, n // 1000, k)
                ms = timed(lambda: ctx.feature_knn(q, t, k), reps=a.reps if n < 200000 else min(a.reps, 3))
                out[nm] = round(ms, 4)
                out[nm + "_pairs_per_s"] = float("%.4g" % (n * float(n) / (ms * 1e-3)))
                out[nm + "_share_of_f32_rate"] = round(99.0 * n * float(n) / (ms * 1e-3) / rate, 4)
        # scoring: sources of 5k and 20k points (the moved view, downsampled at two leaves) against the 200k view
        ctx.upload(2, view)
        inv = np.linalg.inv(pose)
        near = [rigid(np, rng.standard_normal(3), rng.uniform(0, 0.02), rng.normal(0, 1.0, 3), centre) @ inv for _ in range(500)]
        far = [rigid(np, rng.standard_normal(3), rng.uniform(0, np.pi), rng.normal(0, 30.0, 3), centre) @ inv for _ in range(500)]
        P = np.stack(near + far).astype(np.float32)
        for want, slot in ((5000, 3), (20000, 4)):
            ctx.upload(slot, moved[rng.choice(len(moved), want, replace=False)])
            ns = ctx.size(slot)
            nm = "pose_scores_%dk_x1000" % (ns // 1000)
            ms = timed(lambda: ctx.pose_scores(slot, 2, P, MAX_DIST))
            inl, _ = ctx.pose_scores(slot, 2, P, MAX_DIST)
            out[nm] = round(ms, 4)
            out[nm + "_queries_per_s"] = float("%.4g" % (len(P) * float(ns) / (ms * 1e-3)))
            out[nm + "_mean_inlier_share_near_far"] = [round(float(inl[:500].mean() / ns), 3), round(float(inl[500:].mean() / ns), 3)]
        align()
        wall, parts = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = align()
            wall.append((time.perf_counter() - t0) * 1e3)
            parts.append([ctx.stat("prerej_match_ms"), ctx.stat("prerej_hypotheses_ms"), ctx.stat("prerej_score_ms")])
        parts = np.median(np.array(parts), axis=0)
        x = moved[:, :3].astype(np.float64) @ res["T"][:3, :3].astype(np.float64).T + res["T"][:3, 3].astype(np.float64)
        out.update(align_points=[ctx.size(0), ctx.size(1)], align_iterations=a.iterations, align_ms=round(float(np.median(wall)), 3),
                   align_match_ms=round(float(parts[0]), 3), align_hypotheses_ms=round(float(parts[1]), 3), align_score_ms=round(float(parts[2]), 3),
                   align_converged=bool(res["converged"]), align_inliers=res["inliers"], align_scored=res["scored"], align_rejected=res["rejected"],
                   align_worst_displacement_mm=round(float(np.linalg.norm(x - view[:, :3].astype(np.float64), axis=1).max()), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
