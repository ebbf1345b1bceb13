"""Timing of the sample-consensus rejector (mvr_reject_sample_consensus and the SAMPLE_CONSENSUS stage of a chain) on synthetic
turntable views.

Prints ONE JSON line.  Milliseconds per warm call, host clock around calls that end with their own read-back, median of --reps
calls, for
  <tag> = pair            view 1 under its turntable prior against view 0 (n points each)
          merged          the same view against the twelve posed views concatenated
keys <tag>_...:
  pairs                   the correspondences of a non-reciprocal search: the list every list call below runs on
  pass_ms                 a plain device pass over as many bytes as the compacted pairs hold (mvr_cloud_transform_f32 of `pairs`
                          points: 16 bytes read and 16 written per point), the yardstick for a chunk
  chunk<c>_us             ONE MORE chunk of c = 64 / 128 / 256 attempts (tune key rej_sac_chunk): a call that finds nothing
                          (matches drawn at random, a tiny threshold) and so makes exactly max_iterations + 1 attempts, at 8 chunks less the same
                          at 4 chunks, over 4 -- the hypothesis launch, two round trips, the host's solves, the counting launch
  chunk<c>_attempt_us     that per attempt
  list_ms                 mvr_reject_correspondences with one DISTANCE stage on the same list: what the list entry costs by itself
  stage<share>_ms         the whole call at a 30 % / 70 % inlier share (the other matches drawn at random), default chunking,
                          with refine; stage<share>_us: that less list_ms; stage<share>: [attempts, refine rounds, kept, pairs]
and for the pair  icp_ms / icp_median_ms / icp_sac_ms: one whole icp_align beside icp_align_rejected with [median 2.0] and with
[sample_consensus] (--iterations iterations each), and the correspondences of their last iterations.
Usage: python tools/reject_sac_bench.py [--reps 10] [--n 200000] [--views 12] [--iterations 5] [--root DIR]
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
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--max-dist", type=float, default=4.0)
    ap.add_argument("--threshold", type=float, default=1.5)
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    mvr = importlib.import_module("multi-view-registration_amd")
    sp = mvr.synth_params(a.views, 1)
    piv, ax = mvr.synth_prior(sp)
    out = {"n": a.n, "views": a.views, "reps": a.reps, "max_dist": a.max_dist, "threshold": a.threshold}

    def timed(call):
        call()                                                   # warm: code objects, buffers, the clouds' indices
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(t)), 4)

    SRC, TGT, ALL, OUT, TMP = 0, 1, 2, 3, 4
    eye = np.eye(4, dtype=np.float32)
    rng = np.random.default_rng(0)
    with mvr.Context(0) as ctx:
        posed = []
        for v in range(a.views):
            T = mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views))
            ctx.upload(OUT, mvr.synth_view(sp, v, a.n))
            ctx.transform(OUT, OUT, T)
            posed.append(ctx.download(OUT))
            if v <= 1:
                ctx.upload(SRC if v else TGT, posed[-1])
        ctx.upload(ALL, np.concatenate(posed))
        del posed
        for tag, tgt in (("pair", TGT), ("merged", ALL)):
            q, m, d = ctx.correspondences(SRC, tgt, a.max_dist, reciprocal=False)
            n, nt = len(q), ctx.size(tgt)
            out[tag + "_pairs"], out[tag + "_target_points"] = n, nt
            ctx.upload(TMP, ctx.download(SRC)[:n])
            out[tag + "_pass_ms"] = timed(lambda: ctx.transform_f32(OUT, TMP, eye))
            mr = rng.integers(0, nt, n).astype(np.int32)           # matches drawn at random: no motion has three inliers
            for c in (64, 128, 256):
                ctx.tune(rej_sac_chunk=c)
                ms = []
                for chunks in (4, 8):
                    r = mvr.rejector("sample_consensus", 1e-6, max_iterations=c * chunks - 1, seed=1)
                    ms.append(timed(lambda: ctx.reject_sample_consensus(SRC, tgt, q, mr, d, r)))
                    res = ctx.reject_sample_consensus(SRC, tgt, q, mr, d, r)[3]
                    assert not res["found"] and res["attempts"] == c * chunks, res
                out["%s_chunk%d_us" % (tag, c)] = round((ms[1] - ms[0]) / 4 * 1e3, 1)
                out["%s_chunk%d_attempt_us" % (tag, c)] = round((ms[1] - ms[0]) / 4 / c * 1e3, 3)
            ctx.tune(rej_sac_chunk=0)
            out[tag + "_list_ms"] = timed(lambda: ctx.reject_correspondences(SRC, tgt, q, m, d, [mvr.rejector("distance", a.max_dist)]))
            for share in (30, 70):
                m2 = m.copy()
                wrong = rng.permutation(n)[: n - n * share // 100]
                m2[wrong] = rng.integers(0, nt, len(wrong))
                r = mvr.rejector("sample_consensus", a.threshold, refine=True, seed=2)
                ms = timed(lambda: ctx.reject_sample_consensus(SRC, tgt, q, m2, d, r))
                kept, _, _, res = ctx.reject_sample_consensus(SRC, tgt, q, m2, d, r)
                out["%s_stage%d_ms" % (tag, share)] = ms
                out["%s_stage%d_us" % (tag, share)] = round((ms - out[tag + "_list_ms"]) * 1e3, 1)
                out["%s_stage%d" % (tag, share)] = [res["attempts"], res["refine_rounds"], len(kept), n]
        p = mvr.icp_params(reciprocal=True, max_dist=a.max_dist, max_iter=a.iterations, teps=0.0, feps=0.0)
        chains = {"median": [mvr.rejector("median", 2.0)], "sac": [mvr.rejector("sample_consensus", a.threshold, seed=3)]}
        out["pair_icp_ms"] = timed(lambda: ctx.icp_align(SRC, TGT, OUT, p))
        stats = [ctx.icp_align(SRC, TGT, OUT, p)[1]]
        for name, chain in chains.items():
            out["pair_icp_%s_ms" % name] = timed(lambda: ctx.icp_align_rejected(SRC, TGT, OUT, p, chain))
            stats.append(ctx.icp_align_rejected(SRC, TGT, OUT, p, chain)[1])
        last = ctx.last_sample_consensus()
        out["pair_icp_sac_last"] = [last["attempts"], last["inliers"], last["live"]]
        out["pair_icp_iterations"] = [s["iterations"] for s in stats]
        out["pair_icp_n_corr"] = [s["n_corr"] for s in stats]
        out["pair_icp_mse"] = [round(s["mse"], 6) for s in stats]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
