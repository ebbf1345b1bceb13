"""Timing of the Euclidean cluster extraction (mvr_cloud_euclidean_clusters) on synthetic turntable views with a platter added
under the object, as tools/sac_bench.py builds them.

Prints ONE JSON line and writes it to --out (default profiles/cluster_bench.json).  Milliseconds per warm call, measured with
HIP events (torch.cuda.Event on the stream the context enqueues on) around the call, median of --reps calls, for
  <tag> = 1x200k          one 200k view
          12x200k         the twelve views posed by their turntable prior and concatenated (2.4 M)
each with 15 % of its points replaced by a platter, keys <tag>_...:
  copy_ms                 a plain device-to-device copy of the cloud (16 bytes per point read and written)
  t<tol>_call_ms          the whole call at a tolerance of 1 / 2.5 / 5 mm (min_size 10, every output array, no output slot) on a
                          slot that already holds its grid, and its n_components / n_clusters / largest
  t<tol>_cold_ms          the same right after an upload: the call builds the cloud's grid first
  t<tol>_normals_ms       the call with the slot's normals (k = 16) and eps_angle = 0.5
  t<tol>_denoise_ms       mvr_cloud_denoise(10, the same radius) on a fresh copy of the same cloud (the copy is not timed): the same
                          linking through a private sort-based grid, one sort fewer
  t<tol>_ratio            call_ms / denoise_ms
and one more: <tag>_plane_then_isolate_ms = mvr_cloud_segment_plane (perpendicular model, everything but the plane into slot 1)
followed by the clustering of slot 1 at 2.5 mm that keeps the largest cluster in place.
Usage: python tools/cluster_bench.py [--reps 10] [--n 200000] [--views 12] [--out FILE] [--root DIR]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.json"))
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    mvr = importlib.import_module("multi-view-registration_amd")
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    sp = mvr.synth_params(a.views, 3)
    piv, ax = mvr.synth_prior(sp)
    piv, ax = np.asarray(piv, np.float64), np.asarray(ax, np.float64) / np.linalg.norm(ax)
    views = [mvr.synth_view(sp, v, a.n) for v in range(a.views)]
    out = {"n": a.n, "views": a.views, "reps": a.reps}

    def timed(call, prep=None):
        if prep:
            prep()
        call()                                                   # warm: code objects, arena, buffers
        ev = []
        for _ in range(a.reps):
            if prep:
                prep()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        return round(float(np.median(ev)), 4)

    def with_platter(p, share, rng):
        """tools/sac_bench.py's: `share` of the points replaced by a disc perpendicular to the axis, below the object"""
        n = len(p)
        n_plane = int(round(share * n))
        keep = p[rng.choice(n, n - n_plane, replace=False)]
        rel = keep[:, :3].astype(np.float64) - piv
        along = rel @ ax
        radial = np.linalg.norm(rel - np.outer(along, ax), axis=1).max()
        u = np.cross(ax, [1.0, 0.0, 0.0] if abs(ax[0]) < 0.9 else [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(ax, u)
        r, t = 1.2 * radial * np.sqrt(rng.random(n_plane)), 2 * np.pi * rng.random(n_plane)
        disc = piv + (along.min() - 2.0) * ax + np.outer(r * np.cos(t), u) + np.outer(r * np.sin(t), v) + np.outer(0.1 * rng.standard_normal(n_plane), ax)
        q = np.ones((n, 4), np.float32)
        q[:len(keep)] = keep
        q[len(keep):, :3] = disc.astype(np.float32)
        return np.ascontiguousarray(q[rng.permutation(n)])

    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        posed = []
        for v, p in enumerate(views):
            ctx.upload(2, p)
            ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
            posed.append(ctx.download(2))
        clouds = (("1x%dk" % (a.n // 1000), views[0]), ("%dx%dk" % (a.views, a.n // 1000), np.concatenate(posed)))
        u32 = C.POINTER(C.c_uint32)
        rng = np.random.default_rng(11)
        for tag, cloud in clouds:
            p = with_platter(cloud, 0.15, rng)
            n = len(p)
            ctx.upload(0, p)
            ctx.estimate_normals(0, k=16)
            nrm = ctx.download_normals(0)
            src = torch.from_numpy(p).cuda()
            dst = torch.empty_like(src)
            out[tag + "_copy_ms"] = timed(lambda: dst.copy_(src))
            del src, dst
            off, cidx, lab = np.empty(n + 2, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint32)

            def clusters(dst_slot, src_slot, tol, eps=None):
                q = mvr.ClusterParams(float(tol), 10, 2 ** 31 - 1, int(eps is not None), float(eps or 0.0), 0, 1, 0)
                res, n_out = mvr.ClusterResult(), C.c_size_t()
                rc = mvr._lib.mvr_cloud_euclidean_clusters(ctx._h, dst_slot, src_slot, C.byref(q), None, 0, C.byref(res), C.byref(n_out),
                                                           off.ctypes.data_as(u32), len(off), cidx.ctypes.data_as(u32), lab.ctypes.data_as(u32))
                assert rc == mvr.OK, rc
                return res

            def reload():
                ctx.upload(0, p)
                ctx.upload_normals(0, nrm)

            def denoise(tol):
                kept, comps = C.c_size_t(), C.c_size_t()
                rc = mvr._lib.mvr_cloud_denoise(ctx._h, 3, 10, float(tol), C.byref(kept), C.byref(comps), None)
                assert rc == mvr.OK, rc

            for tol in (1.0, 2.5, 5.0):
                key = "%s_t%g" % (tag, tol)
                reload()
                out[key + "_call_ms"] = timed(lambda: clusters(-1, 0, tol))
                res = clusters(-1, 0, tol)
                out[key + "_components"], out[key + "_clusters"], out[key + "_largest"] = res.n_components, res.n_clusters, res.largest
                out[key + "_normals_ms"] = timed(lambda: clusters(-1, 0, tol, 0.5))
                out[key + "_normals_clusters"] = clusters(-1, 0, tol, 0.5).n_clusters
                out[key + "_cold_ms"] = timed(lambda: clusters(-1, 0, tol), prep=reload)
                out[key + "_denoise_ms"] = timed(lambda: denoise(tol), prep=lambda: ctx.copy(3, 0))
                out[key + "_ratio"] = round(out[key + "_call_ms"] / out[key + "_denoise_ms"], 3)

            def plane_then_isolate():
                q = mvr.SacParams(1, 0.5, 1000, 0.99, 1, (C.c_double * 3)(*ax), 0.1, 1, 1, 0)
                res = mvr.SacResult()
                rc = mvr._lib.mvr_cloud_segment_plane(ctx._h, 1, 0, C.byref(q), C.byref(res), None, None, None, None, 0)
                assert rc == mvr.OK, rc
                return res.inliers, clusters(1, 1, 2.5).largest

            reload()
            out[tag + "_plane_then_isolate_ms"] = timed(plane_then_isolate)
            out[tag + "_plane_points"], out[tag + "_object_points"] = plane_then_isolate()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
