"""Timing of the SHOT local reference frames and descriptors (mvr_cloud_shot_lrf, mvr_cloud_shot, mvr_cloud_shot_at) beside FPFH
and PFH at the same radius, of the matcher at 33 / 125 / 352 floats per row, and of one coarse alignment from each descriptor.
There is no time bar: the numbers are what they are.

Merges its keys into ONE JSON line in --out (default profiles/shot_bench.json) and prints them.  One --section per process, so
that a caller can put every section under a time limit of its own and chain them:
  view    a 200k view at 2.5 and 5 mm        object  the twelve posed views concatenated (2.4 M) at 2.5 mm
  match   mvr_feature_knn on 5k x 5k rows    align   the recovery pair of tests/align_cases.py, by phase
A time is milliseconds of a warm call with every output NULL (kernels, the norm of rule H8 and synchronisations; the rows are
not written to device memory nor copied out: a call that asks for the table pays 1.4 KiB per row on top, the align_* figures
show it), measured with HIP events around the call: [median, min, max] of --reps calls.
  <cloud>_r<radius>_lrf / _desc / _shot     frames alone; descriptor with frames passed in (their upload included); the whole call
  <cloud>_r<radius>_fpfh / _pfh             the existing calls at the same radius (PFH on the object at 2.5 mm only)
  <cloud>_r<radius>_iss_*                   the same through the _at entries at the cloud's ISS keypoints; _iss_queries: how many
  match_<dim>                               k = 2, 5 000 queries in 5 000 rows
  align_<name>_*                            descriptors on both clouds (wall ms, tables on the host), then the aligner's three
                                            phases (matching, hypotheses, scoring) and its result; FPFH and PFH at 20 mm, SHOT at
                                            20 mm (shot20) and at 40 mm (shot: tests/test_gpu_shot_match.py says why)
Usage: python tools/shot_bench.py --section view [--reps 5] [--n 200000] [--views 12] [--out profiles/shot_bench.json]
The whole run, every GPU step under a time limit of its own, the next only after the last ended well:
  timeout -k 10 200 python tools/shot_bench.py --section view && timeout -k 10 100 python tools/shot_bench.py --section match && \
  timeout -k 10 150 python tools/shot_bench.py --section align && timeout -k 10 300 python tools/shot_bench.py --section object
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("view", "object", "match", "align"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shot_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    mvr = importlib.import_module("multi-view-registration_amd")
    torch.cuda.init()
    stream = torch.cuda.current_stream()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.loads(f.readline() or "{}")
    out.update({"n": a.n, "views": a.views, "reps": a.reps, "device": torch.cuda.get_device_name(0)})

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")

    def timed(call):
        t0 = time.perf_counter()
        call()                                                   # warm: code objects, arena, buffers, the slot's grid
        reps = 1 if time.perf_counter() - t0 > 5.0 else a.reps
        ev = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        return [round(float(np.median(ev)), 4), round(float(min(ev)), 4), round(float(max(ev)), 4)]

    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float)) if x is not None else None
    with mvr.Context(0, stream=stream.cuda_stream) as ctx:
        L, h = mvr._lib, ctx._h

        def ok(rc):
            assert rc == mvr.OK, rc

        def cloud_section(tag, radii, with_pfh):
            n = ctx.size(0)
            ctx.estimate_normals(0, radius=2.5)
            _, d2 = ctx.knn(0, 0, 2)
            spacing = float(np.sqrt(np.median(d2[:, 1])))
            key = np.ascontiguousarray(ctx.iss_keypoints(-1, 0, 6.0 * spacing, 4.0 * spacing, return_index=True)[1], np.uint32)
            kp = key.ctypes.data_as(C.POINTER(C.c_uint32))
            out[tag + "_points"], out[tag + "_iss_queries"] = int(n), int(len(key))
            for r in radii:
                nm = "%s_r%g" % (tag, r)
                sp_, fpp, pp = mvr.ShotParams(r, 0.0, 0), mvr.FpfhParams(r, 0), mvr.PfhParams(r, 0, 0)
                frames = ctx.shot_lrf(0, r)
                out[nm + "_lrf"] = timed(lambda: ok(L.mvr_cloud_shot_lrf(h, 0, C.byref(sp_), None, None)))
                out[nm + "_desc"] = timed(lambda: ok(L.mvr_cloud_shot(h, 0, C.byref(sp_), fp(frames), None, None, None, None)))
                out[nm + "_shot"] = timed(lambda: ok(L.mvr_cloud_shot(h, 0, C.byref(sp_), None, None, None, None, None)))
                out[nm + "_fpfh"] = timed(lambda: ok(L.mvr_cloud_fpfh(h, 0, C.byref(fpp), None, None, None)))
                save()
                if with_pfh(r):
                    out[nm + "_pfh"] = timed(lambda: ok(L.mvr_cloud_pfh(h, 0, C.byref(pp), None, None, None)))
                kframes = np.ascontiguousarray(frames[key])
                out[nm + "_iss_desc"] = timed(lambda: ok(L.mvr_cloud_shot_at(h, 0, kp, len(key), 0, C.byref(sp_), fp(kframes), None, None, None, None)))
                out[nm + "_iss_shot"] = timed(lambda: ok(L.mvr_cloud_shot_at(h, 0, kp, len(key), 0, C.byref(sp_), None, None, None, None, None)))
                out[nm + "_iss_fpfh"] = timed(lambda: ok(L.mvr_cloud_fpfh_at(h, 0, kp, len(key), 0, C.byref(fpp), None, None)))
                if with_pfh(r):
                    out[nm + "_iss_pfh"] = timed(lambda: ok(L.mvr_cloud_pfh_at(h, 0, kp, len(key), 0, C.byref(pp), None, None, None)))
                nb = ctx.shot_at(0, 0, r, indices=key[:2000], return_neighbors=True)[1]
                out[nm + "_neighbours"] = round(float(nb.mean()), 1)
                save()

        sp = mvr.synth_params(a.views, 3)
        if a.section == "view":
            ctx.upload(0, mvr.synth_view(sp, 0, a.n))
            cloud_section("1x%dk" % (a.n // 1000), (2.5, 5.0), lambda r: True)
        elif a.section == "object":
            piv, ax = mvr.synth_prior(sp)
            posed = []
            for v in range(a.views):
                ctx.upload(2, mvr.synth_view(sp, v, a.n))
                ctx.transform(2, 2, mvr.axis_rotation(piv, ax, mvr.turntable_angle(v, a.views)))
                posed.append(ctx.download(2))
            ctx.upload(0, np.concatenate(posed))
            cloud_section("%dx%dk" % (a.views, a.n // 1000), (2.5,), lambda r: True)
        elif a.section == "match":
            rng = np.random.default_rng(1)
            for dim in (33, 125, 352):
                q = rng.uniform(0, 1, (5000, dim)).astype(np.float32)
                t = rng.uniform(0, 1, (5000, dim)).astype(np.float32)
                ts = []
                ctx.feature_knn(q, t, 2)
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    ctx.feature_knn(q, t, 2)                     # (host tables in and out: wall ms)
                    ts.append((time.perf_counter() - t0) * 1e3)
                out["match_%d" % dim] = [round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)]
        else:
            import align_cases as AC
            s_raw, t_raw = AC.recovery_view(mvr)
            for slot, raw in ((3, s_raw), (4, t_raw)):
                ctx.upload(slot, raw)
                ctx.voxel_grid(slot, slot, AC.REC_LEAF)
                ctx.estimate_normals(slot, radius=AC.REC_NORMAL_RADIUS)
            s = ctx.download(3)
            inv = np.linalg.inv(AC.REC_POSE.astype(np.float64))
            y = s[:, :3].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
            r = AC.REC_FPFH_RADIUS
            out["align_points"] = [ctx.size(3), ctx.size(4)]
            for name, rows in (("fpfh", lambda sl: ctx.fpfh(sl, r)), ("pfh", lambda sl: ctx.pfh(sl, radius=r)), ("shot20", lambda sl: ctx.shot(sl, r)),
                               ("shot", lambda sl: ctx.shot(sl, 2.0 * r))):
                rows(3)
                t0 = time.perf_counter()
                tabs = [rows(3), rows(4)]
                out["align_%s_descriptors" % name] = round((time.perf_counter() - t0) * 1e3, 3)
                ctx.align_prerejective(3, 4, tabs[0], tabs[1], **dict(AC.REC_PARAMS, max_iterations=100))      # warm
                res = ctx.align_prerejective(3, 4, tabs[0], tabs[1], **AC.REC_PARAMS)
                x = s[:, :3].astype(np.float64) @ res["T"][:3, :3].astype(np.float64).T + res["T"][:3, 3].astype(np.float64)
                out["align_%s_phases" % name] = [round(ctx.stat("prerej_%s_ms" % ph), 3) for ph in ("match", "hypotheses", "score")]
                out["align_%s_result" % name] = dict(converged=int(res["converged"]), inliers=int(res["inliers"]), scored=int(res["scored"]),
                                                     worst_displacement_mm=round(float(np.linalg.norm(x - y, axis=1).max()), 3))
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
