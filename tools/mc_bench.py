"""Timing of the surface reconstruction (mvr_cloud_marching_cubes_hoppe) by stage.  There is no time bar: the numbers are what
they are.

Merges its keys into ONE JSON line in --out (default profiles/mc_bench.json) and prints them.  One --section per process, so that
a caller can put every section under a time limit of its own and chain them:
  view    a 200k view                        object  the twelve posed views concatenated (2.4 M), their analytic normals
  cross   the view at res 64: the capped walk (tune mc_route 1) beside the culled (2) and the tiled (3) search for caps of 1..32 voxels
Per cloud and res in --res (default 128 256 512), without dist_ignore (the culled search over slabs of the lattice) and with
dist_ignore = (3 voxels)^2 (the capped walk of the cloud's own grid):
  <cloud>_res<r>[_cap]_ms         wall ms of one call by stage (tune mc_clock: the call waits after each stage), after a warm-up
                                  at res 16: [search, values, classify + scan, emit, weld, copies home]; welded, grid not copied
  <cloud>_res<r>[_cap]_triangles  T, and _vertices the welded count
  <cloud>_res<r>_tiled_search_ms  the search stage of the same uncapped call through the tiled exact search (mc_route 3)
  <cloud>_res<r>_nn_ms            wall ms of mvr_nn for as many uniformly random queries in the lattice's box (outputs NULL; the
                                  culled search; queries uploaded before the clock starts), beside the search stage
A configuration whose tiled search would take more than --max-pairs point pairs (default 1e13, a few seconds) is not run through
it and is listed under "skipped" as <cloud>_res<r>_tiled.
Usage: python tools/mc_bench.py --section view [--res 128 256 512] [--n 200000] [--views 12] [--out profiles/mc_bench.json]
The whole run, every GPU step under a time limit of its own, the next only after the last ended well:
  timeout -k 10 200 python tools/mc_bench.py --section view && timeout -k 10 100 python tools/mc_bench.py --section cross && \\
  timeout -k 10 400 python tools/mc_bench.py --section object
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

STAGES = ("search", "values", "classify", "emit", "weld", "copy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("view", "object", "cross"), required=True)
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--max-pairs", type=float, default=1e13)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_bench.json"))
    a = ap.parse_args()
    import numpy as np
    mvr = importlib.import_module("multi-view-registration_amd")
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.loads(f.readline() or "{}")
    out.update({"n": a.n, "views": a.views})
    out.setdefault("skipped", [])

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")

    with mvr.Context(0) as ctx:
        L, h = mvr._lib, ctx._h
        name = C.create_string_buffer(128)
        L.mvr_device_info(h, name, 128, None, None)
        out["device"] = name.value.decode()
        ctx.tune(mc_clock=1)

        def staged(res, cap, route=0):
            """one call, welded, grid not copied -> (stage ms, T, V, route taken)"""
            ctx.tune(mc_route=route)
            v, t = ctx.marching_cubes_hoppe(0, (res,) * 3, percentage_extend_grid=0.2, dist_ignore=cap, weld=True)
            ctx.tune(mc_route=0)
            return [round(ctx.stat("mc_%s_ms" % s), 3) for s in STAGES], len(t), len(v), int(ctx.stat("mc_route_used"))

        def warm():
            for route in (1, 2, 3):      # code objects, the slot's own grid, the small buffers
                staged(16, 1.0e6, route)

        def cloud_section(tag, pts):
            n = len(pts)
            lo, hi = pts[:, :3].min(0).astype(np.float64), pts[:, :3].max(0).astype(np.float64)
            lo, hi = lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo)
            out[tag + "_points"] = n
            rng = np.random.default_rng(1)
            warm()
            for res in a.res:
                key = "%s_res%d" % (tag, res)
                voxel = float((hi - lo).max()) / res
                ms, T, V, route = staged(res, (3.0 * voxel) ** 2)
                out[key + "_cap_ms"], out[key + "_cap_triangles"], out[key + "_cap_vertices"], out[key + "_cap_route"] = ms, T, V, route
                save()
                ms, T, V, route = staged(res, -1.0)
                out[key + "_ms"], out[key + "_triangles"], out[key + "_vertices"], out[key + "_route"] = ms, T, V, route
                save()
                if float(res) ** 3 * n > a.max_pairs:
                    if key + "_tiled" not in out["skipped"]:
                        out["skipped"].append(key + "_tiled")
                else:
                    out[key + "_tiled_search_ms"] = staged(res, -1.0, 3)[0][0]
                    save()
                if res ** 3 <= 1 << 25:
                    q = np.ones((res ** 3, 4), np.float32)
                    q[:, :3] = rng.uniform(lo, hi, (res ** 3, 3))
                    ctx.upload(1, q)
                    ts = []
                    for _ in range(2):      # the first call builds the queries' index
                        t0 = time.perf_counter()
                        assert L.mvr_nn(h, 1, 0, 0, None, None) == mvr.OK
                        ts.append(round((time.perf_counter() - t0) * 1e3, 3))
                    out[key + "_nn_ms"] = ts[1]
                    ctx.clear(1)
                    save()

        sp = mvr.synth_params(a.views, 3)
        if a.section in ("view", "cross"):
            pts, nrm = mvr.synth_view(sp, 0, a.n, normals=True)
            ctx.upload(0, pts)
            ctx.upload_normals(0, nrm)
            if a.section == "view":
                cloud_section("1x%dk" % (a.n // 1000), pts)
            else:
                res = 64
                warm()
                voxel = float((pts[:, :3].max(0) - pts[:, :3].min(0)).max()) * 1.2 / res
                for k in (1, 2, 4, 8, 16, 32):
                    cap = (k * voxel) ** 2
                    out["cross_res%d_cap%d_walk_search_ms" % (res, k)] = staged(res, cap, 1)[0][0]
                    out["cross_res%d_cap%d_culled_search_ms" % (res, k)] = staged(res, cap, 2)[0][0]
                    out["cross_res%d_cap%d_tiled_search_ms" % (res, k)] = staged(res, cap, 3)[0][0]
                    save()
        else:
            # the registered object: view v turned back by its true angle (points and normals); the true pivot and axis
            posed, normals = [], []
            for v in range(a.views):
                p, m = mvr.synth_view(sp, v, a.n, normals=True)
                T = mvr.axis_rotation(np.array(sp.pivot), np.array(sp.axis), mvr.turntable_angle(v, a.views))
                ctx.upload(2, p)
                ctx.upload_normals(2, m)
                ctx.transform(2, 2, T)
                posed.append(ctx.download(2))
                normals.append(ctx.download_normals(2))
            pts = np.concatenate(posed)
            ctx.clear(2)
            ctx.upload(0, pts)
            ctx.upload_normals(0, np.concatenate(normals))
            cloud_section("%dx%dk" % (a.views, a.n // 1000), pts)
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
