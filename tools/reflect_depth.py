#!/usr/bin/env python3
"""What reflections of depth D cost on the bench workload (DESIGN.md sections 6 and 8).

    python tools/reflect_depth.py [-o profiles/reflect_depth.json] [--depths 1,2,3,4,8]

The bench setting: crash 1 M triangles at 1920x1080, two streams per renderer fed by one host thread, four renderers
in flight, the bounce's launch options of bench.py.  For each depth D:
  - ms per frame from hipEvents around `steps` frames dealt round-robin (after a warm-up), `repeats` times
    (median, min, max);
  - active rays per level (renderer 0's last frame);
  - ms of each level's trace_dda from the stage profiler, in a separate run on one plain context that traces the
    levels of a finished frame again in frame order: with split walks at every level, each launch cut by the history
    of the level before it and level 1 by that of level D ("split_history_across_levels"), and with the split walks
    off for levels >= 2 ("no_history_after_level_1": what a frame does, ugrt_reflect_rays_next tells the
    trace_dda behind it);
  - every renderer's last frame (image, ids, every level) against one sequential single-context frame.
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--depths", default="1,2,3,4,8")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import importlib

    import torch

    import bench

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    s = bench.load_scene(ugrt, "crash", 1.0, 0)
    setup = ugrt.FrameSetup.from_scene(s)
    W, H, lg, ud = 1920, 1080, (128, 128), (128, 128, 64)
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    main_stream = torch.cuda.current_stream()
    out = {"workload": "crash 1M triangles, 1920x1080, shadows + reflections, 4 renderers x 2 streams in flight",
           "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "depths": {}}
    for D in [int(x) for x in a.depths.split(",")]:
        rs = []
        for i in range(4):
            stream = torch.cuda.Stream() if i else None
            with torch.cuda.stream(stream):
                cx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
                rr = ugrt.Renderer(cx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], overlap=True,
                                   helper_thread=False)
            rr._stream = stream
            rr.aux.set_option("dda_blocks", bench.DDA_WAVES_THROUGHPUT)
            rr.aux.set_option("dda_rays_per_wave", bench.DDA_RPW_THROUGHPUT)
            rr.aux.set_option("dda_split", bench.DDA_SPLIT_THROUGHPUT)
            rr.ctx.set_option("shadow_waves", bench.SHADOW_WAVES_THROUGHPUT)
            rs.append(rr)
        turn = [0]

        def step():
            rr = rs[turn[0] % len(rs)]
            turn[0] += 1
            with torch.cuda.stream(rr._stream):
                rr.display(setup, frame_cnt=1, shadows=True, reflect=True, bounces=D)

        def drain():
            for rr in rs:
                rr.synchronize()
            torch.cuda.synchronize()

        for _ in range(max(a.warmup, 8)):
            step()
        drain()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main_stream)
            for rr in rs[1:]:
                rr._stream.wait_stream(main_stream)
            for _ in range(a.steps):
                step()
            for rr in rs[1:]:
                main_stream.wait_stream(rr._stream)
            e1.record(main_stream)
            drain()
            times.append(e0.elapsed_time(e1) / a.steps)
        r0 = rs[0]
        if D > 1:
            active = [int(x) for x in r0.active_levels[:D].sum(1).tolist()]
            hits = [int(x) for x in (r0.hit_id_levels[:D] >= 0).sum(1).tolist()]
        else:
            active, hits = [int(r0.active.sum())], [int((r0.hit_id >= 0).sum())]
        # verification: one sequential context, one stream, builds that wait
        fctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
        fr = ugrt.Renderer(fctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
        fr.display(setup, frame_cnt=1, shadows=True, reflect=True, bounces=D)
        fctx.synchronize()
        names = ["image", "intersect_id", "is_shadowed"] + (
            ["rays_levels", "active_levels", "hit_t_levels", "hit_id_levels"] if D > 1 else ["rays", "active", "hit_t", "hit_id"])
        bad = [[n for n in names if not torch.equal(getattr(fr, n).view(torch.uint8), getattr(rr, n).view(torch.uint8))]
               for rr in rs]
        # per-level trace_dda from the stage profiler: the levels of fr's frame traced again, in frame order
        uvalue, uspan, uoffset, _ = fctx.grid_ptrs(ugrt.GRID_UNIFORM)
        R = [fr.rays_levels[j] for j in range(D)] if D > 1 else [fr.rays]
        A = [fr.active_levels[j] for j in range(D)] if D > 1 else [fr.active]
        T = [torch.empty_like(fr.t) for _ in range(D)]
        I = [torch.empty_like(fr.intersect_id) for _ in range(D)]
        fctx.prof_enable(True, stages=["trace_dda"])
        per_level = {}
        for mode in ("split_history_across_levels", "no_history_after_level_1"):
            ms = [[] for _ in range(D)]
            for _ in range(a.repeats + 1):
                for j in range(D):
                    fctx.set_option("dda_split", 0 if (mode != "split_history_across_levels" and j > 0) else 1)
                    fctx.prof_reset()
                    fctx.trace_dda(uvalue, uspan, uoffset, fr.d_verts, fr.d_faces, R[j], A[j], T[j], I[j])
                    fctx.synchronize()
                    ms[j].append(fctx.prof_get()["trace_dda"][0])
            per_level[mode] = [round(statistics.median(m[1:]), 4) for m in ms]
        fctx.set_option("dda_split", 1)
        same_hits = all(torch.equal(I[j], (fr.hit_id_levels[j] if D > 1 else fr.hit_id)) for j in range(D))
        out["depths"][str(D)] = {
            "ms_per_frame": round(statistics.median(times), 4), "ms_per_frame_min": round(min(times), 4),
            "ms_per_frame_max": round(max(times), 4), "active_rays_per_level": active, "hits_per_level": hits,
            "trace_dda_ms_per_level": per_level, "retraced_levels_equal": same_hits,
            "verified": all(not b for b in bad) and same_hits}
        if any(bad):
            out["depths"][str(D)]["mismatches_per_renderer"] = bad
        print(json.dumps({D: out["depths"][str(D)]}), flush=True)
        for rr in rs:
            rr.close()
        del rs, fr, fctx
        gc.collect()
        torch.cuda.synchronize()
    base = out["depths"].get("1", {}).get("ms_per_frame")
    if base:
        for d in out["depths"].values():
            d["x_depth_1"] = round(d["ms_per_frame"] / base, 3)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
