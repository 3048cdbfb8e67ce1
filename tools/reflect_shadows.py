#!/usr/bin/env python3
"""What shadows on reflected hits cost on the bench workload.

    python tools/reflect_shadows.py [-o profiles/reflect_shadows.json] [--depth 3]

The bench setting: crash 1 M triangles at 1920x1080, uniform grid 128x128x64.
  - Per level 1..depth of one finished frame, on one plain context: that level's occlusion rays traced by
    ugrt_trace_dda_any (t_max 1) and, beside it in the same process, by ugrt_trace_dda (default window kernel) --
    the yardstick: a nearest hit with 0 < t < 1 answers the same question.  Median, min and max over `launches`
    launches after `warm` warm-ups, from the stage profiler: "kernel" is stage trace_dda, "call" adds the ray list's
    stage (worklist).  The two answers are compared ray by ray.
  - The same for other launch shapes of the any-hit kernel (rays per wave, cooperative threshold).
  - The whole frame with and without reflect_shadows, alternating, one frame at a time (one two-stream renderer, a
    wait behind every frame) and four renderers in flight (bench.py's setting).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import importlib

    import torch

    import bench

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    s = bench.load_scene(ugrt, "crash", 1.0, 0)
    setup = ugrt.FrameSetup.from_scene(s)
    W, H, lg, ud, D = 1920, 1080, (128, 128), (128, 128, 64), a.depth
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    out = {"workload": "crash 1M triangles, 1920x1080, uniform grid 128x128x64, shadows + reflections of depth %d" % D,
           "launches": a.launches, "warm": a.warm, "steps": a.steps, "repeats": a.repeats, "levels": {}}

    # ---- the kernels, level by level, on the rays of one finished frame
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    fr = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    fr.display(setup, shadows=True, reflect=True, bounces=D, reflect_shadows=True)
    ctx.synchronize()
    light = ugrt.renderer.make_camera(setup.light_camera, setup.fovy, fr.aspect).worldori[:3]
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    ctx.prof_enable(True, stages=["worklist", "trace_dda"])

    def timed(call):
        kernel, whole = [], []
        for k in range(a.warm + a.launches):
            ctx.prof_reset()
            call()
            ctx.synchronize()
            p = ctx.prof_get()
            if k >= a.warm:
                kernel.append(p["trace_dda"][0])
                whole.append(p["trace_dda"][0] + p["worklist"][0])
        return {"kernel_ms": spread(kernel), "call_ms": spread(whole)}

    for j in range(D):
        orays, oactive = torch.empty_like(fr.rays), torch.empty_like(fr.active)
        ctx.occlusion_rays(fr.rays_levels[j], fr.active_levels[j], fr.hit_t_levels[j], fr.hit_id_levels[j], fr.d_verts,
                           fr.d_faces, light, fr.reflect_eps, orays, oactive)
        occ, ht, hid = torch.empty_like(fr.active), torch.empty_like(fr.t), torch.empty_like(fr.active)
        lv = {"occlusion_rays": int(oactive.sum())}
        lv["trace_dda_any"] = timed(lambda: ctx.trace_dda_any(uvalue, uspan, uoffset, fr.d_verts, fr.d_faces, orays,
                                                              oactive, 1.0, occ))
        lv["trace_dda"] = timed(lambda: ctx.trace_dda(uvalue, uspan, uoffset, fr.d_verts, fr.d_faces, orays, oactive,
                                                      ht, hid))
        nearest = ((hid >= 0) & (ht > 0) & (ht < 1)).to(torch.int32)
        lv["occluded"] = int(occ.sum())
        lv["differ_from_the_nearest_hit"] = int((nearest != occ).sum())
        lv["equal_the_frame_s_flags"] = bool(torch.equal(occ, fr.occluded_levels[j]))
        lv["any_over_dda_kernel"] = round(lv["trace_dda_any"]["kernel_ms"]["median"] / lv["trace_dda"]["kernel_ms"]["median"], 3)
        shapes = {}
        for key, v in (("any_rays_per_wave", 8), ("any_rays_per_wave", 16), ("any_rays_per_wave", 64), ("any_coop", 4),
                       ("any_coop", 16), ("any_coop", 64)):
            ctx.set_option(key, v)
            shapes["%s=%d" % (key, v)] = timed(lambda: ctx.trace_dda_any(uvalue, uspan, uoffset, fr.d_verts, fr.d_faces,
                                                                         orays, oactive, 1.0, occ))["kernel_ms"]
            ctx.set_option(key, -1)
        lv["launch_shapes_kernel_ms"] = shapes
        out["levels"][str(j + 1)] = lv
        print(json.dumps({"level": j + 1, **lv}), flush=True)
    del fr, ctx

    # ---- the frame, with and without the option
    main_stream = torch.cuda.current_stream()

    def renderers(n):
        rs = []
        for i in range(n):
            stream = torch.cuda.Stream() if i else None
            with torch.cuda.stream(stream):
                cx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
                rr = ugrt.Renderer(cx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], overlap=True,
                                   helper_thread=False)
            rr._stream = stream
            rr.aux.set_option("dda_blocks", bench.DDA_WAVES_THROUGHPUT if n > 1 else bench.DDA_WAVES_ONE_FRAME)
            if n > 1:
                rr.aux.set_option("dda_rays_per_wave", bench.DDA_RPW_THROUGHPUT)
            rr.aux.set_option("dda_split", bench.DDA_SPLIT_THROUGHPUT)
            rr.ctx.set_option("shadow_waves", bench.SHADOW_WAVES_THROUGHPUT)
            rs.append(rr)
        return rs

    def frames(rs, on, wait):
        """ms per frame over `steps` frames dealt round-robin"""
        def drain():
            for rr in rs:
                rr.synchronize()
            torch.cuda.synchronize()

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(main_stream)
        for rr in rs[1:]:
            rr._stream.wait_stream(main_stream)
        for k in range(a.steps):
            rr = rs[k % len(rs)]
            with torch.cuda.stream(rr._stream):
                rr.display(setup, frame_cnt=1, shadows=True, reflect=True, bounces=D, reflect_shadows=on)
            if wait:
                drain()
        for rr in rs[1:]:
            main_stream.wait_stream(rr._stream)
        e1.record(main_stream)
        drain()
        return e0.elapsed_time(e1) / a.steps

    out["frame_ms"] = {}
    for name, n, wait in (("one_frame_at_a_time", 1, True), ("four_in_flight", 4, False)):
        rs = renderers(n)
        for on in (False, True):  # warm-up of both forms
            frames(rs, on, wait)
        ms = {False: [], True: []}
        for _ in range(a.repeats):
            for on in (False, True):
                ms[on].append(frames(rs, on, wait))
        out["frame_ms"][name] = {"without": spread(ms[False]), "with_reflect_shadows": spread(ms[True])}
        print(json.dumps({name: out["frame_ms"][name]}), flush=True)
        for rr in rs:
            rr.close()
        del rs
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
