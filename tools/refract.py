#!/usr/bin/env python3
"""What refraction costs.

    python tools/refract.py [-o profiles/refract.json] [--depth 4]

scenes.glass grown to roughly the bench workload's triangle count (1 M) at 1920x1080, uniform grid 128x128x64.
  (a) The frame at depth `depth` with reflect_shadows on one plain context, refract=False against refract=True,
      alternating, `steps` frames per sample with a wait behind every frame, `repeats` samples each.
  (b) Per level 1..depth of the finished refract frame: that level's occlusion rays traced by ugrt_trace_dda_any_thru and,
      beside it in the same process, by ugrt_trace_dda_any.  Median, min and max over `launches` launches after `warm`
      warm-ups, from the stage profiler: "kernel" is stage trace_dda, "call" adds the ray list's stage (worklist).
      How many rays each form marks occluded is recorded beside the times: the see-through form walks the rays that
      pass the glass further.
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


def grown_glass(ugrt, target):
    """scenes.glass at the scale whose triangle count comes closest to `target` in three steps."""
    scale = target / float(ugrt.scenes.glass(scale=1.0)["num_faces"])
    s = None
    for _ in range(3):
        s = ugrt.scenes.glass(scale=scale)
        if abs(s["num_faces"] - target) <= 0.05 * target:
            break
        scale *= target / float(s["num_faces"])
    return s, scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import importlib

    import torch

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    s, scale = grown_glass(ugrt, a.triangles)
    setup = ugrt.FrameSetup.from_scene(s)
    W, H, lg, ud, D = 1920, 1080, (128, 128), (128, 128, 64), a.depth
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    out = {"workload": "glass(scale=%.1f): %d triangles, 1920x1080, uniform grid 128x128x64, shadows + levels of depth %d "
                       "with reflect_shadows" % (scale, s["num_faces"], D),
           "launches": a.launches, "warm": a.warm, "steps": a.steps, "repeats": a.repeats}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    fr = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], s["transmit"], s["ior"])
    kw = dict(shadows=True, reflect=True, bounces=D, reflect_shadows=True)

    # ---- (a) the frame, with and without the option
    def frames(on):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fr.display(setup, refract=on, **kw)
            ctx.synchronize()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for on in (False, True):  # warm-up of both forms
        frames(on)
    ms = {False: [], True: []}
    for _ in range(a.repeats):
        for on in (False, True):
            ms[on].append(frames(on))
    out["frame_ms"] = {"refract_false": spread(ms[False]), "refract_true": spread(ms[True])}
    print(json.dumps({"frame_ms": out["frame_ms"]}), flush=True)

    # ---- (b) the two walks on the occlusion rays of the refract frame's levels
    fr.display(setup, refract=True, **kw)
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

    out["levels"] = {}
    for j in range(D):
        orays, oactive = torch.empty_like(fr.rays), torch.empty_like(fr.active)
        ctx.occlusion_rays(fr.rays_levels[j], fr.active_levels[j], fr.hit_t_levels[j], fr.hit_id_levels[j], fr.d_verts,
                           fr.d_faces, light, fr.reflect_eps, orays, oactive)
        plain, thru = torch.empty_like(fr.active), torch.empty_like(fr.active)
        lv = {"occlusion_rays": int(oactive.sum())}
        lv["trace_dda_any"] = timed(lambda: ctx.trace_dda_any(uvalue, uspan, uoffset, fr.d_verts, fr.d_faces, orays, oactive,
                                                              1.0, plain))
        lv["trace_dda_any_thru"] = timed(lambda: ctx.trace_dda_any_thru(uvalue, uspan, uoffset, fr.d_verts, fr.d_faces, orays,
                                                                        oactive, 1.0, thru, fr.d_matidx, fr.d_transmit,
                                                                        fr.num_materials))
        lv["occluded_plain"], lv["occluded_thru"] = int(plain.sum()), int(thru.sum())
        lv["thru_marks_a_ray_the_plain_walk_does_not"] = int(((thru == 1) & (plain == 0)).sum())
        lv["equal_the_frame_s_flags"] = bool(torch.equal(thru, fr.occluded_levels[j]))
        lv["thru_over_plain_kernel"] = round(lv["trace_dda_any_thru"]["kernel_ms"]["median"] /
                                             lv["trace_dda_any"]["kernel_ms"]["median"], 3)
        out["levels"][str(j + 1)] = lv
        print(json.dumps({"level": j + 1, **lv}), flush=True)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
