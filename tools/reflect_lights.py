#!/usr/bin/env python3
"""What reflections under several lights cost on the bench workload.

    python tools/reflect_lights.py [-o profiles/reflect_lights.json] [--depth 3]

The bench setting: crash 1 M triangles at 1920x1080, uniform grid 128x128x64, on the one-stream renderer with waiting
builds -- the only frame the lights run in.  The lights are the scene's own and its eye moved by a third of the scene's
extent along +x, +y, -x (tools/lights.py).  One process.
  (a) Per level 1..depth of one finished frame and L = 1..4: ugrt_trace_dda_any_lights against
      L x (ugrt_occlusion_rays + ugrt_trace_dda_any) on the same hits, the two sides in turn; median, min and max over
      `launches` launches after `warm` warm-ups, from the stage profiler (worklist + reflect_gen + trace_dda: the fused
      side's single ugrt_occlusion_rays is counted with it).  The flags of the two sides are compared.
  (b) ugrt_shade_reflect_lights against L x (ugrt_shade_reflect_depth_occluded + ugrt_shade_add_shadows), stage shade.
      The composed side has no kernel that averages its L images: that pass is not counted.
  (c) The whole frame at L = 1..4, depth 1 and `depth`, with and without reflect_shadows: `steps` frames back to back
      between two events, the forms in turn, `repeats` rounds after a warm-up round.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="triangle-count scale of the scene (1.0 = the bench's)")
    a = ap.parse_args()
    import importlib

    import torch

    import bench
    from lights import lights_for

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    s = bench.load_scene(ugrt, "crash", a.scale, 0)
    W, H, lg, ud, D, LMAX = 1920, 1080, (128, 128), (128, 128, 64), a.depth, 4
    N = W * H
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    lights = lights_for(s, LMAX)
    out = {"workload": "crash %d triangles, %dx%d, uniform grid 128x128x64, shadows + reflections of depth %d, one-stream "
                       "renderer, waiting builds" % (len(s["faces"]), W, H, D),
           "launches": a.launches, "warm": a.warm, "steps": a.steps, "repeats": a.repeats}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    setups = {L: ugrt.FrameSetup.from_scene(s, lights=lights[:L]) for L in range(1, LMAX + 1)}
    kw = dict(shadows=True, reflect=True, reflect_lights=True)
    r.display(setups[LMAX], bounces=D, reflect_shadows=True, **kw)
    ctx.synchronize()
    eyes = [tuple(float(x) for x in ugrt.renderer.make_camera(p, setups[1].fovy, r.aspect).worldori[:3]) for p, _ in lights]
    pos = [p for _, p in lights]
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    frame_flags = r.occluded_lights.clone()  # [D, LMAX, N]

    # ---- (a) the any-hit walks, level by level, on the hits of the finished frame
    ctx.prof_enable(True, stages=["worklist", "reflect_gen", "trace_dda"])
    out["walk_ms"] = {}
    orays, oactive = r.occlusion_rays, r.occlusion_active
    fused_occ = torch.empty((LMAX, N), dtype=torch.int32, device=ctx.device)
    single_occ = torch.empty((LMAX, N), dtype=torch.int32, device=ctx.device)
    for j in range(D):
        lv = (r.rays_levels[j], r.active_levels[j], r.hit_t_levels[j], r.hit_id_levels[j], r.d_verts, r.d_faces)
        row = {}
        for L in range(1, LMAX + 1):
            def fused():
                ctx.occlusion_rays(*lv, eyes[0], r.reflect_eps, orays, oactive)
                ctx.trace_dda_any_lights(uvalue, uspan, uoffset, r.d_verts, r.d_faces, orays, oactive, eyes[:L], fused_occ[:L])

            def composed():
                for l in range(L):
                    ctx.occlusion_rays(*lv, eyes[l], r.reflect_eps, orays, oactive)
                    ctx.trace_dda_any(uvalue, uspan, uoffset, r.d_verts, r.d_faces, orays, oactive, 1.0, single_occ[l])

            t = {"fused": [], "composed": []}
            n = {}
            for k in range(a.warm + a.launches):
                for name, call in (("fused", fused), ("composed", composed)):
                    ctx.prof_reset()
                    call()
                    ctx.synchronize()
                    p = ctx.prof_get()
                    n[name] = sum(p[st][1] for st in ("worklist", "reflect_gen", "trace_dda"))
                    if k >= a.warm:
                        t[name].append(sum(p[st][0] for st in ("worklist", "reflect_gen", "trace_dda")))
            e = {name: dict(spread(v), timed_stages=n[name]) for name, v in t.items()}
            e["fused_over_composed"] = round(e["fused"]["median"] / e["composed"]["median"], 3)
            e["flags_agree"] = bool(torch.equal(fused_occ[:L], single_occ[:L]) and torch.equal(fused_occ[:L], frame_flags[j, :L]))
            e["occluded_per_light"] = [int(x) for x in fused_occ[:L].sum(1).tolist()]
            row["lights_%d" % L] = e
            print(json.dumps({"level": j + 1, "lights": L, **e}), flush=True)
        row["occlusion_rays"] = int(oactive.sum())
        out["walk_ms"]["level_%d" % (j + 1)] = row

    # ---- (b) the shading, on the arrays of the finished frame
    ctx.prof_enable(True, stages=["shade"])
    # (the shading rewrites the triangle ids to material indices: the camera pass and the shadow stages once more, without
    # the shading, leave the ids as the shading kernels expect them and every other array of the frame as it is)
    r.display(setups[LMAX], bounces=D, reflect_shadows=True, shade=False, **kw)
    ctx.synchronize()
    ids0 = r.intersect_id.clone()
    out["shade_ms"] = {}
    levels = (r.rays_levels, r.active_levels, r.hit_t_levels, r.hit_id_levels)
    head = (r.image, r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.d_matlist, r.d_reflect, r.num_materials,
            r.d_verts, r.d_faces, D) + levels
    per_light = [frame_flags[:, l].contiguous() for l in range(LMAX)]  # [D, N] per light, as the single-light call takes them
    for L in range(1, LMAX + 1):
        occ_L = frame_flags[:, :L].contiguous()

        def fused():
            ctx.shade_reflect_lights(*head, pos[:L], r.shadowed_lights, occ_L)

        def composed():
            for l in range(L):
                if l:
                    r.intersect_id.copy_(ids0)  # (a device copy outside the timed stage)
                ctx.set_light_position(pos[l])
                ctx.shade_reflect_depth_occluded(*head, per_light[l])
                ctx.shade_add_shadows(r.image, r.shadowed_lights[l])

        row = {}
        t = {"fused": [], "composed": []}
        for k in range(a.warm + a.launches):
            for name, call in (("fused", fused), ("composed", composed)):
                r.intersect_id.copy_(ids0)
                ctx.prof_reset()
                call()
                ctx.synchronize()
                v, n = ctx.prof_get()["shade"]
                row[name + "_launches"] = n
                if k >= a.warm:
                    t[name].append(v)
        row.update({name: spread(v) for name, v in t.items()})
        row["fused_over_composed"] = round(row["fused"]["median"] / row["composed"]["median"], 3)
        out["shade_ms"]["lights_%d" % L] = row
        print(json.dumps({"shade": L, **row}), flush=True)
    ctx.prof_enable(False)

    # ---- (c) the frame
    stream = torch.cuda.current_stream()

    def frames(L, depth, rs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            r.display(setups[L], bounces=depth, reflect_shadows=rs, **kw)
        e1.record(stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    forms = [(L, depth, rs) for depth in sorted({1, D}) for rs in (False, True) for L in range(1, LMAX + 1)]
    ms = {f: [] for f in forms}
    for rnd in range(a.repeats + 1):  # round 0 warms every form up
        for f in forms:
            v = frames(*f)
            if rnd:
                ms[f].append(v)
    out["frame_ms"] = {"depth_%d%s_lights_%d" % (depth, "_reflect_shadows" if rs else "", L): spread(ms[(L, depth, rs)])
                       for (L, depth, rs) in forms}
    print(json.dumps({"frame_ms": out["frame_ms"]}), flush=True)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
