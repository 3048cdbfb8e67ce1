#!/usr/bin/env python3
"""What the indirect diffuse light costs on the bench workload, and what the single launch saves over the composition of
the calls that existed.

    python tools/indirect.py [-o profiles/indirect.json] [--workload hall]

The setting and the method of tools/ambient_sets.py: crash 1 M triangles at 1920x1080, uniform grid 128x128x64, the
one-stream renderer with waiting builds, one process.  --workload hall: the bench's other scene.  On the primary hits of
one finished frame, per S = 4, 8 and 16, per radius (5 % of the scene's largest extent, and +inf) and with and without
the shadow phase, in turn, each between two events on the stream; median, min and max over `launches` launches after
`warm` warm-ups:
  (a) ugrt_gi_gather, one set;
  (b) the composition on the same rays {o, D_s} (formed here with torch in fp32 and uploaded per direction, which is not
      timed): S times ugrt_trace_dda and, with the shadow phase, S times ugrt_occlusion_rays + ugrt_trace_dda_any.  The
      composition has no radius: its closest-hit walk is the +inf one at either radius.  It leaves out the shading of
      the S levels and the sum, which ugrt_gi_gather includes: the comparison favours the composition;
  (c) ugrt_gi_gather with the sixteen turned sets;
and ugrt_gi_filter of radius 2 (cosine 0.9, plane 1 % of the extent) over the S = 8 sums, and ugrt_gi_apply.
  (d) the frame with gi=8, gi_sets=16, gi_filter=2 against the frame without (call for call the frame as it was before
      the option existed): `steps` frames back to back between two events, the forms in turn, `repeats` rounds after a
      warm-up round.
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
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="triangle-count scale of the scene (1.0 = the bench's)")
    ap.add_argument("--workload", choices=("crash", "hall"), default="crash")
    a = ap.parse_args()
    import importlib

    import numpy as np
    import torch

    import bench

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    rmod = importlib.import_module("uniformgrid-raytracing_amd.renderer")
    s = bench.load_scene(ugrt, a.workload, a.scale, 0)
    W, H, lg, ud = 1920, 1080, (128, 128), (128, 128, 64)
    N = W * H
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    v = np.asarray(s["verts"], np.float32).reshape(-1, 3)
    extent = float((v.max(0) - v.min(0)).max())
    radii = {"5_percent": float(np.float32(0.05 * extent)), "inf": float("inf")}
    plane = rmod.default_filter_plane(v.min(0), v.max(0))
    out = {"workload": "%s %d triangles, %dx%d, uniform grid 128x128x64, one-stream renderer, waiting builds"
                       % (a.workload, len(s["faces"]), W, H),
           "radii": {k: (v_ if v_ != float("inf") else "inf") for k, v_ in radii.items()}, "filter_cos": 0.9,
           "filter_plane": plane, "launches": a.launches, "warm": a.warm, "steps": a.steps, "repeats": a.repeats}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    setup = ugrt.FrameSetup.from_scene(s)
    r.display(setup, shadows=True, gi=8)          # builds the uniform grid, allocates the buffers
    r.display(setup, shadows=True, shade=False)   # the ids are triangle ids again
    ctx.synchronize()
    ctx.ao_rays(r.cam_pos, r.t, r.dir, r.intersect_id, r.d_verts, r.d_faces, r.reflect_eps, r.ao_rays, r.ao_active)
    ctx.synchronize()
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    stream = torch.cuda.current_stream()
    orays, oactive = r.ao_rays, r.ao_active
    light = tuple(float(x) for x in rmod.make_camera(setup.light_camera, setup.fovy, r.aspect).worldori[:3])
    f32, i32 = torch.float32, torch.int32

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def explicit(local):
        """[6N] rays {o, D} of one local direction over the stored normals (the kernel's basis rule, in torch fp32)."""
        o, n = orays.view(N, 6)[:, :3], orays.view(N, 6)[:, 3:]
        axis = n.abs().argmin(1)  # (the first of equal minima)
        e = torch.nn.functional.one_hot(axis, 3).to(f32)
        T = torch.cross(n, e, dim=1)
        T = T / T.norm(dim=1, keepdim=True).clamp(min=1e-30)
        B = torch.cross(n, T, dim=1)
        D = (float(local[0]) * T + float(local[1]) * B) + float(local[2]) * n
        return torch.cat([o, D], 1).contiguous().view(-1)

    sums, acc = (torch.zeros(4 * N, dtype=i32, device=ctx.device) for _ in range(2))
    hit_t, occ_rays = torch.empty(N, dtype=f32, device=ctx.device), torch.empty(6 * N, dtype=f32, device=ctx.device)
    hit_id, occ_act, occ = (torch.empty(N, dtype=i32, device=ctx.device) for _ in range(3))

    def gather(S, tile, table, radius, shadow):
        ctx.gi_gather(uvalue, uspan, uoffset, r.d_verts, r.d_faces, orays, oactive, S, tile, tile, table, radius, r.d_matidx,
                      r.d_matlist, r.num_materials, light if shadow else None, r.reflect_eps, sums)

    def composed(rays, shadow):
        for d_rays in rays:
            ctx.trace_dda(uvalue, uspan, uoffset, r.d_verts, r.d_faces, d_rays, oactive, hit_t, hit_id)
            if shadow:
                ctx.occlusion_rays(d_rays, oactive, hit_t, hit_id, r.d_verts, r.d_faces, light, r.reflect_eps, occ_rays, occ_act)
                ctx.trace_dda_any(uvalue, uspan, uoffset, r.d_verts, r.d_faces, occ_rays, occ_act, 1.0, occ)

    out["gather_ms"] = {}
    for S in (4, 8, 16):
        dirs = ugrt.scenes.ao_directions(S)
        d_one = ctx.upload(dirs.reshape(-1))
        d_sets = ctx.upload(ugrt.scenes.ao_direction_sets(S, 16).reshape(-1))
        rays = [explicit(d) for d in dirs]
        calls = {}
        for rname, radius in radii.items():
            for shadow in (True, False):
                tag = "%s_%s" % (rname, "shadow" if shadow else "plain")
                calls["gather_" + tag] = lambda radius=radius, shadow=shadow: gather(S, 1, d_one, radius, shadow)
                calls["gather_sets_" + tag] = lambda radius=radius, shadow=shadow: gather(S, 4, d_sets, radius, shadow)
        for shadow in (True, False):
            calls["composed_%s" % ("shadow" if shadow else "plain")] = lambda shadow=shadow: composed(rays, shadow)
        if S == 8:
            calls["filter_2"] = lambda: ctx.gi_filter(sums, orays, oactive, 2, 0.9, plane, acc)
            calls["apply"] = lambda: ctx.gi_apply(r.image, acc, 8, 0.0, r.intersect_id, r.d_matlist, r.num_materials)
        t = {name: [] for name in calls}
        for k in range(a.warm + a.launches):
            for name, call in calls.items():
                ms = timed(call)
                if k >= a.warm:
                    t[name].append(ms)
        e = {name: spread(ms) for name, ms in t.items()}
        for rname in radii:
            for kind in ("shadow", "plain"):
                g, c = e["gather_%s_%s" % (rname, kind)], e["composed_%s" % kind]
                e["composed_over_gather_%s_%s" % (rname, kind)] = round(c["median"] / g["median"], 3)
                # the single launch wins beyond the spread when its slowest launch is quicker than the composition's quickest
                e["gather_wins_beyond_spread_%s_%s" % (rname, kind)] = bool(g["max"] < c["min"])
        out["gather_ms"]["S_%d" % S] = e
        print(json.dumps({"S": S, "gather_ms": e}), flush=True)
        del rays

    def frames(kw):
        def run():
            for _ in range(a.steps):
                r.display(setup, shadows=True, **kw)
        return timed(run) / a.steps

    kinds = {"no_gi": dict(), "gi_8_sets_16_filter_2": dict(gi=8, gi_sets=16, gi_filter=2),
             "gi_8_sets_16_filter_2_5_percent": dict(gi=8, gi_sets=16, gi_filter=2, gi_radius=radii["5_percent"])}
    ms = {k: [] for k in kinds}
    for rnd in range(a.repeats + 1):  # round 0 warms every form up
        for k, kw in kinds.items():
            t_ = frames(kw)
            if rnd:
                ms[k].append(t_)
    out["frame_ms"] = {k: spread(v_) for k, v_ in ms.items()}
    print(json.dumps({"frame_ms": out["frame_ms"]}), flush=True)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
