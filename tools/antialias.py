#!/usr/bin/env python3
"""What the adaptive anti-aliasing costs on the bench workload, what it buys, and what it saves over the composition of the
calls that existed and over brute supersampling.

    python tools/antialias.py [-o profiles/antialias.json] [--workload hall]

The setting and the method of tools/indirect.py: crash 1 M triangles at 1920x1080, uniform grid 128x128x64, the one-stream
renderer with waiting builds, one process.  --workload hall: the bench's other scene.  On the primary hits and the shadow
flags of one finished frame, per S = 4, 8 and 16, each between two events on the stream; median, min and max over
`launches` launches after `warm` warm-ups:
  (a) ugrt_aa_edges (once: it does not depend on S), ugrt_aa_gather with one set and with sixteen, with and without the
      shadow phase, ugrt_aa_resolve;
  (b) the composition on the same rays {eye, d_s} (formed here on the host in fp32 and uploaded per sample, which is not
      timed): S times ugrt_trace_dda and, with the shadow phase, S times ugrt_occlusion_rays + ugrt_trace_dda_any, with
      d_edge as the active flags.  It leaves out the depth gate, the shading of the S hits and the sum, which
      ugrt_aa_gather includes: the comparison favours the composition;
  (c) the frame with aa = S against the frame without (call for call the frame as it was before the option existed), and
      the plain frame at 3840x2160 -- what brute 2 x 2 supersampling costs before its four pixels are averaged: `steps`
      frames back to back between two events, the forms in turn, `repeats` rounds after a warm-up round;
  (d) the error, the mean absolute byte difference over all pixels against ugrt_aa_gather + ugrt_aa_resolve with EVERY
      pixel flagged at S = 32: of the plain frame and of each aa frame.
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
    out = {"workload": "%s %d triangles, %dx%d, uniform grid 128x128x64, one-stream renderer, waiting builds"
                       % (a.workload, len(s["faces"]), W, H),
           "aa_cos": 0.9, "aa_plane": "1 % of the largest extent", "launches": a.launches, "warm": a.warm, "steps": a.steps,
           "repeats": a.repeats}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    setup = ugrt.FrameSetup.from_scene(s)
    stream = torch.cuda.current_stream()
    f32, i32 = torch.float32, torch.int32

    def timed(call, c=ctx):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        c.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def image_of(**kw):
        r.display(setup, shadows=True, **kw)
        ctx.synchronize()
        return r.image.cpu().numpy().astype(np.int32)

    # (d) first: the images.  The converged image: every pixel flagged, S = 32, on top of the plain frame
    plain = image_of()
    r.display(setup, shadows=True, aa=4)         # builds the uniform grid, allocates the buffers
    r.display(setup, shadows=True, shade=False)  # the ids are triangle ids again; the context holds the light camera's block
    ctx.synchronize()
    cam = rmod.make_camera(setup.camera, setup.fovy, r.aspect)
    eye_cc = np.asarray(cam.camcoords, np.float32).copy()
    light = tuple(float(x) for x in rmod.make_camera(setup.light_camera, setup.fovy, r.aspect).worldori[:3])
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    plane = rmod.default_filter_plane(r.bbmin, r.bbmax)
    ones = torch.ones(N, dtype=i32, device=ctx.device)
    sums = torch.zeros(4 * N, dtype=i32, device=ctx.device)
    t32 = ctx.upload(ugrt.scenes.aa_offsets(32).reshape(-1))
    ctx.aa_gather(uvalue, uspan, uoffset, r.d_verts, r.d_faces, eye_cc, ones, 32, 1, 1, t32, r.d_matidx, r.d_matlist, r.num_materials,
                  light, r.reflect_eps, sums)
    ref_img = ctx.upload(plain.astype(np.uint8))
    ctx.aa_resolve(ref_img, sums, 32)
    ctx.synchronize()
    ref = ref_img.cpu().numpy().astype(np.int32)
    err = lambda img: round(float(np.abs(img - ref).mean()), 4)
    out["error_vs_all_pixels_S32"] = {"plain": err(plain)}
    for S in (4, 8, 16):
        out["error_vs_all_pixels_S32"]["aa_%d" % S] = err(image_of(aa=S))
        out["error_vs_all_pixels_S32"]["aa_%d_sets_16" % S] = err(image_of(aa=S, aa_sets=16))
    out["edge_share"] = round(float((r.aa_edge != 0).sum().item()) / N, 4)
    print(json.dumps({"error": out["error_vs_all_pixels_S32"], "edge_share": out["edge_share"]}), flush=True)

    # (a), (b): the calls, on the arrays of a frame that has not been shaded
    r.display(setup, shadows=True, shade=False)
    ctx.synchronize()
    edge = r.aa_edge
    tex = np.zeros(100, np.float32)
    import ctypes as C

    ugrt.check(ugrt.lib.ugrt_camera_direction_table(ugrt._f3(eye_cc), tex.ctypes.data_as(C.POINTER(C.c_float))))
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))

    def explicit(off):
        """[6N] rays {eye, d} of one sub-pixel offset (d_ray_dir_at's arithmetic in numpy fp32; not the strict rule)."""
        ftx = np.float32(1) - (cols + np.float32(off[0])) / np.float32(W)
        fty = (rows + np.float32(off[1])) / np.float32(H)
        xs, ys = ftx * np.float32(4), fty * np.float32(4)
        i, j = np.minimum(xs.astype(np.int32), 3), np.minimum(ys.astype(np.int32), 3)
        fa, fb = xs - i.astype(np.float32), ys - j.astype(np.float32)
        t4 = tex.reshape(5, 5, 4)
        d = (((1 - fa) * (1 - fb))[..., None] * t4[j, i, :3] + (fa * (1 - fb))[..., None] * t4[j, i + 1, :3]
             + ((1 - fa) * fb)[..., None] * t4[j + 1, i, :3] + (fa * fb)[..., None] * t4[j + 1, i + 1, :3]) - eye_cc[:3]
        d = (d / np.sqrt((d * d).sum(-1, keepdims=True))).astype(np.float32)
        rays = np.concatenate([np.broadcast_to(eye_cc[:3], d.shape), d], -1).astype(np.float32)
        return ctx.upload(rays.reshape(-1))

    hit_t, occ_rays = torch.empty(N, dtype=f32, device=ctx.device), torch.empty(6 * N, dtype=f32, device=ctx.device)
    hit_id, occ_act, occ = (torch.empty(N, dtype=i32, device=ctx.device) for _ in range(3))
    img = torch.zeros(3 * N, dtype=torch.uint8, device=ctx.device)

    def gather(S, tile, table, shadow):
        ctx.aa_gather(uvalue, uspan, uoffset, r.d_verts, r.d_faces, eye_cc, edge, S, tile, tile, table, r.d_matidx, r.d_matlist,
                      r.num_materials, light if shadow else None, r.reflect_eps, sums)

    def composed(rays, shadow):
        for d_rays in rays:
            ctx.trace_dda(uvalue, uspan, uoffset, r.d_verts, r.d_faces, d_rays, edge, hit_t, hit_id)
            if shadow:
                ctx.occlusion_rays(d_rays, edge, hit_t, hit_id, r.d_verts, r.d_faces, light, r.reflect_eps, occ_rays, occ_act)
                ctx.trace_dda_any(uvalue, uspan, uoffset, r.d_verts, r.d_faces, occ_rays, occ_act, 1.0, occ)

    out["calls_ms"] = {}
    for S in (4, 8, 16):
        offs = ugrt.scenes.aa_offsets(S)
        d_one = ctx.upload(offs.reshape(-1))
        d_sets = ctx.upload(ugrt.scenes.aa_offset_sets(S, 16).reshape(-1))
        rays = [explicit(o) for o in offs]
        calls = {}
        if S == 4:
            calls["edges"] = lambda: ctx.aa_edges(r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.is_shadowed, 0.9,
                                                  plane, edge)
        for shadow in (True, False):
            tag = "shadow" if shadow else "plain"
            calls["gather_" + tag] = lambda shadow=shadow: gather(S, 1, d_one, shadow)
            calls["gather_sets_" + tag] = lambda shadow=shadow: gather(S, 4, d_sets, shadow)
            calls["composed_" + tag] = lambda shadow=shadow: composed(rays, shadow)
        calls["resolve"] = lambda: ctx.aa_resolve(img, sums, S)
        t = {name: [] for name in calls}
        for k in range(a.warm + a.launches):
            for name, call in calls.items():
                ms = timed(call)
                if k >= a.warm:
                    t[name].append(ms)
        e = {name: spread(ms) for name, ms in t.items()}
        for kind in ("shadow", "plain"):
            g, c = e["gather_" + kind], e["composed_" + kind]
            e["composed_over_gather_" + kind] = round(c["median"] / g["median"], 3)
            # the single launch wins beyond the spread when its slowest launch is quicker than the composition's quickest
            e["gather_wins_beyond_spread_" + kind] = bool(g["max"] < c["min"])
        out["calls_ms"]["S_%d" % S] = e
        print(json.dumps({"S": S, "calls_ms": e}), flush=True)
        del rays

    # (c) the frames
    def frames(rr, kw):
        def run():
            for _ in range(a.steps):
                rr.display(setup, shadows=True, **kw)
        return timed(run, rr.ctx) / a.steps

    ctx4 = ugrt.Context(2 * W, 2 * H, light_grid=lg, flags=flags, uniform_dims=ud)
    r4 = ugrt.Renderer(ctx4, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    kinds = {"no_aa": (r, dict()), "aa_4": (r, dict(aa=4)), "aa_8": (r, dict(aa=8)), "aa_16": (r, dict(aa=16)),
             "aa_8_sets_16": (r, dict(aa=8, aa_sets=16)), "plain_3840x2160": (r4, dict())}
    ms = {k: [] for k in kinds}
    for rnd in range(a.repeats + 1):  # round 0 warms every form up
        for k, (rr, kw) in kinds.items():
            t_ = frames(rr, kw)
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
