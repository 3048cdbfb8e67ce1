#!/usr/bin/env python3
"""What the pixel-major hemisphere walk, interleaved direction sets and the gather cost and gain on the bench workload
(DESIGN.md section 6.9).

    python tools/ambient_sets.py [-o profiles/ambient_sets.json] [--workload hall]

The setting and the method of tools/area_sets.py: crash 1 M triangles at 1920x1080, uniform grid 128x128x64, the
one-stream renderer with waiting builds, one process; the radii are 2 % and 5 % of the scene's largest extent.
--workload hall: the bench's other scene.  On the primary hits of one finished frame, per radius and S = 4, 8 and 16,
the calls in turn, each between two events on the stream; median, min and max over `launches` launches after `warm`
warm-ups:
  (a) ugrt_trace_dda_any_hemi_sets with a 1 x 1 tile against ugrt_trace_dda_any_hemi along the same directions, and
      whether their masks are equal: the pixel-major order alone;
  (b) the 4 x 4 tile with sixteen copies of set 0 against the 1 x 1 tile: what the table, its copy and k(p) cost;
  (c) the 4 x 4 tile with the 16 turned sets against the 1 x 1 tile: the sets' spread;
and the gather of radius 2 over the S = 8 masks (ugrt_filter_visibility, cosine 0.9, plane 1 % of the extent).
  (d) the frames ao=4 and ao=8 with ao_sets=16, ao_filter=2 against ao=8, ao=16 and ao=32 as they were: `steps` frames
      back to back between two events, the forms in turn, `repeats` rounds after a warm-up round; and the mean absolute
      error of the open share over the partly occluded hit pixels of a 16 x 32-direction mask computed here on the GPU
      (16 launches of ugrt_trace_dda_any_hemi along the 16 turned sets of 32).
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
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
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
    radii = {"2_percent": float(np.float32(0.02 * extent)), "5_percent": float(np.float32(0.05 * extent))}
    plane = rmod.default_filter_plane(v.min(0), v.max(0))
    out = {"workload": "%s %d triangles, %dx%d, uniform grid 128x128x64, one-stream renderer, waiting builds"
                       % (a.workload, len(s["faces"]), W, H),
           "radii": radii, "filter_cos": 0.9, "filter_plane": plane, "launches": a.launches, "warm": a.warm, "steps": a.steps,
           "repeats": a.repeats}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    setup = ugrt.FrameSetup.from_scene(s)
    r.display(setup, shadows=True, ao=8, ao_radius=radii["2_percent"])  # builds the uniform grid
    r.display(setup, shadows=True, shade=False)                         # the ids are triangle ids again
    ctx.synchronize()
    ctx.ao_rays(r.cam_pos, r.t, r.dir, r.intersect_id, r.d_verts, r.d_faces, r.reflect_eps, r.ao_rays, r.ao_active)
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    stream = torch.cuda.current_stream()
    orays, oactive = r.ao_rays, r.ao_active
    hit = oactive != 0

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def new_mask():
        return torch.empty(N, dtype=torch.int32, device=ctx.device)

    def hemi(dirs, radius, mask):
        ctx.trace_dda_any_hemi(uvalue, uspan, uoffset, r.d_verts, r.d_faces, orays, oactive, dirs, radius, mask)

    def sets(S, tile, table, radius, mask):
        ctx.trace_dda_any_hemi_sets(uvalue, uspan, uoffset, r.d_verts, r.d_faces, orays, oactive, S, tile, tile, table, radius, mask)

    def opens(mask, S):
        """open directions per pixel of an int32 mask tensor."""
        m = mask.to(torch.int64) & ((1 << S) - 1)
        dark = torch.zeros_like(m)
        for b in range(S):
            dark += (m >> b) & 1
        return S - dark

    def gathered(mask, S, R):
        vis = torch.zeros(2 * N, dtype=torch.int32, device=ctx.device)
        ctx.filter_visibility(mask, S, orays, oactive, R, 0.9, plane, vis)
        ctx.synchronize()
        num, den = vis[0::2].to(torch.float64), vis[1::2].to(torch.float64)
        return num / (S * den.clamp(min=1))

    out["walk_ms"], out["error"] = {}, {}
    vis = torch.zeros(2 * N, dtype=torch.int32, device=ctx.device)
    for rname, radius in radii.items():
        # ---- (a), (b), (c): the calls in turn
        calls, masks = {}, {}
        for S in (4, 8, 16):
            dirs = ugrt.scenes.ao_directions(S)
            d_one = ctx.upload(dirs.reshape(-1))
            d_same = ctx.upload(np.tile(dirs.reshape(-1), 16))
            d_sets = ctx.upload(ugrt.scenes.ao_direction_sets(S, 16).reshape(-1))
            for form in ("hemi", "one", "same", "sets"):
                masks["%s_%d" % (form, S)] = new_mask()
            calls["hemi_%d" % S] = lambda S=S, dirs=dirs: hemi(dirs, radius, masks["hemi_%d" % S])
            calls["one_%d" % S] = lambda S=S, t=d_one: sets(S, 1, t, radius, masks["one_%d" % S])
            calls["same_%d" % S] = lambda S=S, t=d_same: sets(S, 4, t, radius, masks["same_%d" % S])
            calls["sets_%d" % S] = lambda S=S, t=d_sets: sets(S, 4, t, radius, masks["sets_%d" % S])
        calls["sets_8"]()
        ctx.synchronize()
        calls["gather_2"] = lambda: ctx.filter_visibility(masks["sets_8"], 8, orays, oactive, 2, 0.9, plane, vis)
        t = {name: [] for name in calls}
        for k in range(a.warm + a.launches):
            for name, call in calls.items():
                ms = timed(call)
                if k >= a.warm:
                    t[name].append(ms)
        e = {name: spread(ms) for name, ms in t.items()}
        for S in (4, 8, 16):
            e["one_over_hemi_%d" % S] = round(e["one_%d" % S]["median"] / e["hemi_%d" % S]["median"], 3)
            e["one_equals_hemi_%d" % S] = bool(torch.equal(masks["one_%d" % S], masks["hemi_%d" % S]))
            e["same_over_one_%d" % S] = round(e["same_%d" % S]["median"] / e["one_%d" % S]["median"], 3)
            e["same_equals_one_%d" % S] = bool(torch.equal(masks["same_%d" % S], masks["one_%d" % S]))
            e["sets_over_one_%d" % S] = round(e["sets_%d" % S]["median"] / e["one_%d" % S]["median"], 3)
            e["sets_over_hemi_%d" % S] = round(e["sets_%d" % S]["median"] / e["hemi_%d" % S]["median"], 3)
        out["walk_ms"]["radius_%s" % rname] = e
        print(json.dumps({"radius": rname, "walk_ms": e}), flush=True)
        # ---- (d) the errors against 16 x 32 directions
        truth = torch.zeros(N, dtype=torch.float64, device=ctx.device)
        turned = ugrt.scenes.ao_direction_sets(32, 16)
        m32 = new_mask()
        fixed32 = None
        for k in range(16):
            hemi(turned[k], radius, m32)
            ctx.synchronize()
            o = opens(m32, 32).to(torch.float64)
            fixed32 = o / 32 if k == 0 else fixed32
            truth += o
        truth /= 512
        partly = hit & (truth > 0) & (truth < 1)
        shares = {"fixed_4": opens(masks["hemi_4"], 4).to(torch.float64) / 4,
                  "fixed_8": opens(masks["hemi_8"], 8).to(torch.float64) / 8,
                  "fixed_16": opens(masks["hemi_16"], 16).to(torch.float64) / 16, "fixed_32": fixed32,
                  "sets_4_gather_2": gathered(masks["sets_4"], 4, 2), "sets_8_gather_2": gathered(masks["sets_8"], 8, 2),
                  "sets_8": opens(masks["sets_8"], 8).to(torch.float64) / 8,
                  "fixed_8_gather_2": gathered(masks["hemi_8"], 8, 2)}
        err = {name: round(float((sh[partly] - truth[partly]).abs().mean()), 4) for name, sh in shares.items()}
        err["partly_occluded_pixels"], err["hit_pixels"] = int(partly.sum()), int(hit.sum())
        out["error"]["radius_%s" % rname] = err
        print(json.dumps({"radius": rname, "error": err}), flush=True)

    # ---- (d) the frames
    def frames(kw, radius):
        def run():
            for _ in range(a.steps):
                r.display(setup, shadows=True, ao_radius=radius, **kw)
        return timed(run) / a.steps

    kinds = {"no_ao": dict(), "ao_32": dict(ao=32), "ao_16": dict(ao=16), "ao_8": dict(ao=8),
             "ao_8_sets_16_filter_2": dict(ao=8, ao_sets=16, ao_filter=2),
             "ao_4_sets_16_filter_2": dict(ao=4, ao_sets=16, ao_filter=2)}
    forms = [(kind, rname) for kind in kinds for rname in radii]
    ms = {f: [] for f in forms}
    for rnd in range(a.repeats + 1):  # round 0 warms every form up
        for f in forms:
            t = frames(kinds[f[0]], radii[f[1]])
            if rnd:
                ms[f].append(t)
    out["frame_ms"] = {"%s_radius_%s" % f: spread(ms[f]) for f in forms}
    print(json.dumps({"frame_ms": out["frame_ms"]}), flush=True)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
