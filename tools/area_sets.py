#!/usr/bin/env python3
"""What interleaved sample sets and the edge-aware gather cost and gain on the bench workload.

    python tools/area_sets.py [-o profiles/area_sets.json] [--workload hall]

The setting of tools/area_light.py: crash 1 M triangles at 1920x1080, uniform grid 128x128x64, the one-stream renderer
with waiting builds, radii of 2 % and 10 % of the scene's largest extent, one process.  --workload hall: the bench's
other scene.  On the primary hits of one finished frame, per radius:
  (a) the walk over 16 sample sets (ugrt_trace_dda_any_area_sets, tile 4 x 4) against ugrt_trace_dda_any_area at
      S = 4, 8 and 16, the same call with sixteen copies of set 0 (the mechanism without the sets' spread: its words
      are the plain call's), and one sample's walk (S = 1), the calls in turn; median, min and max over `launches` launches
      after `warm` warm-ups, each between two events on the stream;
  (b) the gather (ugrt_filter_visibility, cosine 0.9, plane 1 % of the extent) at R = 1, 2, 4 and 8 over the S = 8 masks
      of the sets, timed the same way, in the same turns as (a);
  (c) the frames area=8, area_sets=16, area_filter=2 and area=4, area_sets=16, area_filter=3 against area=32 and
      area=8 as they were (the default keywords enqueue the calls of the frame before this feature): `steps` frames
      back to back between two events, the forms in turn, `repeats` rounds after a warm-up round;
  (d) the mean absolute error of the lit share over the penumbra pixels of a 16 x 32-sample mask computed here on the
      GPU (16 launches of ugrt_trace_dda_any_area with the 16 turned sets of 32), for fixed S = 8 and 32, the two
      interleaved forms of (c), and the gather over fixed samples.
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
    radii = {"2_percent": float(np.float32(0.02 * extent)), "10_percent": float(np.float32(0.10 * extent))}
    plane = rmod.default_filter_plane(v.min(0), v.max(0))
    out = {"workload": "%s %d triangles, %dx%d, uniform grid 128x128x64, one-stream renderer, waiting builds"
                       % (a.workload, len(s["faces"]), W, H),
           "radii": radii, "filter_cos": 0.9, "filter_plane": plane, "launches": a.launches, "warm": a.warm, "steps": a.steps,
           "repeats": a.repeats}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    setup = ugrt.FrameSetup.from_scene(s)
    eye = np.asarray(setup.light_camera["eye"], np.float64)
    axis = np.asarray(setup.light_camera["look"], np.float64) - eye
    r.display(setup, shadows=True, area=8, area_radius=radii["2_percent"])  # builds the uniform grid
    r.display(setup, shadows=True, shade=False)                             # the ids are triangle ids again
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

    def plain(samples, mask):
        ctx.trace_dda_any_area(uvalue, uspan, uoffset, r.d_verts, r.d_faces, orays, oactive, samples, mask)

    def sets(S, table, mask):
        ctx.trace_dda_any_area_sets(uvalue, uspan, uoffset, r.d_verts, r.d_faces, orays, oactive, S, 4, 4, table, mask)

    def opens(mask, S):
        """open samples per pixel of an int32 mask tensor."""
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

    out["walk_ms"], out["gather_ms"], out["error"] = {}, {}, {}
    vis = torch.zeros(2 * N, dtype=torch.int32, device=ctx.device)
    for rname, radius in radii.items():
        # ---- (a), (b): the calls in turn
        calls, masks = {}, {}
        one = ugrt.scenes.area_samples(1, eye, axis, radius)
        masks["one"] = new_mask()
        calls["plain_1"] = lambda one=one: plain(one, masks["one"])
        for S in (4, 8, 16):
            samples = ugrt.scenes.area_samples(S, eye, axis, radius)
            table = ctx.upload(ugrt.scenes.area_sample_sets(S, 16, eye, axis, radius).reshape(-1))
            masks["plain_%d" % S], masks["sets_%d" % S] = new_mask(), new_mask()
            calls["plain_%d" % S] = lambda S=S, samples=samples: plain(samples, masks["plain_%d" % S])
            calls["sets_%d" % S] = lambda S=S, table=table: sets(S, table, masks["sets_%d" % S])
            # the same call with sixteen copies of set 0: what the table, its copy and k(p) cost without the sets' spread
            same = ctx.upload(np.tile(samples.reshape(-1), 16))
            masks["same_%d" % S] = new_mask()
            calls["same_%d" % S] = lambda S=S, same=same: sets(S, same, masks["same_%d" % S])
        calls["sets_8"]()
        ctx.synchronize()
        for R in (1, 2, 4, 8):
            calls["gather_%d" % R] = lambda R=R: ctx.filter_visibility(masks["sets_8"], 8, orays, oactive, R, 0.9, plane, vis)
        t = {name: [] for name in calls}
        for k in range(a.warm + a.launches):
            for name, call in calls.items():
                ms = timed(call)
                if k >= a.warm:
                    t[name].append(ms)
        e = {name: spread(ms) for name, ms in t.items() if not name.startswith("gather")}
        for S in (4, 8, 16):
            e["sets_over_plain_%d" % S] = round(e["sets_%d" % S]["median"] / e["plain_%d" % S]["median"], 3)
            e["same_over_plain_%d" % S] = round(e["same_%d" % S]["median"] / e["plain_%d" % S]["median"], 3)
            e["same_equals_plain_%d" % S] = bool(torch.equal(masks["same_%d" % S], masks["plain_%d" % S]))
        out["walk_ms"]["radius_%s" % rname] = e
        g = {name: spread(ms) for name, ms in t.items() if name.startswith("gather")}
        for R in (1, 2, 4, 8):
            g["gather_%d_over_one_sample" % R] = round(g["gather_%d" % R]["median"] / e["plain_1"]["median"], 3)
        out["gather_ms"]["radius_%s" % rname] = g
        print(json.dumps({"radius": rname, "walk_ms": e, "gather_ms": g}), flush=True)
        # ---- (d) the errors against 16 x 32 samples
        truth = torch.zeros(N, dtype=torch.float64, device=ctx.device)
        turned = ugrt.scenes.area_sample_sets(32, 16, eye, axis, radius)
        m32 = new_mask()
        fixed32 = None
        for k in range(16):
            plain(turned[k], m32)
            ctx.synchronize()
            o = opens(m32, 32).to(torch.float64)
            fixed32 = o / 32 if k == 0 else fixed32
            truth += o
        truth /= 512
        pen = hit & (truth > 0) & (truth < 1)
        m4s = new_mask()
        sets(4, ctx.upload(ugrt.scenes.area_sample_sets(4, 16, eye, axis, radius).reshape(-1)), m4s)
        ctx.synchronize()
        shares = {"fixed_8": opens(masks["plain_8"], 8).to(torch.float64) / 8, "fixed_32": fixed32,
                  "sets_8_gather_2": gathered(masks["sets_8"], 8, 2), "sets_4_gather_3": gathered(m4s, 4, 3),
                  "fixed_8_gather_2": gathered(masks["plain_8"], 8, 2)}
        err = {name: round(float((sh[pen] - truth[pen]).abs().mean()), 4) for name, sh in shares.items()}
        err["penumbra_pixels"], err["hit_pixels"] = int(pen.sum()), int(hit.sum())
        out["error"]["radius_%s" % rname] = err
        print(json.dumps({"radius": rname, "error": err}), flush=True)

    # ---- (c) the frames
    def frames(kw, radius):
        def run():
            for _ in range(a.steps):
                r.display(setup, shadows=True, area_radius=radius, **kw)
        return timed(run) / a.steps

    kinds = {"area_32": dict(area=32), "area_8": dict(area=8), "area_8_sets_16_filter_2": dict(area=8, area_sets=16, area_filter=2),
             "area_4_sets_16_filter_3": dict(area=4, area_sets=16, area_filter=3)}
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
