#!/usr/bin/env python3
"""What several lights cost on the bench workload.

    python tools/lights.py [-o profiles/lights.json]

The bench setting (bench.py's scene loader and its one-GPU resolution), primary + shadows, no reflections, on the
one-stream renderer with waiting builds -- the only frame the lights run in.
  (a) The frame with FrameSetup.lights of 1, 2, 3 and 4 lights against the frame without `lights`: `steps` frames
      back to back between two events, the five forms in turn, `repeats` rounds after a warm-up round; median, min and
      max of the rounds' ms per frame.
  (b) ugrt_shade_lights at L = 1..4 against L x (ugrt_shade_simple + ugrt_shade_add_shadows) on the arrays of one
      finished four-light frame: stage "shade" of the built-in profiler, the two sides in turn, `launches` launches
      after `warm` warm-ups.  The composed side has no kernel that averages its L images: that pass is not counted.
The lights are the scene's own and its eye moved by a third of the scene's extent along +x, +y, -x.
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


def lights_for(s, count):
    import numpy as np

    v = np.asarray(s["verts"], np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    ext, centre = hi - lo, (lo + hi) / 2
    base = s["light_camera"]
    eye0, sl0 = np.asarray(base["eye"], np.float64), np.asarray(s["shading_light"], np.float64)
    out = [(base, tuple(float(x) for x in sl0))]
    for off in ((ext[0] / 3, 0, 0), (0, ext[1] / 3, 0), (-ext[0] / 3, 0, 0)):
        off = np.asarray(off)
        cam = dict(eye=tuple(float(x) for x in eye0 + off), look=tuple(float(x) for x in centre), up=(0.0, 1.0, 0.0),
                   near=base["near"], far=base["far"])
        out.append((cam, tuple(float(x) for x in sl0 + off)))
    return out[:count]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="triangle-count scale of the scene (1.0 = the bench's)")
    a = ap.parse_args()
    import importlib

    import torch

    import bench

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    s = bench.load_scene(ugrt, "crash", a.scale, 0)
    W, H = importlib.import_module(ugrt.__name__ + ".parallel").weak_scaling_resolution(1)
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    LMAX = 4
    lights = lights_for(s, LMAX)
    out = {"workload": "crash %d triangles, %dx%d, primary + shadows, one-stream renderer, waiting builds"
                       % (len(s["faces"]), W, H),
           "launches": a.launches, "warm": a.warm, "steps": a.steps, "repeats": a.repeats}
    ctx = ugrt.Context(W, H, flags=flags)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    setups = {0: ugrt.FrameSetup.from_scene(s)}
    for L in range(1, LMAX + 1):
        setups[L] = ugrt.FrameSetup.from_scene(s, lights=lights[:L])
    stream = torch.cuda.current_stream()

    # ---- (a) the frame
    def frames(L):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            r.display(setups[L], frame_cnt=1, shadows=True)
        e1.record(stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    ms = {L: [] for L in setups}
    for rnd in range(a.repeats + 1):  # round 0 warms every form up
        for L in setups:
            v = frames(L)
            if rnd:
                ms[L].append(v)
    single = statistics.median(ms[0])
    out["frame_ms"] = {"without_lights": spread(ms[0])}
    for L in range(1, LMAX + 1):
        out["frame_ms"]["lights_%d" % L] = dict(spread(ms[L]), over_the_single_light_frame=round(statistics.median(ms[L]) / single, 3))
    print(json.dumps({"frame_ms": out["frame_ms"]}), flush=True)

    # ---- (b) the shading, on the arrays of one finished four-light frame
    r.display(setups[LMAX], shadows=True, shade=False)
    ctx.synchronize()
    ids0 = r.intersect_id.clone()
    ctx.prof_enable(True, stages=["shade"])

    def fused(L):
        ctx.shade_lights(r.image, r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.d_matlist,
                         r.num_materials, [p for _, p in lights[:L]], r.shadowed_lights)

    def composed(L):
        for l in range(L):
            if l:
                r.intersect_id.copy_(ids0)  # (a device copy outside the timed stage)
            ctx.set_light_position(lights[l][1])
            ctx.shade_simple(r.image, r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.d_matlist,
                             r.num_materials)
            ctx.shade_add_shadows(r.image, r.shadowed_lights[l])

    def once(call, L):
        r.intersect_id.copy_(ids0)
        ctx.prof_reset()
        call(L)
        ctx.synchronize()
        return ctx.prof_get()["shade"]

    out["shade_ms"] = {}
    for L in range(1, LMAX + 1):
        t = {"shade_lights": [], "simple_plus_add_shadows_x_L": []}
        launches = {}
        for k in range(a.warm + a.launches):
            for name, call in (("shade_lights", fused), ("simple_plus_add_shadows_x_L", composed)):
                v, n = once(call, L)
                launches[name] = n
                if k >= a.warm:
                    t[name].append(v)
        row = {name: dict(spread(v), launches=launches[name]) for name, v in t.items()}
        row["fused_over_composed"] = round(row["shade_lights"]["median"] / row["simple_plus_add_shadows_x_L"]["median"], 3)
        out["shade_ms"]["lights_%d" % L] = row
        print(json.dumps({"lights": L, **row}), flush=True)
    # L = 1 is byte for byte the composed image (the tests pin this; the figure is only worth something if it holds here)
    once(fused, 1)
    img = r.image.clone()
    once(composed, 1)
    out["one_light_equals_simple_plus_add_shadows"] = bool(torch.equal(img, r.image))
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
