#!/usr/bin/env python3
"""What temporal accumulation gains and costs on the bench workload.

    python tools/temporal.py [-o profiles/temporal.json] [--workload hall]

The setting and the method of tools/ambient_sets.py: crash 1 M triangles at 1920x1080, uniform grid 128x128x64, the
one-stream renderer with waiting builds, one process; the ambient radius is 5 % and the light's disk 10 % of the scene's
largest extent.  --workload hall: the bench's other scene.  Per effect -- ao=4, area=8, gi=8, each with *_sets=16,
*_filter=2 and temporal=16 -- a sequence of 16 frames under a standing camera and one under a slow orbit (a quarter of
a degree per frame about the up axis through the point looked at).  After 1, 2, 4, 8 and 16 frames the running mean (the
history the temporal call wrote) is compared with 512 samples taken here on the GPU from that frame's own primary hits
(16 launches of 32 along the 16 turned sets): the mean absolute error of the open share (ao), the lit share (area) or
the three colour shares (gi) over the hit pixels whose 512-sample value lies strictly between 0 and 1.  Beside them the
single frames ao=32 and area=32 (and gi=32), the share of hit pixels whose history was dropped per orbit frame, the frame
times (`steps` frames back to back between two events, the forms in turn, `repeats` rounds after a warm-up round) and the
two temporal kernels' own times (median, min, max over `launches` launches after `warm` warm-ups).
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

AT = (1, 2, 4, 8, 16)


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def orbit(camera, degrees):
    """The camera turned by `degrees` about its up axis through the point it looks at."""
    import numpy as np

    eye, look, up = (np.asarray(camera[k], np.float64) for k in ("eye", "look", "up"))
    u = up / np.sqrt((up * up).sum())
    d, a = eye - look, math.radians(degrees)
    turned = d * math.cos(a) + np.cross(u, d) * math.sin(a) + u * (u @ d) * (1.0 - math.cos(a))
    return dict(camera, eye=tuple(float(x) for x in look + turned))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="triangle-count scale of the scene (1.0 = the bench's)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--step-degrees", type=float, default=0.25)
    ap.add_argument("--workload", choices=("crash", "hall"), default="crash")
    a = ap.parse_args()
    import importlib

    import numpy as np
    import torch

    import bench

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    rmod = importlib.import_module("uniformgrid-raytracing_amd.renderer")
    s = bench.load_scene(ugrt, a.workload, a.scale, 0)
    W, H, lg, ud = a.width, a.height, (128, 128), (128, 128, 64)
    N = W * H
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    v = np.asarray(s["verts"], np.float32).reshape(-1, 3)
    extent = float((v.max(0) - v.min(0)).max())
    ao_radius, area_radius = float(np.float32(0.05 * extent)), float(np.float32(0.10 * extent))
    plane = rmod.default_filter_plane(v.min(0), v.max(0))
    out = {"workload": "%s %d triangles, %dx%d, uniform grid 128x128x64, one-stream renderer, waiting builds"
                       % (a.workload, len(s["faces"]), W, H),
           "ao_radius": ao_radius, "area_radius": area_radius, "filter_cos": 0.9, "filter_plane": plane, "temporal": 16,
           "orbit_degrees_per_frame": a.step_degrees, "launches": a.launches, "warm": a.warm, "steps": a.steps,
           "repeats": a.repeats}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    setup0 = ugrt.FrameSetup.from_scene(s)
    stream = torch.cuda.current_stream()
    lcam = rmod.make_camera(setup0.light_camera, setup0.fovy, r.aspect)
    light_eye = np.asarray(setup0.light_camera["eye"], np.float64)
    light_axis = np.asarray(setup0.light_camera["look"], np.float64) - light_eye

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def opens(mask, S):
        m = mask.to(torch.int64) & ((1 << S) - 1)
        dark = torch.zeros_like(m)
        for b in range(S):
            dark += (m >> b) & 1
        return (S - dark).to(torch.float64)

    m32 = torch.empty(N, dtype=torch.int32, device=ctx.device)
    sum32 = torch.zeros(4 * N, dtype=torch.int32, device=ctx.device)
    turned = ugrt.scenes.ao_direction_sets(32, 16)
    d_turned = [ctx.upload(turned[k].reshape(-1)) for k in range(16)]
    disk = ugrt.scenes.area_sample_sets(32, 16, light_eye, light_axis, area_radius)

    def truth(kind):
        """[N, C] float64: 512 samples from the primary hits r.ao_rays / r.ao_active of the frame just rendered."""
        uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
        acc = torch.zeros((N, 3 if kind == "gi" else 1), dtype=torch.float64, device=ctx.device)
        for k in range(16):
            if kind == "ao":
                ctx.trace_dda_any_hemi(uvalue, uspan, uoffset, r.d_verts, r.d_faces, r.ao_rays, r.ao_active, turned[k], ao_radius, m32)
            elif kind == "area":
                ctx.trace_dda_any_area(uvalue, uspan, uoffset, r.d_verts, r.d_faces, r.ao_rays, r.ao_active, disk[k], m32)
            else:
                ctx.gi_gather(uvalue, uspan, uoffset, r.d_verts, r.d_faces, r.ao_rays, r.ao_active, 32, 1, 1, d_turned[k],
                              float("inf"), r.d_matidx, r.d_matlist, r.num_materials, lcam.worldori[:3], r.reflect_eps, sum32)
            ctx.synchronize()
            if kind == "gi":
                acc += sum32.view(N, 4)[:, :3].to(torch.float64) / (255.0 * 32.0)
            else:
                acc[:, 0] += opens(m32, 32) / 32.0
        return acc / 16.0

    def share_of(kind):
        """The running mean the last temporal frame left, [N, C] float64."""
        h = r.temporal_history(kind).to(torch.float64)
        return h.view(N, 4)[:, :3] if kind == "gi" else h.view(N, 2)[:, :1]

    def single_share(kind, S):
        """The share of one frame without a gather, from the frame's own mask or sums."""
        if kind == "gi":
            return r.gi_sum.view(N, 4)[:, :3].to(torch.float64) / (255.0 * S)
        return (opens(r.ao_mask if kind == "ao" else r.area_mask, S) / S).view(N, 1)

    def error(share, want, hit):
        partly = hit[:, None] & (want > 0) & (want < 1)
        return round(float((share[partly] - want[partly]).abs().mean()), 5), int(partly.sum())

    effects = {"ao": dict(ao=4, ao_sets=16, ao_filter=2, ao_radius=ao_radius),
               "area": dict(area=8, area_sets=16, area_filter=2, area_radius=area_radius),
               "gi": dict(gi=8, gi_sets=16, gi_filter=2)}
    big = {"ao": dict(ao=32, ao_radius=ao_radius), "area": dict(area=32, area_radius=area_radius), "gi": dict(gi=32)}
    out["error"], out["dropped_share_per_orbit_frame"] = {}, {}
    for kind, kw in effects.items():
        e = {}
        # the single frame at 32 samples, and the effect's own single frame (sets and gather, no accumulation)
        r.display(setup0, **big[kind])
        ctx.synchronize()
        hit = r.ao_active != 0
        want = truth(kind)
        e["single_frame_32"], e["partly_pixels"] = error(single_share(kind, 32), want, hit)
        e["hit_pixels"] = int(hit.sum())
        for path in ("standing", "orbit"):
            r.temporal_reset()
            errs, dropped = {}, []
            for f in range(1, 17):
                cam = setup0.camera if path == "standing" else orbit(setup0.camera, a.step_degrees * (f - 1))
                r.display(ugrt.FrameSetup(cam, setup0.light_camera, setup0.shading_light), temporal=16, **kw)
                ctx.synchronize()
                hit = r.ao_active != 0
                if path == "orbit" and f > 1:
                    n = r.temporal_history(kind).view(N, -1)[:, -1]
                    dropped.append(round(float((n[hit] == 1).to(torch.float64).mean()), 5))
                if f in AT:
                    if path == "orbit" or f == 1:
                        want = truth(kind)
                    errs["after_%d" % f] = error(share_of(kind), want, hit)[0]
            e[path] = errs
            if path == "orbit":
                out["dropped_share_per_orbit_frame"][kind] = dropped
        out["error"][kind] = e
        print(json.dumps({"effect": kind, "error": e}), flush=True)

    # ---- the frame times
    def frames(kw):
        def run():
            for _ in range(a.steps):
                r.display(setup0, **kw)
        return timed(run) / a.steps

    kinds = {"plain": dict()}
    for kind, kw in effects.items():
        kinds[kind + "_32"] = big[kind]
        kinds[kind + "_sets_16_filter_2"] = kw
        kinds[kind + "_sets_16_filter_2_temporal_16"] = dict(kw, temporal=16)
    ms = {k: [] for k in kinds}
    for rnd in range(a.repeats + 1):  # round 0 warms every form up
        for k, kw in kinds.items():
            t = frames(kw)
            if rnd:
                ms[k].append(t)
    out["frame_ms"] = {k: spread(v) for k, v in ms.items()}
    print(json.dumps({"frame_ms": out["frame_ms"]}), flush=True)

    # ---- the two kernels, on the last temporal frames' buffers
    r.temporal_reset()
    for _ in range(2):
        r.display(setup0, temporal=16, **dict(effects["ao"], **effects["gi"]))
    ctx.synchronize()
    cc = rmod.make_camera(setup0.camera, setup0.fovy, r.aspect).camcoords
    sa, sg = r._temporal["ao"], r._temporal["gi"]
    calls = {"temporal_visibility": lambda: ctx.temporal_visibility(r.ao_vis, 4, r.ao_rays, r.ao_active, cc, r.prev_ao_rays,
                                                                    r.prev_ao_active, sa["hist"][sa["turn"]], 16, 0.9, plane,
                                                                    sa["hist"][1 - sa["turn"]], r.ao_tvis),
             "temporal_gi": lambda: ctx.temporal_gi(r.gi_acc, 8, r.ao_rays, r.ao_active, cc, r.prev_ao_rays, r.prev_ao_active,
                                                    sg["hist"][sg["turn"]], 16, 0.9, plane, sg["hist"][1 - sg["turn"]], r.gi_tacc),
             "filter_visibility_radius_2": lambda: ctx.filter_visibility(r.ao_mask, 4, r.ao_rays, r.ao_active, 2, 0.9, plane, r.ao_vis)}
    t = {name: [] for name in calls}
    for k in range(a.warm + a.launches):
        for name, call in calls.items():
            one = timed(call)
            if k >= a.warm:
                t[name].append(one)
    out["kernel_ms"] = {name: spread(v) for name, v in t.items()}
    r.temporal_reset()
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
