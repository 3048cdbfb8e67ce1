#!/usr/bin/env python3
"""What smooth shading costs on the bench workload.

    python tools/smooth.py [-o profiles/smooth.json] [--workload hall]

The setting and the method of tools/glossy.py: crash 1 M triangles at 1920x1080, uniform grid 128x128x64, the one-stream
renderer with waiting builds, UGRT_FLAG_STATIC_GEOMETRY, one process.  --workload hall: the bench's other scene.  The
vertices are welded with scenes.weld(verts, 1e-5); smooth_cos 0.5.
  (a) the three calls on the scene and on the primary hits of one finished frame, each between two events on the stream,
      median, min and max over `launches` launches after `warm` warm-ups: ugrt_smooth_adjacency, ugrt_smooth_corner_normals
      at crease_cos 0.5 and -1, ugrt_smooth_normals;
  (b) the bytes calls 2 and 3 cannot avoid and the rate that makes of the median.  Corner normals: the face list (12 F),
      every vertex once (12 V), the sorted corners (12 F), the starts (4 V) and the result (36 F).  Shading normals: per
      pixel t, direction, id, the flat normal and the result (44 N), and per DISTINCT triangle hit its indices, vertices and
      corner normals (84 each).  What the kernels move beyond that (the per-face records, the keys, a triangle gathered
      once per pixel that hits it) is their own;
  (c) the frame with and without smooth -- without it the frame is, call for call, the frame as it was before the option
      existed --, static and, where the scene has an animated sub-range, animated (rotate_bunny before every frame, as
      bench.py --animate does: the corner normals are formed again every frame): `steps` frames back to back between two
      events, the forms in turn, `repeats` rounds after a warm-up round.
No time is a pass criterion.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def spread_of(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="triangle-count scale of the scene (1.0 = the bench's)")
    ap.add_argument("--workload", choices=("crash", "hall"), default="crash")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import importlib

    import numpy as np
    import torch

    import bench

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    s = bench.load_scene(ugrt, a.workload, a.scale, 0)
    W, H, lg, ud = a.width, a.height, (128, 128), (128, 128, 64)
    N = W * H
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    verts = np.asarray(s["verts"], np.float32).reshape(-1, 3)
    F, V = len(s["faces"]), len(verts)
    key = ugrt.scenes.weld(verts, 1e-5)
    valence = np.bincount(key[np.asarray(s["faces"]).reshape(-1)], minlength=V)
    out = {"workload": "%s %d triangles, %d vertices, %dx%d, uniform grid 128x128x64, one-stream renderer, waiting builds"
                       % (a.workload, F, V, W, H),
           "weld_tol": 1e-5, "keys": int(len(np.unique(key))), "smooth_cos": 0.5, "launches": a.launches, "warm": a.warm,
           "steps": a.steps, "repeats": a.repeats,
           "corners_per_key": {"mean": round(float(valence[valence > 0].mean()), 2), "max": int(valence.max()),
                               "list_entries_walked": int((valence.astype(np.int64) ** 2).sum())}}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], vertex_key=key)
    setup = ugrt.FrameSetup.from_scene(s)
    r.display(setup, shadows=True, smooth=True)   # builds the adjacency, allocates the buffers
    r.display(setup, shadows=True, shade=False)   # the ids are triangle ids again
    ctx.synchronize()
    stream = torch.cuda.current_stream()
    ids = r.intersect_id.cpu().numpy()
    hit = (ids >= 0) & (r.t.cpu().numpy() > 0)
    out["hit_pixels"], out["distinct_triangles_hit"] = int(hit.sum()), int(len(np.unique(ids[hit])))
    d_key = r._smooth["key"]

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    calls = {
        "adjacency": lambda: ctx.smooth_adjacency(r.d_faces, F, V, d_key),
        "corner_normals_cos_0.5": lambda: ctx.smooth_corner_normals(r.d_faces, r.d_verts, F, 0.5, r.corner_normals),
        "corner_normals_cos_-1": lambda: ctx.smooth_corner_normals(r.d_faces, r.d_verts, F, -1.0, r.corner_normals),
        "normals": lambda: ctx.smooth_normals(r.t, r.dir, r.intersect_id, r.cam_pos, r.d_verts, r.d_faces, r.corner_normals,
                                              r.normal, 1, r.snormal)}
    t = {name: [] for name in calls}
    for k in range(a.warm + a.launches):
        for name, call in calls.items():
            ms = timed(call)
            if k >= a.warm:
                t[name].append(ms)
    calls["corner_normals_cos_0.5"]()  # (what the frames below expect to find)
    out["call_ms"] = {name: spread_of(ms) for name, ms in t.items()}
    bytes_2 = 60 * F + 16 * V
    bytes_3 = 44 * N + 84 * out["distinct_triangles_hit"]
    out["compulsory_bytes"] = {"corner_normals": bytes_2, "normals": bytes_3}
    out["achieved_GB_per_s"] = {
        "corner_normals_cos_0.5": round(bytes_2 / out["call_ms"]["corner_normals_cos_0.5"]["median"] / 1e6, 1),
        "corner_normals_cos_-1": round(bytes_2 / out["call_ms"]["corner_normals_cos_-1"]["median"] / 1e6, 1),
        "normals": round(bytes_3 / out["call_ms"]["normals"]["median"] / 1e6, 1)}
    print(json.dumps({k: out[k] for k in ("call_ms", "compulsory_bytes", "achieved_GB_per_s")}), flush=True)

    # (c) the frame
    animated = "animated_size" in s  # (the hall has no animated sub-range: its static forms only)
    if animated:
        r.init_orig_list(s["animated_size"], s["animated_offset"])
    frame_no = [0]

    def frames(kw, animate):
        def run():
            for _ in range(a.steps):
                if animate:
                    frame_no[0] += 1
                    r.rotate_bunny(1.81 + 0.05 * frame_no[0])
                r.display(setup, shadows=True, **kw)
        return timed(run) / a.steps

    kinds = {"static": (dict(), False), "static_smooth": (dict(smooth=True), False)}
    if animated:
        kinds.update({"animated": (dict(), True), "animated_smooth": (dict(smooth=True), True)})
    ms = {k: [] for k in kinds}
    for rnd in range(a.repeats + 1):  # round 0 warms every form up
        for k, (kw, animate) in kinds.items():
            t_ = frames(kw, animate)
            if rnd:
                ms[k].append(t_)
    out["frame_ms"] = {k: spread_of(v_) for k, v_ in ms.items()}
    out["builds"] = {"adjacency": ctx.get_state("smooth_adjacency_builds"), "corner_normals": ctx.get_state("smooth_normal_builds")}
    print(json.dumps({"frame_ms": out["frame_ms"]}), flush=True)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
