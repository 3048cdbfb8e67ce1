#!/usr/bin/env python3
"""What texture mapping costs on the bench workload.

    python tools/texture.py [-o profiles/texture.json] [--workload hall] [--parent DIR]

The setting and the method of tools/smooth.py: crash 1 M triangles at 1920x1080, uniform grid 128x128x64, the one-stream
renderer with waiting builds, UGRT_FLAG_STATIC_GEOMETRY, one process.  --workload hall: the bench's other scene.  Every
material is textured with a 1024 x 1024 checker of 64 x 64 cells through scenes.planar_uvs(verts, faces, 1.0).
  (a) ugrt_texture_set, and ugrt_texture_albedo at texture_aniso 1, 4, 8 and 16 on the primary hits of one finished frame,
      each between two events on the stream: median, min and max over `launches` launches after `warm` warm-ups;
  (b) the shading call with and without the albedo;
  (c) the bytes ugrt_texture_albedo cannot avoid -- per pixel t, direction, id and the result (32 N), per DISTINCT triangle
      hit its indices, vertices, uv indices and uvs (84 each) -- and the rate that makes of the median.  The texels are not
      counted: which of them a frame needs depends on the levels, and 8 taps of 8 texels re-read their neighbours' lines;
  (d) the frame with and without textures=True -- without it the frame is, call for call, the frame as it was before the
      option existed --: `steps` frames back to back between two events, the forms in turn, `repeats` rounds after a warm-up
      round;
  (e) with --parent DIR, a checkout of the parent commit with its library built: the plain frame of that tree and of this
      one, each in a fresh child process of this script (--plain-only --root), in turn, `repeats` times, timed as in (d).
      The plain frame of this tree must not be slower than the parent's by more than the spread of the parent's own
      repeats; the tool reports both lists and that spread.
No time is a pass criterion.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:  # (a child of (e): the tree whose package and bench.py are imported)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread_of(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=None)
    ap.add_argument("--launches", type=int, default=9)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="triangle-count scale of the scene (1.0 = the bench's)")
    ap.add_argument("--workload", choices=("crash", "hall"), default="crash")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: (e)")
    ap.add_argument("--root", default=None, help="(child of --parent) the tree to import")
    ap.add_argument("--plain-only", action="store_true", help="(child of --parent) time the plain frame and print it")
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
    F = len(s["faces"])
    M = len(s["reflect"])
    out = {"workload": "%s %d triangles, %dx%d, uniform grid 128x128x64, one-stream renderer, waiting builds" % (a.workload, F, W, H),
           "texture": "1024 x 1024 checker of 64 x 64 cells on every material, planar_uvs at 1 repeat per unit", "launches": a.launches,
           "warm": a.warm, "steps": a.steps, "repeats": a.repeats}
    ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
    if a.plain_only:  # nothing here names a texture: the parent's package runs it as well
        r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
        setup = ugrt.FrameSetup.from_scene(s)
        stream = torch.cuda.current_stream()
        ms = []
        for rnd in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.steps):
                r.display(setup, shadows=True)
            e1.record(stream)
            ctx.synchronize()
            torch.cuda.synchronize()
            if rnd:
                ms.append(e0.elapsed_time(e1) / a.steps)
        print(json.dumps({"plain_frame_ms": ms}), flush=True)
        return
    uvs, uv_faces = ugrt.scenes.planar_uvs(s["verts"], s["faces"], 1.0)
    tex = ugrt.scenes.checker_texture(1024, 64)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], uvs=uvs, uv_faces=uv_faces,
                      textures=[tex], mat_texture=np.zeros(M, np.int32))
    setup = ugrt.FrameSetup.from_scene(s)
    r.display(setup, shadows=True, textures=True)  # builds the atlas, allocates the buffers
    r.display(setup, shadows=True, shade=False)    # the ids are triangle ids again
    cam = ugrt.renderer.make_camera(setup.camera, setup.fovy, r.aspect)
    ctx.upload_camera(cam.camcoords)               # the eye's camera, as behind the camera pass
    ctx.synchronize()
    stream = torch.cuda.current_stream()
    ids = r.intersect_id.cpu().numpy()
    hit = (ids >= 0) & (r.t.cpu().numpy() > 0)
    out["hit_pixels"], out["distinct_triangles_hit"] = int(hit.sum()), int(len(np.unique(ids[hit])))
    st = r._tex

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def albedo(aniso):
        return lambda: ctx.texture_albedo(r.t, r.dir, r.intersect_id, r.cam_pos, r.d_verts, r.d_faces, st["uvs"], st["num_uvs"],
                                          st["uv_faces"], r.d_matidx, r.d_matlist, r.num_materials, st["mat_texture"],
                                          st["mat_texture_host"], aniso, 0, r.albedo)

    ids_copy = r.intersect_id.clone()

    def shade(with_albedo):
        def call():
            r.intersect_id.copy_(ids_copy)  # (the shading call rewrites the ids; the copy is inside both timings alike)
            if with_albedo:
                ctx.texture_shade(r.image, r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.d_matlist, r.num_materials,
                                 r.albedo)
            else:
                ctx.shade_simple(r.image, r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.d_matlist, r.num_materials)
        return call

    calls = {"texture_set": lambda: ctx.texture_set([tex])}
    calls.update({"albedo_aniso_%d" % k: albedo(k) for k in (1, 4, 8, 16)})
    calls.update({"ids_copy+shade_simple": shade(False), "ids_copy+texture_shade": shade(True)})
    t = {name: [] for name in calls}
    for k in range(a.warm + a.launches):
        for name, call in calls.items():
            ms = timed(call)
            if k >= a.warm:
                t[name].append(ms)
    r.intersect_id.copy_(ids_copy)
    out["call_ms"] = {name: spread_of(ms) for name, ms in t.items()}
    nbytes = 32 * N + 84 * out["distinct_triangles_hit"]
    out["compulsory_bytes"] = {"albedo": nbytes}
    out["achieved_GB_per_s"] = {name: round(nbytes / out["call_ms"][name]["median"] / 1e6, 1) for name in calls if name.startswith("albedo")}
    print(json.dumps({k: out[k] for k in ("call_ms", "compulsory_bytes", "achieved_GB_per_s")}), flush=True)

    # (d) the frame
    def frames(kw):
        def run():
            for _ in range(a.steps):
                r.display(setup, shadows=True, **kw)
        return timed(run) / a.steps

    kinds = {"plain": dict(), "textures_aniso_1": dict(textures=True, texture_aniso=1), "textures_aniso_8": dict(textures=True),
             "textures_aniso_16": dict(textures=True, texture_aniso=16)}
    ms = {k: [] for k in kinds}
    for rnd in range(a.repeats + 1):  # round 0 warms every form up
        for k, kw in kinds.items():
            t_ = frames(kw)
            if rnd:
                ms[k].append(t_)
    out["frame_ms"] = {k: spread_of(v_) for k, v_ in ms.items()}
    out["builds"] = {"texture": ctx.get_state("texture_builds")}
    print(json.dumps({"frame_ms": out["frame_ms"]}), flush=True)
    if a.parent:
        def child(root):
            cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--root", root, "--workload", a.workload, "--scale",
                   str(a.scale), "--steps", str(a.steps), "--repeats", str(a.repeats), "--width", str(W), "--height", str(H)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise RuntimeError("the plain frame of %s failed: %s" % (root, p.stderr[-2000:]))
            return json.loads(p.stdout.strip().split("\n")[-1])["plain_frame_ms"]
        both = {"parent": [], "this": []}
        for _ in range(3):
            both["parent"] += child(os.path.abspath(a.parent))
            both["this"] += child(ROOT)
        out["plain_frame_vs_parent_ms"] = {k: dict(spread_of(v), runs=[round(x, 4) for x in v]) for k, v in both.items()}
        out["plain_frame_vs_parent_ms"]["parent_spread"] = round(max(both["parent"]) - min(both["parent"]), 4)
        out["plain_frame_vs_parent_ms"]["median_difference"] = round(statistics.median(both["this"]) - statistics.median(both["parent"]), 4)
        print(json.dumps({"plain_frame_vs_parent_ms": out["plain_frame_vs_parent_ms"]}), flush=True)
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
