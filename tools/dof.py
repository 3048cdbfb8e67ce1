#!/usr/bin/env python3
"""What the depth of field costs on the bench workload and what the lens's divergence costs on top of the same number of
pinhole rays.

    python tools/dof.py [-o profiles/dof.json] [--workload hall]

The setting and the method of tools/antialias.py: crash 1 M triangles (--workload bench) or the hall at 1920x1080, uniform
grid 128x128x64, the one-stream renderer with waiting builds, one process.  The lens is focused on the camera's look-at
point; two apertures, `small` and `wide`, in world units.  On the primary hits of one finished frame, each call between two
events on the stream; median, min and max over `launches` launches after `warm` warm-ups:
  (a) ugrt_dof_pixels at the default criterion (dof_min 0.5, dof_window 4) and the share of the pixels it flags, per
      aperture;
  (b) ugrt_dof_gather at S = 4, 8 and 16 with sixteen sets, with and without the shadow phase, per aperture, and the same
      call on the same flags with a lens of radius 0 -- ugrt_aa_gather's rays: the difference is what the lens's
      divergence costs the walks;
  (c) the composition on the same rays {o_s, d_s} (formed here on the host in fp32 and uploaded per sample, which is not
      timed): S times ugrt_trace_dda and, with the shadow phase, S times ugrt_occlusion_rays + ugrt_trace_dda_any, with
      the flags as the active flags.  It leaves out the depth gate, the shading and the sum.  Asserted at S = 4, wide
      aperture, one set: the S one-sample gathers of the table's entries add up to the S-sample gather's sums word for word
      (equal sums), and a sample that has bytes is a sample the composition's ugrt_trace_dda hit -- but for at most one in
      100 000, since the host's rays may differ from the kernel's in an ulp; the count is reported;
  (d) the frame with dof = S against the frame without: `steps` frames back to back between two events, the forms in turn,
      `repeats` rounds after a warm-up round;
  (e) at 256x144, the mean absolute byte difference over all pixels against a 512-sample image -- every pixel flagged, the
      sixteen sets of scenes.lens_sample_sets(32, 16) one after the other, the sums added: of the plain frame and of each
      dof frame, per aperture.
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
    ap.add_argument("--workload", choices=("bench", "hall"), default="bench")
    ap.add_argument("--small", type=float, default=0.05, help="the small aperture, world units")
    ap.add_argument("--wide", type=float, default=0.15, help="the wide aperture, world units")
    a = ap.parse_args()
    import ctypes as C
    import importlib

    import numpy as np
    import torch

    import bench

    ugrt = importlib.import_module("uniformgrid-raytracing_amd")
    rmod = importlib.import_module("uniformgrid-raytracing_amd.renderer")
    s = bench.load_scene(ugrt, "crash" if a.workload == "bench" else "hall", a.scale, 0)
    lg, ud = (128, 128), (128, 128, 64)
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY
    setup = ugrt.FrameSetup.from_scene(s)
    apertures = {"small": a.small, "wide": a.wide}
    f32, i32 = torch.float32, torch.int32
    stream = torch.cuda.current_stream()

    def timed(call, c):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        c.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def make(W, H):
        ctx = ugrt.Context(W, H, light_grid=lg, flags=flags, uniform_dims=ud)
        return ctx, ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])

    out = {"workload": "%s %d triangles, 1920x1080, uniform grid 128x128x64, one-stream renderer, waiting builds"
                       % (a.workload, len(s["faces"])),
           "apertures": apertures, "dof_min": 0.5, "dof_window": 4, "launches": a.launches, "warm": a.warm, "steps": a.steps,
           "repeats": a.repeats}

    # (e) first, on a small frame: the 512-sample image and the frames' distance from it
    w, h = 256, 144
    n = w * h
    sctx, sr = make(w, h)
    out["error_vs_512_samples_256x144"] = {}
    for tag, ap_ in apertures.items():
        sr.display(setup, shadows=True)
        sctx.synchronize()
        plain = sr.image.cpu().numpy().astype(np.int32)
        sr.display(setup, shadows=True, dof=4, dof_aperture=ap_)  # builds the uniform grid, allocates the buffers
        sr.display(setup, shadows=True, shade=False)  # triangle ids again; the context holds the light camera's block
        sctx.synchronize()
        cam = rmod.make_camera(setup.camera, setup.fovy, sr.aspect)
        lens, _ = cam.lens(ap_, None, h)
        light = tuple(float(x) for x in rmod.make_camera(setup.light_camera, setup.fovy, sr.aspect).worldori[:3])
        uvalue, uspan, uoffset, _ = sctx.grid_ptrs(ugrt.GRID_UNIFORM)
        ones = torch.ones(n, dtype=i32, device=sctx.device)
        sums = torch.zeros(4 * n, dtype=i32, device=sctx.device)
        total = torch.zeros(4 * n, dtype=torch.int64, device=sctx.device)
        for one in ugrt.scenes.lens_sample_sets(32, 16):
            sctx.dof_gather(uvalue, uspan, uoffset, sr.d_verts, sr.d_faces, cam.camcoords, lens, ones, 32, 1, 1,
                            sctx.upload(one.reshape(-1)), sr.d_matidx, sr.d_matlist, sr.num_materials, light, sr.reflect_eps, sums)
            sctx.synchronize()
            total += sums
        ref = (total.cpu().numpy().reshape(n, 4)[:, :3] + 256) // 512
        err = lambda img: round(float(np.abs(img.reshape(n, 3) - ref).mean()), 4)
        e = {"plain": err(plain)}
        for S in (4, 8, 16):
            for sets in (1, 16):
                sr.display(setup, shadows=True, dof=S, dof_aperture=ap_, dof_sets=sets)
                sctx.synchronize()
                e["dof_%d_sets_%d" % (S, sets)] = err(sr.image.cpu().numpy().astype(np.int32))
        e["flagged_share"] = round(float((sr.dof_flag != 0).sum().item()) / n, 4)
        out["error_vs_512_samples_256x144"][tag] = e
    print(json.dumps({"error": out["error_vs_512_samples_256x144"]}), flush=True)
    del sctx, sr

    # (a), (b), (c): the calls at 1920x1080, on the arrays of a frame that has not been shaded
    W, H = 1920, 1080
    N = W * H
    ctx, r = make(W, H)
    r.display(setup, shadows=True, dof=4, dof_aperture=a.wide)
    r.display(setup, shadows=True, shade=False)
    ctx.synchronize()
    cam = rmod.make_camera(setup.camera, setup.fovy, r.aspect)
    eye_cc = np.asarray(cam.camcoords, np.float32).copy()
    light = tuple(float(x) for x in rmod.make_camera(setup.light_camera, setup.fovy, r.aspect).worldori[:3])
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    sums = torch.zeros(4 * N, dtype=i32, device=ctx.device)
    tex = np.zeros(100, np.float32)
    ugrt.check(ugrt.lib.ugrt_camera_direction_table(ugrt._f3(eye_cc), tex.ctypes.data_as(C.POINTER(C.c_float))))
    cols, rows = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))

    def explicit(ent, lens):
        """[6N] rays {o, d} of one table entry (the contract's arithmetic in numpy fp32; not the strict rule)."""
        ftx = np.float32(1) - (cols + np.float32(ent[0])) / np.float32(W)
        fty = (rows + np.float32(ent[1])) / np.float32(H)
        xs, ys = ftx * np.float32(4), fty * np.float32(4)
        i, j = np.minimum(xs.astype(np.int32), 3), np.minimum(ys.astype(np.int32), 3)
        fa, fb = xs - i.astype(np.float32), ys - j.astype(np.float32)
        t4 = tex.reshape(5, 5, 4)
        d = (((1 - fa) * (1 - fb))[..., None] * t4[j, i, :3] + (fa * (1 - fb))[..., None] * t4[j, i + 1, :3]
             + ((1 - fa) * fb)[..., None] * t4[j + 1, i, :3] + (fa * fb)[..., None] * t4[j + 1, i + 1, :3]) - eye_cc[:3]
        d = (d * (np.float32(1) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))[..., None])
        d = d.astype(np.float32)
        c =(d[..., 0] * lens[6] + d[..., 1] * lens[7]) + d[..., 2] * lens[8]
        s_f = np.float32(lens[9]) / c
        L = (np.float32(ent[2]) * lens[0:3] + np.float32(ent[3]) * lens[3:6]).astype(np.float32)
        front = (c > 0)[..., None]
        o = np.where(front, eye_cc[:3] + L, eye_cc[:3]).astype(np.float32)
        d = np.where(front, d - L / s_f[..., None], d).astype(np.float32)
        return ctx.upload(np.concatenate([o, d], -1).astype(np.float32).reshape(-1))

    hit_t, occ_rays = torch.empty(N, dtype=f32, device=ctx.device), torch.empty(6 * N, dtype=f32, device=ctx.device)
    hit_id, occ_act, occ = (torch.empty(N, dtype=i32, device=ctx.device) for _ in range(3))

    def gather(lens, flag, S, tile, table, shadow, into=sums):
        ctx.dof_gather(uvalue, uspan, uoffset, r.d_verts, r.d_faces, eye_cc, lens, flag, S, tile, tile, table, r.d_matidx, r.d_matlist,
                       r.num_materials, light if shadow else None, r.reflect_eps, into)

    def composed(rays, flag, shadow):
        for d_rays in rays:
            ctx.trace_dda(uvalue, uspan, uoffset, r.d_verts, r.d_faces, d_rays, flag, hit_t, hit_id)
            if shadow:
                ctx.occlusion_rays(d_rays, flag, hit_t, hit_id, r.d_verts, r.d_faces, light, r.reflect_eps, occ_rays, occ_act)
                ctx.trace_dda_any(uvalue, uspan, uoffset, r.d_verts, r.d_faces, occ_rays, occ_act, 1.0, occ)

    out["pixels"], out["calls_ms"] = {}, {}
    for tag, ap_ in apertures.items():
        lens, coc_scale = cam.lens(ap_, None, H)
        lens0 = lens.copy()
        lens0[:6] = 0.0
        flag = torch.zeros(N, dtype=i32, device=ctx.device)
        pixels = lambda: ctx.dof_pixels(r.t, r.dir, r.intersect_id, lens[6:9], float(lens[9]), coc_scale, 0.5, 4, flag)
        ms = [timed(pixels, ctx) for _ in range(a.warm + a.launches)][a.warm:]
        out["pixels"][tag] = {"ms": spread(ms), "flagged_share": round(float((flag != 0).sum().item()) / N, 4),
                              "focus": float(lens[9]), "coc_scale": coc_scale}
        print(json.dumps({"aperture": tag, "pixels": out["pixels"][tag]}), flush=True)
        if tag == "wide":  # (c)'s assertion: the sums of the S one-sample gathers are the S-sample gather's
            S = 4
            one = ugrt.scenes.lens_sample_sets(S, 1)
            gather(lens, flag, S, 1, ctx.upload(one.reshape(-1)), True)
            ctx.synchronize()
            whole = sums.clone()
            parts = torch.zeros_like(whole)
            single = torch.zeros_like(whole)
            stray = 0
            for k in range(S):
                gather(lens, flag, 1, 1, ctx.upload(one[0, k].reshape(-1)), True, single)
                d_rays = explicit(one[0, k], lens)
                ctx.trace_dda(uvalue, uspan, uoffset, r.d_verts, r.d_faces, d_rays, flag, hit_t, hit_id)
                ctx.synchronize()
                parts += single
                bytes_ = single.view(N, 4)[:, :3].sum(1) > 0
                stray += int((bytes_ & (hit_id < 0)).sum().item())  # (the host's rays may differ from the kernel's in an ulp)
                del d_rays
            assert stray <= N * S // 100000, "samples with bytes that ugrt_trace_dda did not hit: %d" % stray
            out["samples_with_bytes_the_composition_missed"] = stray
            whole4, parts4 = whole.view(N, 4), parts.view(N, 4)
            assert bool((whole4[:, :3] == parts4[:, :3]).all()) and bool((whole4[:, 3] * S == parts4[:, 3]).all())
            out["sums_of_single_samples_equal"] = True
        for S in (4, 8, 16):
            table = ugrt.scenes.lens_sample_sets(S, 16)
            d_sets = ctx.upload(table.reshape(-1))
            rays = [explicit(e, lens) for e in table[0]]
            calls = {}
            for shadow in (True, False):
                kind = "shadow" if shadow else "plain"
                calls["gather_" + kind] = lambda shadow=shadow: gather(lens, flag, S, 4, d_sets, shadow)
                calls["gather_radius_0_" + kind] = lambda shadow=shadow: gather(lens0, flag, S, 4, d_sets, shadow)
                calls["composed_" + kind] = lambda shadow=shadow: composed(rays, flag, shadow)
            t = {name: [] for name in calls}
            for k in range(a.warm + a.launches):
                for name, call in calls.items():
                    ms_ = timed(call, ctx)
                    if k >= a.warm:
                        t[name].append(ms_)
            e = {name: spread(v) for name, v in t.items()}
            for kind in ("shadow", "plain"):
                g, g0, c = e["gather_" + kind], e["gather_radius_0_" + kind], e["composed_" + kind]
                e["lens_over_radius_0_" + kind] = round(g["median"] / g0["median"], 3)
                e["composed_over_gather_" + kind] = round(c["median"] / g["median"], 3)
                e["gather_wins_beyond_spread_" + kind] = bool(g["max"] < c["min"])
            out["calls_ms"]["%s_S_%d" % (tag, S)] = e
            print(json.dumps({"aperture": tag, "S": S, "calls_ms": e}), flush=True)
            del rays

    # (d) the frames
    def frames(kw):
        def run():
            for _ in range(a.steps):
                r.display(setup, shadows=True, **kw)
        return timed(run, ctx) / a.steps

    kinds = {"no_dof": dict()}
    for tag, ap_ in apertures.items():
        for S in (4, 8, 16):
            kinds["dof_%d_%s" % (S, tag)] = dict(dof=S, dof_aperture=ap_, dof_sets=16)
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
