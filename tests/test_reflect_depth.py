"""Reflections of depth D through the uniform grid: ugrt_reflect_rays_next,
ugrt_shade_reflect_depth and Renderer / BandedRenderer.display(..., bounces=D).

The checker is tests/reflect_depth_ref.c (built here with the oracle's flags): the next-ray and depth-D shading
arithmetic restated on the CPU; the levels in between are traced with the oracle's orc_trace_dda."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="session")
def REF(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("reflect_depth_ref") / "libreflect_depth_ref.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-I",
                    os.path.join(ROOT, "include"), "-shared", "-o", out, os.path.join(HERE, "reflect_depth_ref.c"),
                    "-lm"], check=True, capture_output=True)
    return DepthRef(C.CDLL(out))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class DepthRef:
    def __init__(self, lib):
        self.lib = lib

    def reflect_rays(self, cam_pos, t, dirs, ids, mat_idx, reflect, verts, faces, eps, p0, n, N):
        rays, active = np.zeros(6 * N, np.float32), np.zeros(N, np.int32)
        reflect = _f32(reflect)
        self.lib.rd_reflect_rays(_p(_f32(cam_pos)), _p(_f32(t)), _p(_f32(dirs)), _p(_i32(ids)), _p(_i32(mat_idx)),
                                 _p(reflect), C.c_int(len(reflect)), _p(_f32(verts).reshape(-1)),
                                 _p(_i32(faces).reshape(-1)), C.c_float(eps), C.c_int(p0), C.c_int(n), _p(rays),
                                 _p(active))
        return rays, active

    def reflect_rays_next(self, rays, active, hit_t, hit_id, mat_idx, reflect, verts, faces, eps, p0, n, N):
        rn, an = np.zeros(6 * N, np.float32), np.zeros(N, np.int32)
        reflect = _f32(reflect)
        self.lib.rd_reflect_rays_next(_p(_f32(rays)), _p(_i32(active)), _p(_f32(hit_t)), _p(_i32(hit_id)),
                                      _p(_i32(mat_idx)), _p(reflect), C.c_int(len(reflect)),
                                      _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)), C.c_float(eps),
                                      C.c_int(p0), C.c_int(n), _p(rn), _p(an))
        return rn, an

    def shade_depth(self, cc, light, normal, t, dirs, ids, cam_pos, mat_idx, mat_list, reflect, verts, faces, depth,
                    rays, active, hit_t, hit_id, p0, n, N):
        img = np.zeros(3 * N, np.uint8)
        ids = _i32(ids).copy()
        mat_list = _f32(mat_list).reshape(-1)
        args = [_f32(a) for a in (rays, hit_t)] + [_i32(a) for a in (active, hit_id)]
        self.lib.rd_shade_depth(_p(_f32(cc)), _p(_f32(light)), _p(img), _p(_f32(normal)), _p(_f32(t)),
                                _p(_f32(dirs)), _p(ids), _p(_f32(cam_pos)), _p(_i32(mat_idx)), _p(mat_list),
                                _p(_f32(reflect)), C.c_int(len(mat_list) // 6), _p(_f32(verts).reshape(-1)),
                                _p(_i32(faces).reshape(-1)), C.c_int(depth), C.c_longlong(N), _p(args[0]),
                                _p(args[2]), _p(args[1]), _p(args[3]), C.c_int(p0), C.c_int(n))
        return img, ids


def cpu_frame(O, REF, s, setup, W, H, depth, rows=None, lg=(64, 64), ud=(32, 32, 16), eps=1e-3, brute=False):
    """The depth-D frame on the CPU: the oracle's frame (primary, shadows with every chunk, uniform grid, level 1),
    levels 2..D from REF.reflect_rays_next + the oracle's trace_dda, the image from REF.shade_depth + add_shadows.
    Returns the oracle's frame dict with "levels" (per level: rays, active, hit_t, hit_id) and "image_depth"."""
    want = O.frame(s, setup, W, H, rows=rows, light_grid=lg, reflect=True, uniform_dims=ud, all_chunks=True,
                   reflect_eps=eps)
    p0, n, N = want["p0"], want["n"], W * H
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    levels = [dict(rays=want["rays"], active=want["active"], hit_t=want["hit_t"], hit_id=want["hit_id"])]
    for _ in range(1, depth):
        lv = levels[-1]
        rays, active = REF.reflect_rays_next(lv["rays"], lv["active"], lv["hit_t"], lv["hit_id"], s["matidx"],
                                             s["reflect"], verts, faces, eps, p0, n, N)
        if brute:
            hit_t, hit_id = O.brute_nearest(verts, faces, rays, active, p0, n, N)
        else:
            hit_t, hit_id, _ = O.trace_dda(want["ugrid"], verts, faces, rays, active, p0, n, N)
        levels.append(dict(rays=rays, active=active, hit_t=hit_t, hit_id=hit_id))
    pr = want["primary"]
    stack = {k: np.concatenate([lv[k] for lv in levels]) for k in ("rays", "active", "hit_t", "hit_id")}
    img, ids = REF.shade_depth(want["lcam"].cc, setup.shading_light, pr["normal"], pr["t"], pr["dir"], pr["id"],
                               want["cam"].worldori[:3], s["matidx"], s["mat_list"], s["reflect"], verts, faces,
                               depth, stack["rays"], stack["active"], stack["hit_t"], stack["hit_id"], p0, n, N)
    O.add_shadows(img, want["is_shadowed"], p0, n)
    want.update(levels=levels, image_depth=img, mat_ids_depth=ids)
    return want


SCENES = {}


def scene(ugrt, name):
    if name not in SCENES:
        SCENES[name] = {"hall": lambda: ugrt.scenes.hall(scale=0.1), "crash": lambda: ugrt.scenes.crash(scale=0.02),
                        "mirrors": lambda: ugrt.scenes.mirrors(scale=0.1)}[name]()
    return SCENES[name]


SIZES = {"hall": (256, 256), "crash": (256, 144), "mirrors": (256, 256)}
LG, UD = (64, 64), (32, 32, 16)


def setup_for(ugrt, s):
    return ugrt.FrameSetup.from_scene(s)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_and_prototypes_name_the_depth_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in ("ugrt_reflect_rays_next", "ugrt_shade_reflect_depth"):
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    assert ugrt.MAX_REFLECT_DEPTH == 8


@pytest.mark.parametrize("name", ["hall", "crash"])
def test_cpu_depth1_is_the_oracle_frame(ugrt, O, REF, name):
    """The restatement at depth 1 gives the oracle's single-bounce image and material ids byte for byte."""
    s = scene(ugrt, name)
    W, H = SIZES[name]
    want = cpu_frame(O, REF, s, setup_for(ugrt, s), W, H, 1, lg=LG, ud=UD)
    np.testing.assert_array_equal(want["image_depth"], want["image"])
    np.testing.assert_array_equal(want["mat_ids_depth"], want["mat_ids"])
    assert (want["active"] == 1).sum() > 1000


@pytest.mark.parametrize("name", ["hall", "mirrors"])
def test_cpu_level1_rays_are_the_oracle_rays(ugrt, O, REF, name):
    s = scene(ugrt, name)
    W, H = SIZES[name]
    setup = setup_for(ugrt, s)
    want = O.frame(s, setup, W, H, light_grid=LG, reflect=True, uniform_dims=UD, shadows=False)
    pr, N = want["primary"], W * H
    cam_pos = want["cam"].worldori[:3]
    rays, active = REF.reflect_rays(cam_pos, pr["t"], pr["dir"], pr["id"], s["matidx"], s["reflect"], s["verts"],
                                    s["faces"], 1e-3, 0, N, N)
    orays, oactive = O.reflect_rays(cam_pos, pr["t"], pr["dir"], pr["id"], s["matidx"], s["reflect"], s["verts"],
                                    s["faces"], 1e-3, 0, N, N)
    np.testing.assert_array_equal(active, oactive)
    np.testing.assert_array_equal(bits(rays), bits(orays))
    np.testing.assert_array_equal(bits(rays), bits(want["rays"]))


def test_cpu_levels_are_the_nearest_hits(ugrt, O, REF):
    """Depth 3 on mirrors: the grid walk of every level finds what a test against every triangle finds."""
    s = scene(ugrt, "mirrors")
    W, H = SIZES["mirrors"]
    setup = setup_for(ugrt, s)
    dda = cpu_frame(O, REF, s, setup, W, H, 3, lg=LG, ud=UD)
    brute = cpu_frame(O, REF, s, setup, W, H, 3, lg=LG, ud=UD, brute=True)
    for j, (a, b) in enumerate(zip(dda["levels"], brute["levels"])):
        np.testing.assert_array_equal(a["active"], b["active"], err_msg="level %d" % (j + 1))
        np.testing.assert_array_equal(a["hit_id"], b["hit_id"], err_msg="level %d" % (j + 1))
        np.testing.assert_array_equal(bits(a["hit_t"]), bits(b["hit_t"]), err_msg="level %d" % (j + 1))
    bt, bi = O.brute_nearest(s["verts"], s["faces"], dda["rays"], dda["active"], 0, W * H, W * H)
    np.testing.assert_array_equal(bi, dda["hit_id"])


def test_cpu_depth_is_not_vacuous(ugrt, O, REF):
    """Counts of the restatement (256x256; see DESIGN.md section 6 for the figures): mirrors keeps about half of its
    pixels active at level 2 and ~750 at level 8, hall ~5800 at level 2; every extra level changes pixels."""
    N = 256 * 256
    s = scene(ugrt, "mirrors")
    m = cpu_frame(O, REF, s, setup_for(ugrt, s), 256, 256, 8, lg=LG, ud=UD)
    act = [int(lv["active"].sum()) for lv in m["levels"]]
    assert act[1] >= N // 4, act
    assert act[7] >= 300, act
    assert int((m["levels"][7]["hit_id"] >= 0).sum()) >= 200
    assert int((m["levels"][1]["hit_id"] < 0).sum() - (m["levels"][1]["active"] == 0).sum()) > 1000  # misses
    h = scene(ugrt, "hall")
    hw = cpu_frame(O, REF, h, setup_for(ugrt, h), 256, 256, 2, lg=LG, ud=UD)
    assert int(hw["levels"][1]["active"].sum()) >= 2000
    assert int((hw["image_depth"] != hw["image"]).reshape(-1, 3).any(1).sum()) >= 1000
    prev = None
    for d in range(1, 9):
        img = cpu_frame(O, REF, s, setup_for(ugrt, s), 256, 256, d, lg=LG, ud=UD)["image_depth"].reshape(-1, 3)
        if prev is not None:
            assert int((img != prev).any(1).sum()) >= 300, d
        prev = img


def test_bounces_are_checked_before_anything_runs(ugrt):
    from importlib import import_module

    rmod = import_module(ugrt.__name__ + ".renderer")
    for bad in (0, 9, -1, 1.5, True, "2", None):
        with pytest.raises(ValueError):
            rmod.check_bounces(bad)
    assert [rmod.check_bounces(d) for d in range(1, 9)] == list(range(1, 9))
    assert rmod.check_bounces(np.int64(3)) == 3


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def gpu_levels(r, depth):
    out = []
    for j in range(depth):
        out.append(dict(rays=r.rays_levels[j].cpu().numpy(), active=r.active_levels[j].cpu().numpy(),
                         hit_t=r.hit_t_levels[j].cpu().numpy(), hit_id=r.hit_id_levels[j].cpu().numpy()))
    return out


def assert_frame_equals(r, want, depth, rows=None):
    """Every level's active / rays / hit_t / hit_id and the image + material ids, over the CPU frame's band."""
    a, b = want["p0"], want["p0"] + want["n"]
    got = gpu_levels(r, depth) if depth > 1 else [dict(rays=r.rays.cpu().numpy(), active=r.active.cpu().numpy(),
                                                        hit_t=r.hit_t.cpu().numpy(), hit_id=r.hit_id.cpu().numpy())]
    for j, (g, w) in enumerate(zip(got, want["levels"])):
        what = "level %d" % (j + 1)
        np.testing.assert_array_equal(g["active"][a:b], w["active"][a:b], err_msg=what)
        np.testing.assert_array_equal(bits(g["rays"][6 * a:6 * b]), bits(w["rays"][6 * a:6 * b]), err_msg=what)
        np.testing.assert_array_equal(g["hit_id"][a:b], w["hit_id"][a:b], err_msg=what)
        np.testing.assert_array_equal(bits(g["hit_t"][a:b]), bits(w["hit_t"][a:b]), err_msg=what)
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy()[a:b], want["mat_ids_depth"][a:b])
    np.testing.assert_array_equal(r.image.cpu().numpy()[3 * a:3 * b], want["image_depth"][3 * a:3 * b])


def make(ugrt, s, W, H, **kw):
    ctx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
    return ctx, ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "crash"])
def test_depth1_is_shade_reflect(ugrt, torch, name):
    """shade_reflect_depth at depth 1 writes shade_reflect's image and material ids byte for byte."""
    s = scene(ugrt, name)
    W, H = SIZES[name]
    ctx, r = make(ugrt, s, W, H)
    r.display(setup_for(ugrt, s), shadows=True, reflect=True, shade=False)
    r._ensure_reflect_buffers()
    ctx.reflect_rays(r.cam_pos, r.t, r.dir, r.intersect_id, r.d_matidx, r.d_reflect, r.num_materials, r.d_verts,
                     r.d_faces, r.reflect_eps, r.rays, r.active)
    ctx.grid_build_uniform(r.d_faces, r.d_verts, r.F, r.bbmin, r.bbmax)
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    ctx.trace_dda(uvalue, uspan, uoffset, r.d_verts, r.d_faces, r.rays, r.active, r.hit_t, r.hit_id)
    ids_a, ids_b = r.intersect_id.clone(), r.intersect_id.clone()
    img_a, img_b = torch.zeros_like(r.image), torch.full_like(r.image, 7)
    ctx.shade_reflect(img_a, r.normal, r.t, r.dir, ids_a, r.cam_pos, r.d_matidx, r.d_matlist, r.d_reflect,
                      r.num_materials, r.d_verts, r.d_faces, r.rays, r.active, r.hit_t, r.hit_id)
    ctx.shade_reflect_depth(img_b, r.normal, r.t, r.dir, ids_b, r.cam_pos, r.d_matidx, r.d_matlist, r.d_reflect,
                            r.num_materials, r.d_verts, r.d_faces, 1, r.rays, r.active, r.hit_t, r.hit_id)
    ctx.synchronize()
    assert torch.equal(img_a, img_b)
    assert torch.equal(ids_a, ids_b)
    assert int(r.active.sum()) > 1000 and int((img_a != 0).sum()) > 10000


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3, 4, 8])
@pytest.mark.parametrize("name", ["hall", "crash", "mirrors"])
def test_levels_equal_the_cpu_reference(ugrt, O, REF, torch, name, depth):
    s = scene(ugrt, name)
    W, H = SIZES[name]
    setup = setup_for(ugrt, s)
    ctx, r = make(ugrt, s, W, H)
    r.display(setup, shadows=True, reflect=True, bounces=depth)
    ctx.synchronize()
    want = cpu_frame(O, REF, s, setup, W, H, depth, lg=LG, ud=UD)
    assert r.rays.data_ptr() == r.rays_levels[0].data_ptr() and r.hit_id.data_ptr() == r.hit_id_levels[0].data_ptr()
    assert_frame_equals(r, want, depth)
    assert int(want["levels"][1]["active"].sum()) > 0


@pytest.mark.gpu
def test_launch_options_do_not_change_the_levels(ugrt, O, REF, torch):
    """Kernels, rays per wave, split walks (whose history now crosses levels inside a frame) and the ray sort of the
    DDA: two frames each, the same levels and image."""
    s = scene(ugrt, "mirrors")
    W, H = SIZES["mirrors"]
    setup = setup_for(ugrt, s)
    depth = 4
    want = cpu_frame(O, REF, s, setup, W, H, depth, lg=LG, ud=UD)
    combos = [{"dda_kernel": 0}, {"dda_kernel": 1}, {"dda_rays_per_wave": 16}, {"dda_rays_per_wave": 64},
              {"dda_split": 0}, {"dda_split": 1, "dda_split_load": 50}, {"dda_split": 4, "dda_split_load": 50},
              {"dda_sort": 1}]
    for opts in combos:
        ctx, r = make(ugrt, s, W, H)
        for k, v in opts.items():
            ctx.set_option(k, v)
        for _ in range(2):
            r.display(setup, shadows=True, reflect=True, bounces=depth)
        ctx.synchronize()
        try:
            assert_frame_equals(r, want, depth)
        except AssertionError as e:
            raise AssertionError("options %s: %s" % (opts, e))


def _paths_renderers(ugrt, s, W, H):
    """The plain, overlapped (helper thread) and inline two-stream renderers."""
    flags = ugrt.FLAG_SHADOW_ALL_CHUNKS
    out = {}
    for name, kw in (("plain", {}), ("overlapped", dict(overlap=True)),
                     ("inline", dict(overlap=True, helper_thread=False))):
        ctx = ugrt.Context(W, H, light_grid=LG, flags=flags, uniform_dims=UD)
        out[name] = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], **kw)
    return out


@pytest.mark.gpu
def test_display_paths_agree_at_depth_3(ugrt, O, REF, torch):
    s = scene(ugrt, "mirrors")
    W, H = 320, 192
    setup = setup_for(ugrt, s)
    want = cpu_frame(O, REF, s, setup, W, H, 3, lg=LG, ud=UD)
    rs = _paths_renderers(ugrt, s, W, H)
    for name, r in rs.items():
        r.display(setup, shadows=True, reflect=True, bounces=3)
        r.synchronize()
        torch.cuda.synchronize()
        assert_frame_equals(r, want, 3)
        r.close()
    br = ugrt.BandedRenderer(ugrt.Context, W, H, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"],
                             bands=3, light_grid=LG, uniform_dims=UD, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS)
    for _ in range(2):
        br.display(setup, shadows=True, reflect=True, bounces=3)
    br.synchronize()
    torch.cuda.synchronize()
    assert_frame_equals(br, want, 3)
    assert br.rays.data_ptr() == br.rays_levels[0].data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("async_build", [1, 0])
def test_four_renderers_in_flight_equal_a_sequential_context(ugrt, torch, async_build):
    """Four two-stream renderers fed from one host thread, depth 3, frames dealt round-robin without a wait: each
    equals a plain single-context frame over every level."""
    s = scene(ugrt, "crash")
    W, H = 384, 216
    setup = setup_for(ugrt, s)
    seq_ctx, seq = make(ugrt, s, W, H)
    seq.display(setup, shadows=True, reflect=True, bounces=3)
    seq_ctx.synchronize()
    renderers = []
    for i in range(4):
        stream = torch.cuda.Stream() if i else None
        with torch.cuda.stream(stream):
            cx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
            rr = ugrt.Renderer(cx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], overlap=True,
                               helper_thread=False)
        for c in (rr.ctx, rr.aux):
            c.set_option("async_build", async_build)
        rr._stream = stream
        renderers.append(rr)
    for k in range(8):
        rr = renderers[k % 4]
        with torch.cuda.stream(rr._stream):
            rr.display(setup, shadows=True, reflect=True, bounces=3)
    for rr in renderers:
        rr.synchronize()
    torch.cuda.synchronize()
    for i, rr in enumerate(renderers):
        for n in ("image", "intersect_id", "is_shadowed", "rays_levels", "active_levels", "hit_t_levels",
                  "hit_id_levels"):
            a, b = getattr(rr, n), getattr(seq, n)
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (i, n)
    assert int(seq.active_levels[2].sum()) > 0


@pytest.mark.gpu
def test_full_size_depth_3_bands(ugrt, O, REF, torch):
    """The bench workload (1 M triangles, 1920x1080) at depth 3; four bands of tile rows against the CPU reference."""
    s = ugrt.scenes.crash(scale=1.0)
    W, H, lg, ud = 1920, 1080, (128, 128), (128, 128, 64)
    ctx = ugrt.Context(W, H, light_grid=lg, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    setup = setup_for(ugrt, s)
    r.display(setup, shadows=True, reflect=True, bounces=3)
    ctx.synchronize()
    act = [int(a.sum()) for a in r.active_levels[:3]]
    assert act[0] > 10 ** 5 and act[1] > 0, act
    for rows in ((10, 12), (50, 53), (66, 70), (120, 122)):
        want = cpu_frame(O, REF, s, setup, W, H, 3, rows=rows, lg=lg, ud=ud)
        assert_frame_equals(r, want, 3)


@pytest.mark.gpu
def test_bad_arguments_leave_the_context_usable(ugrt, O, REF, torch):
    s = scene(ugrt, "hall")
    W, H = SIZES["hall"]
    setup = setup_for(ugrt, s)
    ctx, r = make(ugrt, s, W, H)
    r.display(setup, shadows=True, reflect=True, bounces=2)
    ctx.synchronize()
    for depth in (0, 9, -3):
        with pytest.raises(ugrt.UgrtError) as e:
            ctx.shade_reflect_depth(r.image, r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.d_matlist,
                                    r.d_reflect, r.num_materials, r.d_verts, r.d_faces, depth, r.rays_levels,
                                    r.active_levels, r.hit_t_levels, r.hit_id_levels)
        assert e.value.code == ugrt.UGRT_EINVAL and b"depth" in ugrt.lib.ugrt_last_error()
    with pytest.raises(ugrt.UgrtError) as e:
        ctx.shade_reflect_depth(r.image, r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.d_matlist,
                                r.d_reflect, r.num_materials, r.d_verts, r.d_faces, 2, None, r.active_levels,
                                r.hit_t_levels, r.hit_id_levels)
    assert e.value.code == ugrt.UGRT_EINVAL and b"null" in ugrt.lib.ugrt_last_error()
    with pytest.raises(ugrt.UgrtError) as e:
        ctx.reflect_rays_next(r.rays, r.active, r.hit_t, None, r.d_matidx, r.d_reflect, r.num_materials, r.d_verts,
                              r.d_faces, 1e-3, r.rays_levels[1], r.active_levels[1])
    assert e.value.code == ugrt.UGRT_EINVAL and b"null" in ugrt.lib.ugrt_last_error()
    br = ugrt.BandedRenderer(ugrt.Context, W, H, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"],
                             bands=2, light_grid=LG, uniform_dims=UD, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            r.display(setup, shadows=True, reflect=True, bounces=bad)
        with pytest.raises(ValueError):
            br.display(setup, shadows=True, reflect=True, bounces=bad)
    r.display(setup, shadows=True, reflect=True, bounces=3)
    ctx.synchronize()
    assert_frame_equals(r, cpu_frame(O, REF, s, setup, W, H, 3, lg=LG, ud=UD), 3)
