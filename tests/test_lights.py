"""Several lights: ugrt_shade_lights and Renderer.display(FrameSetup(..., lights=...)).

The checker of the shading is tests/lights_ref.c (built here with the oracle's flags): the arithmetic of section 6.3
restated light by light on the CPU.  The primary arrays come from the oracle's frame, and each light's shadow flags from
the oracle's shadow stage (map_rays, grid_spherical, process_rays, trace_shadow with every chunk traced), run once per
light camera."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_reflect_depth as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

_p, _f32, _i32, scene, SIZES, LG, UD = RD._p, RD._f32, RD._i32, RD.scene, RD.SIZES, RD.LG, RD.UD
ODD = (136, 72)  # 9 792 pixels: 38 blocks of 256 threads and a tail of 64
NAMES = ["hall", "crash"]


def _pn(a):
    return None if a is None else _p(a)


class LightsRef:
    def __init__(self, lib):
        self.lib = lib
        lib.lt_shade_lights.restype = C.c_int

    def shade_lights(self, cc, normal, t, dirs, ids, cam_pos, mat_idx, mat_list, light_pos, flags, p0, n, N, img=None):
        """(image, ids) of lt_shade_lights; ids (and img, if given) are copied first.  flags: [L, N] or None."""
        img = np.zeros(3 * N, np.uint8) if img is None else np.ascontiguousarray(img, np.uint8).copy()
        ids = _i32(ids).copy()
        mat_list = _f32(mat_list).reshape(-1)
        pos = _f32(np.asarray(light_pos, np.float32).reshape(-1))
        flags = None if flags is None else _i32(flags).reshape(-1)
        rc = self.lib.lt_shade_lights(_p(_f32(cc)), _p(img), _p(_f32(normal)), _p(_f32(t)), _p(_f32(dirs)), _p(ids),
                                      _p(_f32(cam_pos)), _p(_i32(mat_idx)), _p(mat_list), C.c_int(len(mat_list) // 6),
                                      C.c_int(len(pos) // 3), _p(pos), _pn(flags), C.c_longlong(N), C.c_int(p0),
                                      C.c_int(n))
        assert rc == 0
        return img, ids


@pytest.fixture(scope="session")
def LT(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lights_ref") / "liblights_ref.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-I",
                    os.path.join(ROOT, "include"), "-shared", "-o", out, os.path.join(HERE, "lights_ref.c"), "-lm"],
                   check=True, capture_output=True)
    return LightsRef(C.CDLL(out))


def lights_for(s, count=3):
    """(light_camera_params, shading_light) pairs: the scene's own light; its eye moved by a third of the scene's
    extent along x, then along y, both looking at the scene's centre, the shading light moved alike; from the fourth
    on (the 8-light case) further eyes around the centre."""
    v = np.asarray(s["verts"], np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    ext, centre = hi - lo, (lo + hi) / 2
    base = s["light_camera"]
    eye0, sl0 = np.asarray(base["eye"], np.float64), np.asarray(s["shading_light"], np.float64)
    offsets = [None, (ext[0] / 3, 0, 0), (0, ext[1] / 3, 0), (-ext[0] / 3, 0, 0), (0, -ext[1] / 3, 0),
               (ext[0] / 4, ext[1] / 4, 0), (-ext[0] / 4, ext[1] / 4, 0), (ext[0] / 4, -ext[1] / 4, -ext[2] / 4)]
    out = []
    for off in offsets[:count]:
        if off is None:
            out.append((base, tuple(float(x) for x in sl0)))
            continue
        off = np.asarray(off, np.float64)
        cam = dict(eye=tuple(float(x) for x in eye0 + off), look=tuple(float(x) for x in centre), up=(0.0, 1.0, 0.0),
                   near=base["near"], far=base["far"])
        out.append((cam, tuple(float(x) for x in sl0 + off)))
    return out


def setup_for(ugrt, s, lights=None):
    return ugrt.FrameSetup.from_scene(s, lights=lights)


_FRAMES = {}


def cpu_frame(O, ugrt, name, W, H, nlights=3, shadows=True):
    """The oracle's single-light frame (every chunk traced) plus, per light of lights_for: its camera block "cc" and,
    with shadows, its flags over the whole frame from the oracle's shadow stage.  Computed once per key and shared:
    nobody writes to it."""
    key = (name, W, H, nlights, shadows)
    if key in _FRAMES:
        return _FRAMES[key]
    s = scene(ugrt, name)
    setup = setup_for(ugrt, s)
    want = O.frame(s, setup, W, H, light_grid=LG, all_chunks=True, shadows=shadows)
    pr, N = want["primary"], W * H
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    cam_pos = want["cam"].worldori[:3].copy()
    aspect = float(np.float32(W) / np.float32(H))
    lx, ly = LG
    per = []
    for params, pos in lights_for(s, nlights):
        lcam = O.cam_from(params, setup.fovy, aspect)
        flags = None
        if shadows:
            d_map = O.map_rays(lcam.cc, pr["t"], pr["dir"], cam_pos, lx, ly, 0, N)
            lgrid = O.grid_spherical(lcam.cc, faces, verts, lx, ly)
            prefix, nchunks = O.process_rays(d_map, N, lx * ly + 1, N // 64 + lx * ly + 2)
            flags = np.zeros(N, np.int32)
            O.trace_shadow(lcam.cc, lgrid, lx * ly, verts, faces, pr["t"], pr["dir"], flags, d_map, prefix, cam_pos,
                           nchunks, (W // 8) * (H // 8), N, strict=False)
        per.append(dict(params=params, pos=pos, cc=lcam.cc.copy(), flags=flags))
    want.update(lights=per, cam_pos=cam_pos, scene=s, images={})
    _FRAMES[key] = want
    return want


def stacked_flags(want, L):
    return np.stack([lt["flags"] for lt in want["lights"][:L]])


def cpu_image(LT, want, L, shadows=True, flags=None, p0=0, n=None, img=None, ids=None, matidx=None):
    """(image, ids) of the first L lights with the last one's camera block current, as the frame leaves it."""
    pr, s = want["primary"], want["scene"]
    N = len(pr["t"])
    plain = flags is None and p0 == 0 and n is None and img is None and ids is None and matidx is None
    if plain and (L, shadows) in want["images"]:
        return want["images"][(L, shadows)]
    if flags is None and shadows:
        flags = stacked_flags(want, L)
    out = LT.shade_lights(want["lights"][L - 1]["cc"], pr["normal"], pr["t"], pr["dir"], pr["id"] if ids is None else ids,
                          want["cam_pos"], s["matidx"] if matidx is None else matidx, s["mat_list"],
                          [lt["pos"] for lt in want["lights"][:L]], flags, p0, N if n is None else n, N, img=img)
    if plain:
        want["images"][(L, shadows)] = out
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_and_prototypes_name_the_lights_call(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    assert hasattr(lib, "ugrt_shade_lights")
    assert "ugrt_shade_lights" in ugrt.PROTOTYPES
    assert hasattr(ugrt.Context, "shade_lights")
    assert ugrt.MAX_LIGHTS == 8
    pos = (C.c_float * 3)(1.0, 2.0, 3.0)
    rc = ugrt.lib.ugrt_shade_lights(None, None, None, None, None, None, None, None, None, 1, 1, pos, None)
    assert rc == ugrt.UGRT_EINVAL
    assert b"shade_lights" in ugrt.lib.ugrt_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_cpu_one_light_is_the_oracle_shading(ugrt, O, LT, name):
    """lt_shade_lights with one light == orc_shade + orc_add_shadows, image and ids, with and without flags."""
    W, H = SIZES[name]
    want = cpu_frame(O, ugrt, name, W, H)
    s, pr, N = want["scene"], want["primary"], W * H
    light = setup_for(ugrt, s).shading_light
    args = (want["lcam"].cc, pr["normal"], pr["t"], pr["dir"], pr["id"], want["cam_pos"], s["matidx"], s["mat_list"], [light])
    img, ids = LT.shade_lights(*args, want["is_shadowed"][None, :], 0, N, N)
    np.testing.assert_array_equal(img, want["image"])
    np.testing.assert_array_equal(ids, want["mat_ids"])
    img, ids = LT.shade_lights(*args, None, 0, N, N)
    np.testing.assert_array_equal(img, want["image_unshadowed"])
    np.testing.assert_array_equal(ids, want["mat_ids"])
    assert int((want["image"] != want["image_unshadowed"]).sum()) > 1000
    # the scene's own light is lights_for's first: its flags are the frame's
    np.testing.assert_array_equal(want["lights"][0]["flags"], want["is_shadowed"])


@pytest.mark.parametrize("name", NAMES)
def test_cpu_frame_tells_the_lights_apart(ugrt, O, LT, name):
    """Conditions on the oracle alone, so that the GPU tests below compare something: every light shadows and lights
    at least 1000 hit pixels, every pair of lights differs on at least 1000, and the three-light image differs from
    the one-light image on at least 1000."""
    W, H = SIZES[name]
    want = cpu_frame(O, ugrt, name, W, H)
    hit = (want["primary"]["id"] >= 0) & (want["primary"]["t"] > 0)
    flags = stacked_flags(want, 3)
    assert set(np.unique(flags)) <= {0, 1}
    for l in range(3):
        dark, lit = int((hit & (flags[l] == 1)).sum()), int((hit & (flags[l] == 0)).sum())
        print("%s light %d: %d shadowed, %d lit hit pixels" % (name, l, dark, lit))
        assert dark >= 1000 and lit >= 1000, (name, l, dark, lit)
    for a in range(3):
        for b in range(a + 1, 3):
            diff = int((flags[a] != flags[b]).sum())
            print("%s lights %d and %d: flags differ on %d pixels" % (name, a, b, diff))
            assert diff >= 1000, (name, a, b, diff)
    img3, _ = cpu_image(LT, want, 3)
    changed = int((img3.reshape(-1, 3) != want["image"].reshape(-1, 3)).any(1).sum())
    print("%s: %d pixels differ between the three-light and the one-light image" % (name, changed))
    assert changed >= 1000
    plain3, _ = cpu_image(LT, want, 3, shadows=False)
    assert int((plain3 != img3).sum()) >= 1000 and (img3 <= plain3).all()


def test_lights_are_checked_before_anything_runs(ugrt):
    from importlib import import_module

    rmod = import_module(ugrt.__name__ + ".renderer")
    cam = dict(eye=(1, 2, 3), look=(0, 0, 0), up=(0, 1, 0), near=0.1, far=100.0)
    one = (cam, (1.0, 2.0, 3.0))
    assert rmod.check_lights([one], False, False) == [(cam, (1.0, 2.0, 3.0))]
    assert len(rmod.check_lights([one] * 8, False, False)) == 8
    assert rmod.check_lights((one, (cam, np.float32([4, 5, 6]))), False, False)[1][1] == (4.0, 5.0, 6.0)
    bad_cam = dict(cam)
    del bad_cam["look"]
    for bad in ([], (), [one] * 9, [cam], [(cam,)], [(cam, (1.0, 2.0))], [(cam, "abc")], [(bad_cam, (1, 2, 3))],
                [((1, 2, 3), (1, 2, 3))], [one, None], 5, [(dict(cam, eye=(1, 2)), (1, 2, 3))]):
        with pytest.raises(ValueError):
            rmod.check_lights(bad, False, False)
    with pytest.raises(ValueError):
        rmod.check_lights([one], True, False)   # reflect
    with pytest.raises(ValueError):
        rmod.check_lights([one], False, True)   # two streams / bands


def test_frame_setup_without_lights_is_the_old_object(ugrt):
    s = scene(ugrt, "hall")
    cam = s["cameras"]["ref"]
    a = ugrt.FrameSetup(cam, s["light_camera"], s["shading_light"])
    assert a.lights is None
    assert {k: v for k, v in vars(a).items() if k != "lights"} == dict(camera=cam, light_camera=s["light_camera"],
                                                                      shading_light=s["shading_light"], fovy=45.0)
    b = ugrt.FrameSetup.from_scene(s)
    assert vars(b) == vars(a)
    ls = lights_for(s, 2)
    c = ugrt.FrameSetup.from_scene(s, lights=ls)
    assert c.lights is ls and ugrt.FrameSetup(cam, s["light_camera"], s["shading_light"], 30.0, ls).lights is ls
    assert {k: v for k, v in vars(c).items() if k != "lights"} == {k: v for k, v in vars(a).items() if k != "lights"}


class _Recorder:
    """A context that records the calls a stage enqueues."""

    def __init__(self):
        self.calls = []

    def grid_ptrs(self, which):
        return "value", "span", "offset", None

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name,) + a)


def test_trace_shadows_writes_the_frame_s_flags_unless_told(ugrt):
    import types
    from importlib import import_module

    rmod = import_module(ugrt.__name__ + ".renderer")
    f = types.SimpleNamespace(d_verts="v", d_faces="f", t="t", dir="d", is_shadowed="sh")
    b = types.SimpleNamespace(_d_map="map", _prefix="prefix", cam_pos="cam", _num_chunks=7)
    c = _Recorder()
    rmod.trace_shadows(c, f, b, c.grid_ptrs(1))
    rmod.trace_shadows(c, f, b, c.grid_ptrs(1), "row")
    assert c.calls[0] == ("trace_shadow", "value", "v", "f", "span", "offset", "t", "d", "sh", "map", "prefix", "cam", 7)
    assert c.calls[1] == c.calls[0][:8] + ("row",) + c.calls[0][9:]


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Uploaded:
    """A context with the CPU frame's arrays on the device as they are, and a camera block made current."""

    def __init__(self, ugrt, torch, want, W, H, cc, rows=None, matidx=None):
        s, pr = want["scene"], want["primary"]
        self.ctx = ctx = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD, rows=rows)
        self.N = W * H
        self.normal, self.t, self.dir = ctx.upload(pr["normal"]), ctx.upload(pr["t"]), ctx.upload(pr["dir"])
        self.cam_pos = ctx.upload(_f32(want["cam_pos"]))
        self.matidx = ctx.upload(_i32(s["matidx"] if matidx is None else matidx).reshape(-1))
        self.matlist = ctx.upload(_f32(s["mat_list"]).reshape(-1))
        self.num_materials = len(_f32(s["mat_list"]).reshape(-1)) // 6
        self.torch = torch
        ctx.upload_camera(cc)

    def shade(self, ids, light_pos, flags, img=None):
        """(image, ids) on the host after ugrt_shade_lights and a synchronise."""
        ctx, t = self.ctx, self.torch
        d_img = t.zeros(3 * self.N, dtype=t.uint8, device=ctx.device) if img is None else ctx.upload(img)
        d_ids = ctx.upload(_i32(ids))
        d_flags = None if flags is None else ctx.upload(_i32(flags).reshape(-1))
        ctx.shade_lights(d_img, self.normal, self.t, self.dir, d_ids, self.cam_pos, self.matidx, self.matlist,
                         self.num_materials, light_pos, d_flags)
        ctx.synchronize()
        return d_img.cpu().numpy(), d_ids.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_shade_lights_equals_the_cpu_restatement(ugrt, O, LT, torch, name, L):
    W, H = SIZES[name]
    want = cpu_frame(O, ugrt, name, W, H)
    up = Uploaded(ugrt, torch, want, W, H, want["lights"][L - 1]["cc"])
    pos = [lt["pos"] for lt in want["lights"][:L]]
    for shadows in (True, False):
        w_img, w_ids = cpu_image(LT, want, L, shadows=shadows)
        img, ids = up.shade(want["primary"]["id"], pos, stacked_flags(want, L) if shadows else None)
        np.testing.assert_array_equal(ids, w_ids)
        np.testing.assert_array_equal(img, w_img)
    assert int((w_img != 0).sum()) > 10000


@pytest.mark.gpu
def test_shade_eight_lights_on_a_frame_with_a_tail_block(ugrt, O, LT, torch):
    """136 x 72 = 9 792 pixels, no multiple of the block: 8 lights, flags of the first three from the oracle and random
    ones for the rest; no flags; flags with values other than 0 and 1, of which only 1 darkens."""
    W, H = ODD
    N = W * H
    assert N % 256 != 0
    want = cpu_frame(O, ugrt, "hall", W, H, nlights=8, shadows=False)
    three = cpu_frame(O, ugrt, "hall", W, H, nlights=3)
    rng = np.random.RandomState(8)
    flags = np.concatenate([stacked_flags(three, 3), rng.randint(0, 2, (5, N)).astype(np.int32)])
    odd_flags = rng.choice(np.int32([-1, 0, 1, 2, 3, 255, 256 + 1, -2 ** 31]), (8, N)).astype(np.int32)
    up = Uploaded(ugrt, torch, want, W, H, want["lights"][7]["cc"])
    pos = [lt["pos"] for lt in want["lights"]]
    images = {}
    for which, fl in (("flags", flags), ("none", None), ("odd", odd_flags)):
        w_img, w_ids = cpu_image(LT, want, 8, shadows=False, flags=fl)
        img, ids = up.shade(want["primary"]["id"], pos, fl)
        np.testing.assert_array_equal(ids, w_ids, err_msg=which)
        np.testing.assert_array_equal(img, w_img, err_msg=which)
        images[which] = img
    assert int((images["flags"] != images["none"]).sum()) > 1000
    # only == 1 darkens: the odd flags give the image of their (== 1) mask
    img, _ = up.shade(want["primary"]["id"], pos, (odd_flags == 1).astype(np.int32))
    np.testing.assert_array_equal(img, images["odd"])
    assert int((images["odd"] != images["none"]).sum()) > 1000


@pytest.mark.gpu
def test_shade_lights_bad_materials_and_an_all_miss_frame(ugrt, O, LT, torch):
    W, H = SIZES["hall"]
    N = W * H
    want = cpu_frame(O, ugrt, "hall", W, H)
    s = want["scene"]
    M = len(_f32(s["mat_list"]).reshape(-1)) // 6
    matidx = _i32(s["matidx"]).copy()
    matidx[0::5], matidx[1::5] = M, -3  # two in five triangles: one past the list, and negative
    matidx[2::50] = 2 ** 30
    pos, flags = [lt["pos"] for lt in want["lights"]], stacked_flags(want, 3)
    up = Uploaded(ugrt, torch, want, W, H, want["lights"][2]["cc"], matidx=matidx)
    w_img, w_ids = cpu_image(LT, want, 3, flags=flags, matidx=matidx)
    img, ids = up.shade(want["primary"]["id"], pos, flags)
    np.testing.assert_array_equal(ids, w_ids)
    np.testing.assert_array_equal(img, w_img)
    bad = (w_ids >= M) | (w_ids == -3)
    assert int(bad.sum()) > 1000 and not img.reshape(-1, 3)[bad].any() and int((img != 0).sum()) > 10000
    # every ray misses (ids -2, as the all-miss frame of the reference kernels has them): black, ids kept
    miss = np.full(N, -2, np.int32)
    up = Uploaded(ugrt, torch, want, W, H, want["lights"][2]["cc"])
    img, ids = up.shade(miss, pos, np.ones_like(flags), img=np.full(3 * N, 0xAB, np.uint8))
    assert not img.any()
    np.testing.assert_array_equal(ids, miss)
    w_img, w_ids = cpu_image(LT, want, 3, flags=np.ones_like(flags), ids=miss)
    np.testing.assert_array_equal(img, w_img)
    np.testing.assert_array_equal(ids, w_ids)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_light_is_shade_simple_and_add_shadows(ugrt, O, torch, name):
    """On the GPU, on one context: image and rewritten ids, byte for byte."""
    W, H = SIZES[name]
    N = W * H
    want = cpu_frame(O, ugrt, name, W, H)
    lt = want["lights"][1]
    up = Uploaded(ugrt, torch, want, W, H, lt["cc"])
    ctx = up.ctx
    for flags in (lt["flags"], None):
        img, ids = up.shade(want["primary"]["id"], [lt["pos"]], flags)
        d_img = torch.zeros(3 * N, dtype=torch.uint8, device=ctx.device)
        d_ids = ctx.upload(_i32(want["primary"]["id"]))
        ctx.set_light_position(lt["pos"])
        ctx.shade_simple(d_img, up.normal, up.t, up.dir, d_ids, up.cam_pos, up.matidx, up.matlist, up.num_materials)
        if flags is not None:
            ctx.shade_add_shadows(d_img, ctx.upload(flags))
        ctx.synchronize()
        np.testing.assert_array_equal(img, d_img.cpu().numpy())
        np.testing.assert_array_equal(ids, d_ids.cpu().numpy())
    assert int((img != 0).sum()) > 10000


@pytest.mark.gpu
def test_a_band_context_writes_exactly_its_rows(ugrt, O, LT, torch):
    W, H = SIZES["crash"]
    N, nby = W * H, H // 8
    want = cpu_frame(O, ugrt, "crash", W, H)
    pos, flags = [lt["pos"] for lt in want["lights"]], stacked_flags(want, 3)
    for rows in ((nby // 2, nby // 2 + 1), (1, nby)):
        p0, n = rows[0] * 8 * W, (rows[1] - rows[0]) * 8 * W
        ids = np.full(N, -77, np.int32)
        ids[p0:p0 + n] = want["primary"]["id"][p0:p0 + n]
        sentinel = np.full(3 * N, 0xAB, np.uint8)
        up = Uploaded(ugrt, torch, want, W, H, want["lights"][2]["cc"], rows=rows)
        assert (up.ctx.p0, up.ctx.npix) == (p0, n)
        img, got_ids = up.shade(ids, pos, flags, img=sentinel)
        w_img, w_ids = cpu_image(LT, want, 3, flags=flags, p0=p0, n=n, img=sentinel, ids=ids)
        np.testing.assert_array_equal(img, w_img)
        np.testing.assert_array_equal(got_ids, w_ids)
        full_img, full_ids = cpu_image(LT, want, 3)
        np.testing.assert_array_equal(img[3 * p0:3 * (p0 + n)], full_img[3 * p0:3 * (p0 + n)])
        np.testing.assert_array_equal(got_ids[p0:p0 + n], full_ids[p0:p0 + n])
        outside = np.ones(N, bool)
        outside[p0:p0 + n] = False
        assert (img.reshape(-1, 3)[outside] == 0xAB).all() and (got_ids[outside] == -77).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_display_with_lights_equals_the_cpu_frame(ugrt, O, LT, torch, name):
    """Three lights, the same without shadows, two lights on the same renderer (stale rows, the zeroing), then
    lights=None: the single-light frame as it has always been."""
    W, H = SIZES[name]
    want = cpu_frame(O, ugrt, name, W, H)
    s = want["scene"]
    ctx, r = RD.make(ugrt, s, W, H)
    all_lights = [(lt["params"], lt["pos"]) for lt in want["lights"]]

    def check(L, shadows):
        r.display(setup_for(ugrt, s, all_lights[:L]), frame_cnt=3, shadows=shadows)
        ctx.synchronize()
        if shadows:
            for l in range(L):
                np.testing.assert_array_equal(r.shadowed_lights[l].cpu().numpy(), want["lights"][l]["flags"],
                                              err_msg="light %d of %d" % (l, L))
        w_img, w_ids = cpu_image(LT, want, L, shadows=shadows)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids)
        np.testing.assert_array_equal(r.image.cpu().numpy(), w_img, err_msg="%d lights, shadows %s" % (L, shadows))

    assert r.shadowed_lights is None
    check(3, True)
    check(3, False)
    check(2, True)
    check(1, True)
    r.display(setup_for(ugrt, s), shadows=True)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), want["image"])
    np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), want["is_shadowed"])
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), want["mat_ids"])
    # the lights' frames never touched the single-light frame's flags beyond the primary pass's zeros
    check(2, True)
    assert r.shadowed_lights.shape[0] == 3


@pytest.mark.gpu
def test_display_rejects_what_the_lights_frame_does_not_cover(ugrt, O, torch):
    name = "hall"
    W, H = SIZES[name]
    s = scene(ugrt, name)
    ls = lights_for(s, 2)
    ctx, r = RD.make(ugrt, s, W, H)
    sentinel = torch.full_like(r.image, 0xAB)
    r.image.copy_(sentinel)
    with pytest.raises(ValueError):
        r.display(setup_for(ugrt, s, ls), reflect=True)
    with pytest.raises(ValueError):
        r.display(setup_for(ugrt, s, []))
    with pytest.raises(ValueError):
        r.display(setup_for(ugrt, s, lights_for(s, 8) + ls[:1]))
    ctx.synchronize()
    assert torch.equal(r.image, sentinel)
    for kw in (dict(overlap=True), dict(overlap=True, helper_thread=False)):
        _, two = RD.make(ugrt, s, W, H, **kw)
        with pytest.raises(ValueError):
            two.display(setup_for(ugrt, s, ls))
        two.close()
    br = ugrt.BandedRenderer(ugrt.Context, W, H, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"],
                             bands=2, light_grid=LG, uniform_dims=UD, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS)
    with pytest.raises(ValueError):
        br.display(setup_for(ugrt, s, ls), reflect=False)


@pytest.mark.gpu
def test_bad_light_counts_enqueue_nothing(ugrt, O, torch):
    W, H = ODD
    N = W * H
    want = cpu_frame(O, ugrt, "hall", W, H, nlights=8, shadows=False)
    up = Uploaded(ugrt, torch, want, W, H, want["lights"][0]["cc"])
    ctx = up.ctx
    d_img = torch.full((3 * N,), 0xAB, dtype=torch.uint8, device=ctx.device)
    d_ids = ctx.upload(_i32(want["primary"]["id"]))
    pos = [lt["pos"] for lt in want["lights"]]
    args = [d_img, up.normal, up.t, up.dir, d_ids, up.cam_pos, up.matidx, up.matlist, up.num_materials]
    for bad in ([], pos + pos[:1], None):
        with pytest.raises(ugrt.UgrtError) as e:
            ctx.shade_lights(*args, bad, None)
        assert e.value.code == ugrt.UGRT_EINVAL
        assert (b"null" if bad is None else b"num_lights") in ugrt.lib.ugrt_last_error()
    for hole in (0, 1, 4, 5, 7):
        holed = list(args)
        holed[hole] = None
        with pytest.raises(ugrt.UgrtError) as e:
            ctx.shade_lights(*holed, pos, None)
        assert e.value.code == ugrt.UGRT_EINVAL and b"null" in ugrt.lib.ugrt_last_error()
    ctx.synchronize()
    assert bool((d_img == 0xAB).all())
    np.testing.assert_array_equal(d_ids.cpu().numpy(), want["primary"]["id"])
    ctx.shade_lights(*args, pos, None)  # the context is still usable
    ctx.synchronize()
    assert int((d_img != 0xAB).sum()) > 1000
