"""Reflections under several lights: ugrt_trace_dda_any_lights, ugrt_shade_reflect_lights and
Renderer.display(FrameSetup(..., lights=...), reflect=True, reflect_lights=True).

The checker of the shading is tests/reflect_lights_ref.c (built here with the oracle's flags): the arithmetic of section
6.4 restated light by light on the CPU.  The any-hit side has no restatement of its own: the expected flags are
oc_occlusion_rays + oc_trace_any of tests/occlusion_ref.c, once per light.  The reflection levels come from the CPU frame
of tests/test_reflect_shadows.py, the lights and their primary shadow flags from the one of tests/test_lights.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_lights as TL
import test_reflect_depth as RD
import test_reflect_shadows as RS
from test_reflect_shadows import REFS, SYN  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

_p, _f32, _i32, bits, scene, SIZES, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.scene, RD.SIZES, RD.LG, RD.UD
ODD = TL.ODD  # 136 x 72 = 9 792 pixels: 38 blocks of 256 threads and a tail of 64
CALLS = ("ugrt_trace_dda_any_lights", "ugrt_shade_reflect_lights")
EPS = 1e-3


def _pn(a):
    return None if a is None else _p(a)


class ReflectLightsRef:
    def __init__(self, lib):
        self.lib = lib
        lib.rl_shade.restype = C.c_int

    def shade(self, cc, normal, t, dirs, ids, cam_pos, mat_idx, mat_list, reflect, verts, faces, depth, rays, active,
              hit_t, hit_id, light_pos, flags, occluded, p0, n, N, img=None):
        """(image, ids) of rl_shade; ids (and img, if given) are copied first.  flags: [L, N] or None; occluded:
        [depth, L, N] or None."""
        img = np.zeros(3 * N, np.uint8) if img is None else np.ascontiguousarray(img, np.uint8).copy()
        ids = _i32(ids).copy()
        mat_list = _f32(mat_list).reshape(-1)
        pos = _f32(np.asarray(light_pos, np.float32).reshape(-1))
        flags = None if flags is None else _i32(flags).reshape(-1)
        occluded = None if occluded is None else _i32(occluded).reshape(-1)
        rc = self.lib.rl_shade(_p(_f32(cc)), _p(img), _p(_f32(normal)), _p(_f32(t)), _p(_f32(dirs)), _p(ids),
                               _p(_f32(cam_pos)), _p(_i32(mat_idx)), _p(mat_list), _p(_f32(reflect)),
                               C.c_int(len(mat_list) // 6), _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)),
                               C.c_int(depth), C.c_longlong(N), _p(_f32(rays)), _p(_i32(active)), _p(_f32(hit_t)),
                               _p(_i32(hit_id)), C.c_int(len(pos) // 3), _p(pos), _pn(flags), _pn(occluded), C.c_int(p0),
                               C.c_int(n))
        assert rc == 0
        return img, ids


@pytest.fixture(scope="session")
def RL(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("reflect_lights_ref") / "libreflect_lights_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "reflect_lights_ref.c"), "-lm"], check=True, capture_output=True)
    return ReflectLightsRef(C.CDLL(out))


_FRAMES, _OCCLUDED = {}, {}


def light_eye(O, lt, W, H):
    """The point the occlusion rays of a light aim at: its camera's eye, as the primary shadow pass is cast from it."""
    return O.cam_from(lt["params"], 45.0, float(np.float32(W) / np.float32(H))).worldori[:3].copy()


def level_occluded(O, REFS, base, s, key, j, eye):
    """oc_occlusion_rays + oc_trace_any of level j + 1 towards one eye; computed once per key and shared."""
    if key not in _OCCLUDED:
        OC, lv = REFS[1], base["levels"][j]
        verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
        p0, n, N = base["p0"], base["n"], len(lv["active"])
        orays, oactive = OC.occlusion_rays(lv["rays"], lv["active"], lv["hit_t"], lv["hit_id"], verts, faces, eye, EPS, p0, n, N)
        _OCCLUDED[key] = OC.trace_any(base["ugrid"], verts, faces, orays, oactive, 1.0, p0, n, N)
    return _OCCLUDED[key]


def cpu_frame(O, REFS, RL, ugrt, name, W, H, depth, L=3, nlights=3, shadows=True):
    """The CPU frame under the first L of lights_for(s, nlights): the reflection levels of test_reflect_shadows' frame
    (they do not know the light), per light the oracle's shadow stage (test_lights' frame) and per level and light the
    occlusion flags, then rl_shade with the last light's camera block current, as the frame leaves it.  Computed once
    per key and shared: nobody writes to it."""
    key = (name, W, H, depth, L, nlights, shadows)
    if key in _FRAMES:
        return _FRAMES[key]
    s = scene(ugrt, name)
    base = RS.cpu_frame(O, REFS, ugrt, name, W, H, depth)
    lw = TL.cpu_frame(O, ugrt, name, W, H, nlights=nlights, shadows=shadows)
    lights = lw["lights"][:L]
    eyes = [light_eye(O, lt, W, H) for lt in lights]
    occluded = np.stack([np.stack([level_occluded(O, REFS, base, s, (name, W, H, nlights, j, l), j, eyes[l]) for l in range(L)])
                         for j in range(depth)])
    flags = np.stack([lt["flags"] for lt in lights]) if shadows else None
    pr, st = base["primary"], base["stack"]
    want = dict(base=base, scene=s, lights=lights, eyes=eyes, occluded=occluded, flags=flags, p0=base["p0"], n=base["n"],
                cam_pos=base["cam"].worldori[:3].copy(), N=W * H, depth=depth)
    want["shade_args"] = (pr["normal"], pr["t"], pr["dir"], pr["id"], want["cam_pos"], s["matidx"], s["mat_list"], s["reflect"],
                          s["verts"], s["faces"], depth, st["rays"], st["active"], st["hit_t"], st["hit_id"])
    want["image"], want["mat_ids"] = RL.shade(lights[-1]["cc"], *want["shade_args"], [lt["pos"] for lt in lights], flags,
                                              occluded, base["p0"], base["n"], W * H)
    _FRAMES[key] = want
    return want


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_and_prototypes_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    for name in ("trace_dda_any_lights", "shade_reflect_lights"):
        assert hasattr(ugrt.Context, name), name
    header = open(os.path.join(ROOT, "include", "ugrt.h")).read()
    for name in CALLS:
        assert "int %s(ugrt_ctx *ctx" % name in header
    pos = (C.c_float * 3)(1.0, 2.0, 3.0)
    assert ugrt.lib.ugrt_trace_dda_any_lights(None, None, None, None, None, None, None, None, 1, pos, None) == ugrt.UGRT_EINVAL
    assert b"trace_dda_any_lights" in ugrt.lib.ugrt_last_error()
    rc = ugrt.lib.ugrt_shade_reflect_lights(*([None] * 10 + [1, None, None, 1] + [None] * 4 + [1, pos, None, None]))
    assert rc == ugrt.UGRT_EINVAL
    assert b"shade_reflect_lights" in ugrt.lib.ugrt_last_error()


def _rmod(ugrt):
    from importlib import import_module

    return import_module(ugrt.__name__ + ".renderer")


def test_check_lights_keeps_its_three_arguments_and_the_fourth_admits_reflect(ugrt):
    rmod = _rmod(ugrt)
    cam = dict(eye=(1, 2, 3), look=(0, 0, 0), up=(0, 1, 0), near=0.1, far=100.0)
    one = (cam, (1.0, 2.0, 3.0))
    assert rmod.check_lights([one], False, False) == [(cam, (1.0, 2.0, 3.0))]
    with pytest.raises(ValueError):
        rmod.check_lights([one], True, False)
    with pytest.raises(ValueError):
        rmod.check_lights([one], True, False, False)
    with pytest.raises(ValueError):
        rmod.check_lights([one], False, True)
    assert rmod.check_lights([one], True, False, True) == [(cam, (1.0, 2.0, 3.0))]
    assert len(rmod.check_lights([one] * 8, True, False, True)) == 8
    for bad in ([], [one] * 9, [cam], 5):
        with pytest.raises(ValueError):
            rmod.check_lights(bad, True, False, True)
    with pytest.raises(ValueError):
        rmod.check_lights([one], True, True, True)   # two streams / bands: exclusion (2) stands
    assert rmod.check_reflect_lights(True, True, [one]) is True
    assert rmod.check_reflect_lights(np.bool_(True), True, [one]) is True
    assert rmod.check_reflect_lights(False, False, None) is False and rmod.check_reflect_lights(False, True, [one]) is False
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            rmod.check_reflect_lights(bad, True, [one])
    with pytest.raises(ValueError):
        rmod.check_reflect_lights(True, False, [one])
    with pytest.raises(ValueError):
        rmod.check_reflect_lights(True, True, None)


def _fake_renderer(ugrt, aux=None):
    """A Renderer that was never constructed, around a context that records: what display() checks comes first."""
    r = object.__new__(ugrt.Renderer)
    r.ctx, r.aux = RS._Recorder(), aux
    return r


def test_reflect_lights_is_checked_before_anything_runs(ugrt):
    s = scene(ugrt, "hall")
    ls = TL.lights_for(s, 2)
    for setup, kw in ((TL.setup_for(ugrt, s), dict(reflect=True)),                     # no lights
                      (TL.setup_for(ugrt, s, ls), dict(reflect=False)),                # no reflect
                      (TL.setup_for(ugrt, s, ls), dict(reflect=True, bounces=9)),
                      (TL.setup_for(ugrt, s, []), dict(reflect=True)),
                      (TL.setup_for(ugrt, s, ls), dict(reflect=False, reflect_shadows=True))):
        r = _fake_renderer(ugrt)
        with pytest.raises(ValueError):
            r.display(setup, reflect_lights=True, **kw)
        assert r.ctx.calls == []
    r = _fake_renderer(ugrt)
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s, ls), reflect=True, reflect_lights=1)
    r = _fake_renderer(ugrt, aux=object())  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s, ls), reflect=True, reflect_lights=True)
    # without the keyword the errors of section 6.3 are what they were
    r = _fake_renderer(ugrt)
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s, ls), reflect=True)
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s, ls), reflect=True, reflect_lights=False)
    assert r.ctx.calls == []


def test_stages_enqueue_one_ray_launch_and_one_walk_per_level(ugrt):
    rmod = _rmod(ugrt)
    f = RS._fake_frame(3)
    f.occluded_lights = ["occl%d" % (j + 1) for j in range(3)]
    f.shadowed_lights = "shl"
    eyes = [(1.0, 2.0, 3.0), (4.0, 5.0, 6.0), (7.0, 8.0, 9.0)]
    off, single, on = RS._Recorder(), RS._Recorder(), RS._Recorder()
    rmod.trace_reflections(off, f, 3)
    rmod.trace_reflections(single, f, 3, (1.0, 2.0, 3.0))
    rmod.trace_reflections(on, f, 3, shadow_lights=eyes)
    # reflect_lights off: exactly today's calls
    assert [c[0] for c in off.calls] == ["trace_dda", "reflect_rays_next", "trace_dda", "reflect_rays_next", "trace_dda"]
    assert [c[0] for c in single.calls] == ["trace_dda", "occlusion_rays", "trace_dda_any", "reflect_rays_next"] * 2 + \
        ["trace_dda", "occlusion_rays", "trace_dda_any"]
    assert single.calls[2][1:] == ("value", "span", "offset", "v", "f", "orays", "oact", 1.0, "occluded1")
    # on: the level calls unchanged, one occlusion_rays (towards the first eye) and one walk per level
    assert [c for c in on.calls if c[0] not in ("occlusion_rays", "trace_dda_any_lights")] == off.calls
    assert [c[0] for c in on.calls] == ["trace_dda", "occlusion_rays", "trace_dda_any_lights", "reflect_rays_next"] * 2 + \
        ["trace_dda", "occlusion_rays", "trace_dda_any_lights"]
    for j in range(3):
        rays, walk = [c for c in on.calls if c[0] in ("occlusion_rays", "trace_dda_any_lights")][2 * j:2 * j + 2]
        lv = tuple("%s%d" % (n, j + 1) for n in ("rays", "active", "hit_t", "hit_id"))
        assert rays[1:] == lv + ("v", "f", eyes[0], 1e-3, "orays", "oact")
        assert walk[1:] == ("value", "span", "offset", "v", "f", "orays", "oact", eyes, "occl%d" % (j + 1))
    lights = [("cam%d" % l, (float(l), 0.0, 1.0)) for l in range(3)]
    for shadows, rs in ((True, True), (False, True), (True, False), (False, False)):
        c = RS._Recorder()
        rmod.shade_reflect_lights(c, f, "cam", lights, 3, shadows, rs)
        assert [x[0] for x in c.calls] == ["shade_reflect_lights"]
        assert c.calls[0][13:] == (3, f.rays_levels, f.active_levels, f.hit_t_levels, f.hit_id_levels,
                                   [pos for _, pos in lights], "shl" if shadows else None, f.occluded_lights if rs else None)
    # shade_frame is untouched by the option
    c = RS._Recorder()
    rmod.shade_frame(c, f, "cam", 1, True, True, 3, True)
    assert [x[0] for x in c.calls] == ["shade_reflect_depth_occluded", "shade_add_shadows"]


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("name", ["hall", "mirrors"])
def test_cpu_one_light_is_the_single_light_shading(ugrt, O, REFS, RL, name, depth):
    """rl_shade with one light == oc_shade_depth_occluded + orc_add_shadows byte for byte, ids included; without the
    occlusion flags == rd_shade_depth + orc_add_shadows."""
    W, H = SIZES[name]
    base = RS.cpu_frame(O, REFS, ugrt, name, W, H, depth)
    s, N = scene(ugrt, name), W * H
    pr, st = base["primary"], base["stack"]
    args = (pr["normal"], pr["t"], pr["dir"], pr["id"], base["cam"].worldori[:3], s["matidx"], s["mat_list"], s["reflect"],
            s["verts"], s["faces"], depth, st["rays"], st["active"], st["hit_t"], st["hit_id"])
    light = RD.setup_for(ugrt, s).shading_light
    img, ids = RL.shade(base["lcam"].cc, *args, [light], base["is_shadowed"][None, :], st["occluded"].reshape(depth, 1, N), 0, N, N)
    np.testing.assert_array_equal(img, base["image_occluded"])
    np.testing.assert_array_equal(ids, base["mat_ids_occluded"])
    img, ids = RL.shade(base["lcam"].cc, *args, [light], base["is_shadowed"][None, :], None, 0, N, N)
    np.testing.assert_array_equal(img, base["image_depth"])
    np.testing.assert_array_equal(ids, base["mat_ids_depth"])
    assert int((base["image_occluded"] != base["image_depth"]).sum()) > 1000


# measured on the CPU references: rays of level 1 whose occlusion flag differs between two of
# lights_for's three lights, and pixels on which the three-light reflected frame differs from a one-light frame; the
# tests assert half of each
FLAGS_DIFFER = {"hall": {(0, 1): 4147, (0, 2): 5680, (1, 2): 8555}, "crash": {(0, 1): 1225, (0, 2): 2063, (1, 2): 1974}}
IMAGE_DIFFERS = {"hall": [64125, 63731, 64026], "crash": [36298, 36230, 36194]}


@pytest.mark.parametrize("name", ["hall", "crash"])
def test_cpu_frame_tells_the_lights_apart(ugrt, O, REFS, RL, name):
    """Conditions on the CPU references alone, so that the GPU tests below compare something."""
    W, H = SIZES[name]
    want = cpu_frame(O, REFS, RL, ugrt, name, W, H, 2)
    N = W * H
    l1 = want["occluded"][0]
    assert set(np.unique(want["occluded"])) <= {0, 1}
    np.testing.assert_array_equal(l1[0], want["base"]["levels"][0]["occluded"])  # lights_for's first is the scene's own
    for a in range(3):
        for b in range(a + 1, 3):
            diff = int((l1[a] != l1[b]).sum())
            print("%s lights %d and %d: level-1 occlusion flags differ on %d rays" % (name, a, b, diff))
            assert diff >= 1000 and diff >= FLAGS_DIFFER[name][(a, b)] // 2, (name, a, b, diff)
    for l in range(3):
        lt = want["lights"][l]
        one, _ = RL.shade(lt["cc"], *want["shade_args"], [lt["pos"]], lt["flags"][None, :], want["occluded"][:, l:l + 1], 0, N, N)
        changed = int((one.reshape(-1, 3) != want["image"].reshape(-1, 3)).any(1).sum())
        print("%s: %d pixels differ between the three-light and light %d's reflected frame" % (name, changed, l))
        assert changed >= 1000 and changed >= IMAGE_DIFFERS[name][l] // 2, (name, l, changed)
    # the occlusion flags and the reflections both show in the three-light image
    args = (want["lights"][-1]["cc"],) + want["shade_args"] + ([lt["pos"] for lt in want["lights"]],)
    plain, _ = RL.shade(*args, want["flags"], None, 0, N, N)
    assert int((plain != want["image"]).sum()) >= 1000 and (want["image"] <= plain).all()
    flat, _ = RL.shade(*(args[:13] + (np.zeros_like(want["base"]["stack"]["active"]),) + args[14:]), want["flags"], None, 0, N, N)
    assert int((flat != plain).sum()) >= 1000


# ------------------------------------------------------------------------------------------ the synthetic any-hit scene

# target points in and around the box [0, 8] x [0, 8] x [0, 4] of test_reflect_shadows' synthetic scene: above and below
# the layer of the hand-built cells (z = 1..2), inside it, and outside the box
SYN_LIGHTS = [(4.0, 4.0, 3.9), (0.5, 0.5, 0.2), (7.5, 2.0, 0.1), (2.0, 7.0, 5.5), (9.5, 4.0, 1.5), (4.0, -2.0, 2.0),
              (1.5, 1.5, 1.2), (6.0, 6.0, 0.5)]


def syn_light_rays(SYN, light):
    """[6N]: the synthetic rays' origins with the direction light - o, per component in fp32."""
    o = SYN["rays"].reshape(-1, 6)[:, :3]
    return np.concatenate([o, np.float32(light)[None, :] - o], 1).astype(np.float32).reshape(-1)


def syn_actives():
    a = dict(RS.syn_actives())
    a5 = np.zeros(4096, np.int32)
    a5[np.random.RandomState(6).choice(4096, 5, replace=False)] = 1  # fewer rays than any_rays_per_wave's 32
    a["5"] = a5
    return a


def syn_expected(REFS, SYN, lights, active, p0, n, fill=-7):
    return np.stack([REFS[1].trace_any(SYN["grid"], SYN["verts"], SYN["faces"], syn_light_rays(SYN, lt), active, 1.0, p0, n,
                                       4096, fill=fill) for lt in lights])


def rays_through_cell(rays, i, j, k=1, margin=1e-3):
    """Segments o .. o + d (t in [0, 1]) that cross the cell (i, j, k) of the 8 x 8 x 4 grid over the box, shrunk by a
    margin: rays whose walk visits the cell whatever the rounding."""
    r = np.asarray(rays, np.float64).reshape(-1, 6)
    tn, tf = np.zeros(len(r)), np.ones(len(r))
    for ax, c in enumerate((i, j, k)):
        o, d = r[:, ax], r[:, 3 + ax]
        lo, hi = c + margin, c + 1 - margin
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - o) / d, (hi - o) / d
        inside = (o >= lo) & (o <= hi)
        tn = np.maximum(tn, np.where(d == 0, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1)))
        tf = np.minimum(tf, np.where(d == 0, np.inf, np.maximum(t0, t1)))
    return tn <= tf


def test_synthetic_lights_reach_every_list_length(O, REFS, SYN):
    """CPU: under the first three target points (and so under all eight) every hand-built list length is walked under
    at least two lights, and no light's flags are trivial or another's."""
    act = np.ones(4096, np.int32)
    want = syn_expected(REFS, SYN, SYN_LIGHTS, act, 0, 4096)
    for n, (i, j) in RS.SYN_CELLS.items():
        reach = [int(rays_through_cell(syn_light_rays(SYN, lt), i, j).sum()) for lt in SYN_LIGHTS]
        print("list length %d: rays through its cell per light %s" % (n, reach))
        assert sum(1 for c in reach[:3] if c >= 5) >= 2, (n, reach)
    for l in range(8):
        assert 20 < int(want[l].sum()) < 4096 - 100, (l, int(want[l].sum()))  # (the box is mostly empty: 31..181 measured)
        brute = REFS[1].brute_any(SYN["verts"], SYN["faces"], syn_light_rays(SYN, SYN_LIGHTS[l]), act, 1.0, 0, 4096, 4096)
        np.testing.assert_array_equal(want[l], brute)
        for m in range(l):
            assert int((want[l] != want[m]).sum()) > 20, (l, m)


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _walk(ctx, grid, dv, df, d_rays, active, lights, torch, layers=9, sentinel=-7):
    occ = torch.full((layers, 4096), sentinel, dtype=torch.int32, device=ctx.device)
    ctx.trace_dda_any_lights(grid[0], grid[1], grid[2], dv, df, d_rays, ctx.upload(active), lights, occ)
    ctx.synchronize()
    return occ.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [None, (2, 5)])
def test_fused_walk_equals_the_single_calls_and_the_cpu(ugrt, O, REFS, SYN, torch, rows):
    """L = 1, 3, 8 target points over the 4096 synthetic origins; none / all / 67 / 5 rays active; whole frame and a band
    whose p0 is not 0.  The flags equal oc_trace_any per light and L ugrt_trace_dda_any calls on host-made rays; the
    pixels outside the band and a ninth layer keep the sentinel; the rays' last three floats (NaN here) are not read."""
    N = 4096
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN, rows)
    p0, n = ctx.p0, ctx.npix
    assert (p0, n) == ((0, N) if rows is None else (1024, 1536))
    origins = SYN["rays"].reshape(-1, 6).copy()
    origins[:, 3:] = np.nan
    d_origins = ctx.upload(origins.reshape(-1))
    d_light_rays = [ctx.upload(syn_light_rays(SYN, lt)) for lt in SYN_LIGHTS]
    for which, active in syn_actives().items():
        want8 = syn_expected(REFS, SYN, SYN_LIGHTS, active, p0, n)
        for L in (1, 3, 8):
            got = _walk(ctx, grid, dv, df, d_origins, active, SYN_LIGHTS[:L], torch)
            np.testing.assert_array_equal(got[:L], want8[:L], err_msg="%s, %d lights" % (which, L))
            assert (got[L:] == -7).all() and (got[:, :p0] == -7).all() and (got[:, p0 + n:] == -7).all()
            if which == "none":
                assert not got[:L, p0:p0 + n].any()
        single = np.stack([RS._syn_trace(ctx, grid, dv, df, d_light_rays[l], active, 1.0, torch) for l in range(8)])
        np.testing.assert_array_equal(got[:8], single, err_msg=which)
        if which == "all":
            assert all(5 < int(got[l, p0:p0 + n].sum()) < n - 100 for l in range(8)), got[:8, p0:p0 + n].sum(1)


@pytest.mark.gpu
def test_fused_walk_equals_occlusion_rays_and_any_hit_walks_per_light(ugrt, O, REFS, SYN, torch):
    """From hits: the synthetic rays' nearest hits as a reflection level; ugrt_occlusion_rays once (towards the first
    point) + the fused walk == per light ugrt_occlusion_rays + ugrt_trace_dda_any, and == the CPU, at L = 3 and 8."""
    N, OC = 4096, REFS[1]
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    act = np.ones(N, np.int32)
    ht, hid = O.brute_nearest(SYN["verts"], SYN["faces"], SYN["rays"], act, 0, N, N)
    assert int((hid >= 0).sum()) > 1000
    d_rays, d_act, d_ht, d_hid = ctx.upload(SYN["rays"]), ctx.upload(act), ctx.upload(_f32(ht)), ctx.upload(_i32(hid))
    orays = torch.zeros(6 * N, dtype=torch.float32, device=ctx.device)
    oact = torch.zeros(N, dtype=torch.int32, device=ctx.device)
    per_light = []
    for lt in SYN_LIGHTS:
        occ = torch.full((N,), -7, dtype=torch.int32, device=ctx.device)
        ctx.occlusion_rays(d_rays, d_act, d_ht, d_hid, dv, df, lt, EPS, orays, oact)
        ctx.trace_dda_any(grid[0], grid[1], grid[2], dv, df, orays, oact, 1.0, occ)
        per_light.append(occ.cpu().numpy())
        w_rays, w_act = OC.occlusion_rays(SYN["rays"], act, ht, hid, SYN["verts"], SYN["faces"], lt, EPS, 0, N, N)
        np.testing.assert_array_equal(per_light[-1], OC.trace_any(SYN["grid"], SYN["verts"], SYN["faces"], w_rays, w_act, 1.0, 0, N, N))
    ctx.occlusion_rays(d_rays, d_act, d_ht, d_hid, dv, df, SYN_LIGHTS[0], EPS, orays, oact)
    for L in (3, 8):
        occ = torch.full((L, N), -7, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda_any_lights(grid[0], grid[1], grid[2], dv, df, orays, oact, SYN_LIGHTS[:L], occ)
        ctx.synchronize()
        np.testing.assert_array_equal(occ.cpu().numpy(), np.stack(per_light[:L]))
    assert all(50 < int(x.sum()) for x in per_light)


@pytest.mark.gpu
def test_launch_shapes_give_the_same_flags(ugrt, O, REFS, SYN, torch):
    """any_rays_per_wave 1, 7, 32, 64 x any_coop 1, 8, 2^30, and dda_blocks = 1 (every group beyond the first is drawn from
    the ticket), at L = 3."""
    N = 4096
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    d_rays = ctx.upload(SYN["rays"])
    act = np.ones(N, np.int32)
    d_act = ctx.upload(act)
    d_want = ctx.upload(syn_expected(REFS, SYN, SYN_LIGHTS[:3], act, 0, N))

    def check(what):
        occ = torch.full((3, N), -7, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda_any_lights(grid[0], grid[1], grid[2], dv, df, d_rays, d_act, SYN_LIGHTS[:3], occ)
        assert torch.equal(occ, d_want), what

    for rpw in (1, 7, 32, 64):
        for coop in (1, 8, 1 << 30):
            ctx.set_option("any_rays_per_wave", rpw)
            ctx.set_option("any_coop", coop)
            check((rpw, coop))
    ctx.set_option("any_coop", -1)
    ctx.set_option("dda_blocks", 1)
    for rpw in (7, 32):
        ctx.set_option("any_rays_per_wave", rpw)
        check(("dda_blocks 1", rpw))


class Uploaded:
    """A context with a CPU frame's primary arrays and reflection levels on the device as they are, and a camera block
    made current."""

    def __init__(self, ugrt, torch, want, W, H, cc, rows=None):
        s, pr, st = want["scene"], want["base"]["primary"], want["base"]["stack"]
        self.ctx = ctx = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD, rows=rows)
        self.N, self.torch, self.ids = W * H, torch, pr["id"]
        up = lambda a: ctx.upload(np.ascontiguousarray(a).reshape(-1))
        self.normal, self.t, self.dir = up(pr["normal"]), up(pr["t"]), up(pr["dir"])
        self.cam_pos = up(_f32(want["cam_pos"]))
        self.matidx, self.matlist, self.reflect = up(_i32(s["matidx"])), up(_f32(s["mat_list"])), up(_f32(s["reflect"]))
        self.num_materials = len(_f32(s["mat_list"]).reshape(-1)) // 6
        self.verts, self.faces = up(_f32(s["verts"])), up(_i32(s["faces"]))
        self.rays, self.active, self.hit_t, self.hit_id = up(st["rays"]), up(st["active"]), up(st["hit_t"]), up(st["hit_id"])
        ctx.upload_camera(cc)

    def args(self, d_img, d_ids, depth, active=None):
        return [d_img, self.normal, self.t, self.dir, d_ids, self.cam_pos, self.matidx, self.matlist, self.reflect,
                self.num_materials, self.verts, self.faces, depth, self.rays, self.active if active is None else active,
                self.hit_t, self.hit_id]

    def fresh(self, ids=None, img=None):
        t = self.torch
        d_img = t.zeros(3 * self.N, dtype=t.uint8, device=self.ctx.device) if img is None else self.ctx.upload(img)
        return d_img, self.ctx.upload(_i32(self.ids if ids is None else ids))

    def shade(self, depth, light_pos, flags, occluded, ids=None, img=None):
        """(image, ids) on the host after ugrt_shade_reflect_lights and a synchronise."""
        ctx = self.ctx
        d_img, d_ids = self.fresh(ids, img)
        up = lambda a: None if a is None else ctx.upload(_i32(a).reshape(-1))
        ctx.shade_reflect_lights(*self.args(d_img, d_ids, depth), light_pos, up(flags), up(occluded))
        ctx.synchronize()
        return d_img.cpu().numpy(), d_ids.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("name", ["hall", "crash", "mirrors"])
def test_shading_equals_the_cpu_restatement(ugrt, O, REFS, RL, torch, name, depth):
    """L = 1, 2, 3, with and without each flag array."""
    W, H = SIZES[name]
    N = W * H
    want = cpu_frame(O, REFS, RL, ugrt, name, W, H, depth)
    for L in (1, 2, 3):
        lights = want["lights"][:L]
        up = Uploaded(ugrt, torch, want, W, H, lights[-1]["cc"])
        pos = [lt["pos"] for lt in lights]
        for flags in (want["flags"][:L], None):
            for occluded in (np.ascontiguousarray(want["occluded"][:, :L]), None):
                w_img, w_ids = RL.shade(lights[-1]["cc"], *want["shade_args"], pos, flags, occluded, 0, N, N)
                img, ids = up.shade(depth, pos, flags, occluded)
                what = "%d lights, shadow flags %s, occlusion flags %s" % (L, flags is not None, occluded is not None)
                np.testing.assert_array_equal(ids, w_ids, err_msg=what)
                np.testing.assert_array_equal(img, w_img, err_msg=what)
        if L == 3:
            np.testing.assert_array_equal(up.shade(depth, pos, want["flags"], want["occluded"])[0], want["image"])
    assert int((want["image"] != 0).sum()) > 10000


@pytest.mark.gpu
def test_shading_eight_lights_on_a_frame_with_a_tail_block(ugrt, O, REFS, RL, torch):
    """136 x 72 = 9 792 pixels, no multiple of the block: 8 lights at depth 2, random flags of both kinds (values other
    than 0 and 1 among them, of which only 1 darkens), and no flags."""
    W, H = ODD
    N, depth = W * H, 2
    assert N % 256 != 0
    want = cpu_frame(O, REFS, RL, ugrt, "hall", W, H, depth, L=8, nlights=8, shadows=False)
    rng = np.random.RandomState(8)
    values = np.int32([-1, 0, 1, 1, 2, 255, 256 + 1, -2 ** 31])
    flags, occluded = rng.choice(values, (8, N)).astype(np.int32), rng.choice(values, (depth, 8, N)).astype(np.int32)
    up = Uploaded(ugrt, torch, want, W, H, want["lights"][7]["cc"])
    pos = [lt["pos"] for lt in want["lights"]]
    images = {}
    for which, fl, oc in (("flags", flags, occluded), ("none", None, None), ("real", None, want["occluded"])):
        w_img, w_ids = RL.shade(want["lights"][7]["cc"], *want["shade_args"], pos, fl, oc, 0, N, N)
        img, ids = up.shade(depth, pos, fl, oc)
        np.testing.assert_array_equal(ids, w_ids, err_msg=which)
        np.testing.assert_array_equal(img, w_img, err_msg=which)
        images[which] = img
    np.testing.assert_array_equal(images["real"], want["image"])
    assert int((images["flags"] != images["none"]).sum()) > 1000 and int((images["real"] != images["none"]).sum()) > 100
    img, _ = up.shade(depth, pos, (flags == 1).astype(np.int32), (occluded == 1).astype(np.int32))
    np.testing.assert_array_equal(img, images["flags"])


@pytest.mark.gpu
def test_a_band_context_shades_exactly_its_rows(ugrt, O, REFS, RL, torch):
    W, H = SIZES["crash"]
    N, nby, depth = W * H, H // 8, 3
    want = cpu_frame(O, REFS, RL, ugrt, "crash", W, H, depth)
    pos = [lt["pos"] for lt in want["lights"]]
    for rows in ((nby // 2, nby // 2 + 1), (1, nby)):
        p0, n = rows[0] * 8 * W, (rows[1] - rows[0]) * 8 * W
        ids = np.full(N, -77, np.int32)
        ids[p0:p0 + n] = want["base"]["primary"]["id"][p0:p0 + n]
        sentinel = np.full(3 * N, 0xAB, np.uint8)
        up = Uploaded(ugrt, torch, want, W, H, want["lights"][2]["cc"], rows=rows)
        assert (up.ctx.p0, up.ctx.npix) == (p0, n)
        img, got_ids = up.shade(depth, pos, want["flags"], want["occluded"], ids=ids, img=sentinel)
        np.testing.assert_array_equal(img[3 * p0:3 * (p0 + n)], want["image"][3 * p0:3 * (p0 + n)])
        np.testing.assert_array_equal(got_ids[p0:p0 + n], want["mat_ids"][p0:p0 + n])
        outside = np.ones(N, bool)
        outside[p0:p0 + n] = False
        assert (img.reshape(-1, 3)[outside] == 0xAB).all() and (got_ids[outside] == -77).all()
        assert int((img[3 * p0:3 * (p0 + n)] != 0).sum()) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "mirrors"])
def test_one_light_is_the_old_path(ugrt, O, REFS, RL, torch, name):
    """On the GPU, on one context, with a light that is not the scene's own: image and ids of
    ugrt_shade_reflect_depth_occluded + ugrt_shade_add_shadows, of ugrt_shade_reflect_depth with NULL flags; and with
    no active level-1 ray the bytes of ugrt_shade_lights under three lights."""
    W, H = SIZES[name]
    N, depth = W * H, 3
    want = cpu_frame(O, REFS, RL, ugrt, name, W, H, depth)
    lt = want["lights"][1]
    up = Uploaded(ugrt, torch, want, W, H, lt["cc"])
    ctx = up.ctx
    ctx.set_light_position(lt["pos"])
    occ1 = np.ascontiguousarray(want["occluded"][:, 1])
    img, ids = up.shade(depth, [lt["pos"]], lt["flags"], occ1)
    d_img, d_ids = up.fresh()
    ctx.shade_reflect_depth_occluded(*up.args(d_img, d_ids, depth), ctx.upload(occ1.reshape(-1)))
    ctx.shade_add_shadows(d_img, ctx.upload(lt["flags"]))
    ctx.synchronize()
    np.testing.assert_array_equal(img, d_img.cpu().numpy())
    np.testing.assert_array_equal(ids, d_ids.cpu().numpy())
    assert int((img != 0).sum()) > 10000
    img, ids = up.shade(depth, [lt["pos"]], None, None)
    d_img, d_ids = up.fresh()
    ctx.shade_reflect_depth(*up.args(d_img, d_ids, depth))
    ctx.synchronize()
    np.testing.assert_array_equal(img, d_img.cpu().numpy())
    np.testing.assert_array_equal(ids, d_ids.cpu().numpy())
    # no reflection at all: the lights' shading of section 6.3
    pos = [x["pos"] for x in want["lights"]]
    d_flags = ctx.upload(want["flags"].reshape(-1))
    none_active = torch.zeros_like(up.active)
    d_img, d_ids = up.fresh()
    ctx.shade_reflect_lights(*up.args(d_img, d_ids, depth, active=none_active), pos, d_flags,
                             ctx.upload(want["occluded"].reshape(-1)))
    l_img, l_ids = up.fresh()
    ctx.shade_lights(l_img, up.normal, up.t, up.dir, l_ids, up.cam_pos, up.matidx, up.matlist, up.num_materials, pos, d_flags)
    ctx.synchronize()
    assert torch.equal(d_img, l_img) and torch.equal(d_ids, l_ids)
    assert int((d_img != 0).sum()) > 10000


def assert_lights_frame(r, want, depth, L):
    a, b = want["p0"], want["p0"] + want["n"]
    for j, w in enumerate(want["base"]["levels"][:depth]):
        what = "level %d" % (j + 1)
        np.testing.assert_array_equal(r.active_levels[j].cpu().numpy()[a:b], w["active"][a:b], err_msg=what)
        np.testing.assert_array_equal(bits(r.rays_levels[j].cpu().numpy()[6 * a:6 * b]), bits(w["rays"][6 * a:6 * b]), err_msg=what)
        np.testing.assert_array_equal(r.hit_id_levels[j].cpu().numpy()[a:b], w["hit_id"][a:b], err_msg=what)
        np.testing.assert_array_equal(bits(r.hit_t_levels[j].cpu().numpy()[a:b]), bits(w["hit_t"][a:b]), err_msg=what)
    assert tuple(r.occluded_lights.shape) == (depth, L, want["N"]) and r.occluded_lights.is_contiguous()
    np.testing.assert_array_equal(r.occluded_lights.cpu().numpy(), want["occluded"])
    np.testing.assert_array_equal(r.shadowed_lights[:L].cpu().numpy(), want["flags"])
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy()[a:b], want["mat_ids"][a:b])
    np.testing.assert_array_equal(r.image.cpu().numpy()[3 * a:3 * b], want["image"][3 * a:3 * b])


KW = dict(shadows=True, reflect=True, reflect_shadows=True, reflect_lights=True)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 4])
@pytest.mark.parametrize("name", ["hall", "crash", "mirrors"])
def test_frame_equals_the_cpu_frame(ugrt, O, REFS, RL, torch, name, depth):
    """Three lights; then, on the same renderer, the scene's own light alone: byte for byte the single-light frame of
    section 6.2 on a renderer of its own (image, ids, occluded_lights[:, 0] against occluded_levels)."""
    s = scene(ugrt, name)
    W, H = SIZES[name]
    want = cpu_frame(O, REFS, RL, ugrt, name, W, H, depth)
    lights = [(lt["params"], lt["pos"]) for lt in want["lights"]]
    ctx, r = RD.make(ugrt, s, W, H)
    r.display(TL.setup_for(ugrt, s, lights), bounces=depth, **KW)
    ctx.synchronize()
    assert_lights_frame(r, want, depth, 3)
    r.display(TL.setup_for(ugrt, s, lights[:1]), bounces=depth, **KW)
    ctx.synchronize()
    ctx1, r1 = RD.make(ugrt, s, W, H)
    r1.display(RD.setup_for(ugrt, s), shadows=True, reflect=True, bounces=depth, reflect_shadows=True)
    ctx1.synchronize()
    assert tuple(r.occluded_lights.shape) == (depth, 1, W * H)
    assert torch.equal(r.image, r1.image) and torch.equal(r.intersect_id, r1.intersect_id)
    assert torch.equal(r.occluded_lights[:, 0], r1.occluded_levels[:depth])
    assert torch.equal(r.shadowed_lights[0], r1.is_shadowed)
    RS.assert_occluded_frame(r1, want["base"], depth)


@pytest.mark.gpu
def test_frame_without_shadows_of_either_kind(ugrt, O, REFS, RL, torch):
    """shadows=False and / or reflect_shadows=False pass NULL for the flag arrays: the CPU frame without them."""
    name, depth = "hall", 2
    s = scene(ugrt, name)
    W, H = SIZES[name]
    N = W * H
    want = cpu_frame(O, REFS, RL, ugrt, name, W, H, depth)
    lights = [(lt["params"], lt["pos"]) for lt in want["lights"]]
    pos = [lt["pos"] for lt in want["lights"]]
    ctx, r = RD.make(ugrt, s, W, H)
    for shadows, rs in ((False, True), (True, False), (False, False)):
        r.display(TL.setup_for(ugrt, s, lights), bounces=depth, shadows=shadows, reflect=True, reflect_shadows=rs,
                  reflect_lights=True)
        ctx.synchronize()
        w_img, w_ids = RL.shade(want["lights"][-1]["cc"], *want["shade_args"], pos, want["flags"] if shadows else None,
                                want["occluded"] if rs else None, 0, N, N)
        np.testing.assert_array_equal(r.image.cpu().numpy(), w_img, err_msg="shadows %s, reflect_shadows %s" % (shadows, rs))
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids)


FRAME_ARRAYS = ("image", "intersect_id", "is_shadowed", "rays_levels", "active_levels", "hit_t_levels", "hit_id_levels")


@pytest.mark.gpu
def test_a_plain_reflect_frame_behind_a_lights_frame_is_the_plain_frame(ugrt, O, REFS, RL, torch):
    """The split-walk history and the turn of the ray counters are undisturbed: two plain frames on a renderer that has
    rendered with reflect_lights equal those of a renderer that never has, byte for byte, and the CPU frame."""
    name, depth = "mirrors", 3
    s = scene(ugrt, name)
    W, H = SIZES[name]
    want = cpu_frame(O, REFS, RL, ugrt, name, W, H, depth)
    lights = [(lt["params"], lt["pos"]) for lt in want["lights"]]
    plain = dict(shadows=True, reflect=True, bounces=depth, reflect_shadows=True)
    ctx_a, a = RD.make(ugrt, s, W, H)
    ctx_b, b = RD.make(ugrt, s, W, H)
    for _ in range(2):
        a.display(RD.setup_for(ugrt, s), **plain)
    b.display(TL.setup_for(ugrt, s, lights), bounces=depth, **KW)
    ctx_b.synchronize()
    assert_lights_frame(b, want, depth, 3)
    assert not torch.equal(a.image, b.image)
    for _ in range(2):
        b.display(RD.setup_for(ugrt, s), **plain)
    ctx_a.synchronize()
    ctx_b.synchronize()
    for n in FRAME_ARRAYS + ("occluded_levels",):
        x, y = getattr(a, n), getattr(b, n)
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), n
    RS.assert_occluded_frame(b, want["base"], depth)
    b.display(TL.setup_for(ugrt, s, lights), bounces=depth, **KW)
    ctx_b.synchronize()
    assert_lights_frame(b, want, depth, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("async_build", [1, 0])
def test_four_renderers_in_flight_equal_a_sequential_context(ugrt, torch, async_build):
    """As tests/test_reflect_shadows.py's test of the same name, with one-stream renderers (the frame's only path) on
    streams of their own."""
    s = scene(ugrt, "crash")
    W, H = 384, 216
    setup = TL.setup_for(ugrt, s, TL.lights_for(s, 3))
    kw = dict(bounces=3, **KW)
    seq_ctx, seq = RD.make(ugrt, s, W, H)
    seq.display(setup, **kw)
    seq_ctx.synchronize()
    renderers = []
    for i in range(4):
        stream = torch.cuda.Stream() if i else None
        with torch.cuda.stream(stream):
            cx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
            rr = ugrt.Renderer(cx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
        cx.set_option("async_build", async_build)
        rr._stream = stream
        renderers.append(rr)
    for k in range(8):
        rr = renderers[k % 4]
        with torch.cuda.stream(rr._stream):
            rr.display(setup, **kw)
    for i, rr in enumerate(renderers):
        # the light grid changes from light to light, and an asynchronous build or shadow pass is sized by the one before
        # plus a quarter: a light that needs more is reported (UGRT_EOVERFLOW) and the frame is to be repeated.  ONE repeat
        # repairs it: up to the next synchronisation every pass of every light waits (include/ugrt.h, option "async_build")
        try:
            rr.synchronize()
        except ugrt.UgrtError as e:
            assert async_build and e.code == 6, e
            print("renderer %d: UGRT_EOVERFLOW, frame repeated" % i)
            with torch.cuda.stream(rr._stream):
                rr.display(setup, **kw)
            rr.synchronize()
    torch.cuda.synchronize()
    for i, rr in enumerate(renderers):
        for n in FRAME_ARRAYS + ("occluded_lights", "shadowed_lights"):
            x, y = getattr(rr, n), getattr(seq, n)
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (i, n)
    assert int(seq.occluded_lights[0, 1].sum()) > 1000 and int(seq.occluded_lights[2].sum()) > 0
    assert not torch.equal(seq.occluded_lights[0, 0], seq.occluded_lights[0, 1])


@pytest.mark.gpu
def test_every_pass_of_a_repeat_waits_until_the_next_synchronisation(ugrt, torch):
    """Option "async_build" behind UGRT_EOVERFLOW: a frame with several lights builds the light grid and traces shadows
    once per light, each pass sized by the one before it, so the repeat has passes of unequal need one behind the other.
    Here that is two scenes on one context, with a known order: crash at scale 0.08 outgrows every estimate that
    scale 0.02 leaves (tests/test_gpu_parity.py::test_async_builds_equal_the_waiting_form).  The repeat renders the small
    scene and then the large one before it synchronises: both must run in the waiting form, the second too, and the
    large frame equals that of a context which never built asynchronously."""
    small, big = scene(ugrt, "crash"), ugrt.scenes.crash(scale=0.08)
    W, H = SIZES["crash"]
    plain = dict(shadows=True, reflect=True, bounces=2, reflect_shadows=True)
    ctx, ra = RD.make(ugrt, small, W, H)
    ctx.set_option("async_build", 1)
    rb = ugrt.Renderer(ctx, big["verts"], big["faces"], big["matidx"], big["mat_list"], big["reflect"])
    for _ in range(2):  # the first frame waits (no estimate yet), the second does not
        ra.display(RD.setup_for(ugrt, small), **plain)
    ctx.synchronize()
    rb.display(RD.setup_for(ugrt, big), **plain)
    with pytest.raises(ugrt.UgrtError, match="asynchronous") as e:
        ctx.synchronize()
    assert e.value.code == ugrt.UGRT_EOVERFLOW
    ra.display(RD.setup_for(ugrt, small), **plain)
    rb.display(RD.setup_for(ugrt, big), **plain)
    ctx.synchronize()  # (raised again when only the first pass behind the report waited)
    wctx, wr = RD.make(ugrt, big, W, H)
    wr.display(RD.setup_for(ugrt, big), **plain)
    wctx.synchronize()
    for n in FRAME_ARRAYS + ("occluded_levels",):
        x, y = getattr(rb, n), getattr(wr, n)
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), n
    # behind the synchronisation the estimates count again: a third frame of the large scene does not wait and fits
    rb.display(RD.setup_for(ugrt, big), **plain)
    ctx.synchronize()
    assert torch.equal(rb.image, wr.image)


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, REFS, RL, torch):
    name, depth = "hall", 2
    s = scene(ugrt, name)
    W, H = SIZES[name]
    N = W * H
    want = cpu_frame(O, REFS, RL, ugrt, name, W, H, depth)
    lights = [(lt["params"], lt["pos"]) for lt in want["lights"]]
    pos = [lt["pos"] for lt in want["lights"]]
    fresh = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD)
    z = torch.zeros(6 * N, dtype=torch.int32, device=fresh.device)
    with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
        fresh.trace_dda_any_lights(z, z, z, z, z, z, z, pos, z)
    assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    ctx, r = RD.make(ugrt, s, W, H)
    setup = TL.setup_for(ugrt, s, lights)
    r.display(setup, bounces=depth, **KW)
    ctx.synchronize()
    g = ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3]
    occ = torch.full((3, N), -7, dtype=torch.int32, device=ctx.device)
    sentinel = torch.full_like(r.image, 0xAB)
    img, ids = sentinel.clone(), r.intersect_id.clone()
    walk_args = [g[0], g[1], g[2], r.d_verts, r.d_faces, r.occlusion_rays, r.occlusion_active, pos, occ]
    shade_args = [img, r.normal, r.t, r.dir, ids, r.cam_pos, r.d_matidx, r.d_matlist, r.d_reflect, r.num_materials, r.d_verts,
                  r.d_faces, depth, r.rays_levels, r.active_levels, r.hit_t_levels, r.hit_id_levels, pos, r.shadowed_lights,
                  r.occluded_lights]
    eight = [lt[1] for lt in TL.lights_for(s, 8)]
    for fn, args, where in ((ctx.trace_dda_any_lights, walk_args, 7), (ctx.shade_reflect_lights, shade_args, 17)):
        for bad in ([], eight + eight[:1]):
            with pytest.raises(ugrt.UgrtError) as e:
                fn(*(args[:where] + [bad] + args[where + 1:]))
            assert e.value.code == ugrt.UGRT_EINVAL and b"num_lights" in ugrt.lib.ugrt_last_error()
        holes = range(len(args) - 1) if fn == ctx.trace_dda_any_lights else [h for h in range(18) if h not in (9, 12)]
        for h in list(holes) + ([8] if where == 7 else []):
            holed = list(args)
            holed[h] = None
            with pytest.raises(ugrt.UgrtError) as e:
                fn(*holed)
            assert e.value.code == ugrt.UGRT_EINVAL and b"null" in ugrt.lib.ugrt_last_error(), h
    for bad_depth in (0, 9):
        with pytest.raises(ugrt.UgrtError) as e:
            ctx.shade_reflect_lights(*(shade_args[:12] + [bad_depth] + shade_args[13:]))
        assert e.value.code == ugrt.UGRT_EINVAL and b"depth" in ugrt.lib.ugrt_last_error()
    ctx.synchronize()
    assert torch.equal(img, sentinel) and torch.equal(ids, r.intersect_id) and bool((occ == -7).all())
    for kw in (dict(reflect=True), dict(reflect=False, reflect_lights=True), dict(reflect=True, reflect_lights=1)):
        r.image.copy_(sentinel)
        with pytest.raises(ValueError):
            r.display(setup, **kw)
        ctx.synchronize()
        assert torch.equal(r.image, sentinel)
    with pytest.raises(ValueError):
        r.display(RD.setup_for(ugrt, s), reflect=True, reflect_lights=True)
    for kw in (dict(overlap=True), dict(overlap=True, helper_thread=False)):
        _, two = RD.make(ugrt, s, W, H, **kw)
        with pytest.raises(ValueError):
            two.display(setup, bounces=depth, **KW)
        two.close()
    r.display(setup, bounces=depth, **KW)  # the context is still usable
    ctx.synchronize()
    assert_lights_frame(r, want, depth, 3)
