"""The host path of the passes over a band's pixels: the twelve ugrt_shade_* exports and ugrt_map_rays_to_light.

What every one of them owes its caller, whatever its kernel computes: one bracket of its profiler stage per call and
none with profiling off; exactly the context's rows written, with the bytes and ids a context over the whole image
writes there; its argument checks before anything reaches the device, with its own name in the message.  What the
kernels compute is pinned against the CPU restatements elsewhere (test_gpu_parity, test_lights, test_reflect_depth,
test_reflect_shadows, test_reflect_lights, test_ambient, test_area_light, test_area_sets); here a band is compared with
the full frame of the same library, which is exact because no pass reads a neighbouring pixel.

The scene is test_reference_kernels' soup1 at 128 x 96 (twelve tile rows; hits and misses).  Its four materials are the
Cornell box's, none of which reflects, so the renderer is given reflect values of its own.  One frame under two lights
with reflect=True, bounces=2, reflect_shadows=True fills the input arrays; levels and lights beyond the frame's two are
its arrays repeated, which serves: the passes are compared with themselves."""
import math

import numpy as np
import pytest

import test_reference_kernels as RK

CASE = "soup1_128x96"
REFLECT = (0.5, 0.0, 0.3, 0.8)
UD = (16, 16, 8)
BYTE, ID = 0xA5, -7  # the sentinels
BANDS = ((4, 9), (5, 6))  # tile rows 4..8 of 12; one tile row: 1024 pixels, exactly four blocks


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Frame:
    """The inputs of every pass on the device, and what a context needs to stand where the frame's context stood."""


def _context(ugrt, F, rows=None):
    ctx = ugrt.Context(F.W, F.H, light_grid=(F.W // 8, F.H // 8), flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD,
                       rows=rows)
    ctx.set_light_position(F.light)
    ctx.upload_camera(F.camcoords)
    return ctx


@pytest.fixture(scope="module")
def FRAME(ugrt, torch):
    build, W, H = RK.CASES[CASE]
    s, setup = build(ugrt)
    D, L = ugrt.MAX_REFLECT_DEPTH, ugrt.MAX_LIGHTS
    rng = np.random.default_rng(12)
    eye = np.asarray(setup.light_camera["eye"], np.float64)
    second = dict(setup.light_camera, eye=tuple(eye + (40.0, -25.0, 30.0)))
    lights = [(setup.light_camera, setup.shading_light), (second, tuple(rng.uniform(100.0, 450.0, 3)))]
    ctx = ugrt.Context(W, H, light_grid=(W // 8, H // 8), flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], np.float32(REFLECT))
    # the ids are triangle ids until the frame's shading call rewrites them: keep what it was given
    seen, shade = {}, ctx.shade_reflect_lights

    def keep_ids(img, normal, t, ray_dir, ids, *rest):
        seen["tri"] = ids.clone()
        shade(img, normal, t, ray_dir, ids, *rest)

    ctx.shade_reflect_lights = keep_ids
    r.display(ugrt.FrameSetup(setup.camera, setup.light_camera, setup.shading_light, lights=lights), shadows=True,
              reflect=True, bounces=2, reflect_shadows=True, reflect_lights=True)
    del ctx.shade_reflect_lights
    ctx.synchronize()
    F = Frame()
    F.W, F.H, F.N, F.setup, F.scene = W, H, W * H, setup, s
    N = F.N
    F.light = setup.shading_light
    F.camcoords = ugrt.renderer.make_camera(setup.light_camera, setup.fovy, r.aspect).camcoords
    F.normal, F.t, F.dir, F.tri, F.cam_pos = r.normal, r.t, r.dir, seen["tri"], r.cam_pos
    F.matidx, F.matlist, F.reflect, F.nm, F.verts, F.faces = r.d_matidx, r.d_matlist, r.d_reflect, r.num_materials, r.d_verts, r.d_faces
    rep = lambda a, *k: a.repeat(*k).contiguous()
    F.rays, F.active = rep(r.rays_levels[:2], D // 2, 1).reshape(-1), rep(r.active_levels[:2], D // 2, 1).reshape(-1)
    F.hit_t, F.hit_id = rep(r.hit_t_levels[:2], D // 2, 1).reshape(-1), rep(r.hit_id_levels[:2], D // 2, 1).reshape(-1)
    F.shadowed = rep(r.shadowed_lights[:2], L // 2, 1)  # [L, N]
    F.occluded = rep(r.occluded_lights[:2, :2], D // 2, L // 2, 1)  # [D, L, N]
    F.lights = [pos for _, pos in lights] + [tuple(rng.uniform(100.0, 450.0, 3)) for _ in range(L - 2)]
    # mask words with bits above any low-bit window; a quarter of them zero inside the one-bit window, a quarter zero
    mask = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    mask &= rng.choice(np.uint32([0xFFFFFFFF, 0xFFFFFFFE, 0xFFFF0001, 0]), N)
    F.mask = ctx.upload(mask.view(np.int32))
    den = rng.integers(0, 60, N) * (rng.random(N) < 0.8)
    F.vis = ctx.upload(np.stack([rng.integers(0, den + 1), den], 1).astype(np.uint32).reshape(-1).view(np.int32))
    tri, act = F.tri.cpu().numpy(), r.active_levels[:2].cpu().numpy()
    assert int((tri >= 0).sum()) > 1000 and int((tri < 0).sum()) > 100, "hits and misses"
    assert int(act[0].sum()) > 500 and int(act[1].sum()) > 50, "both reflection levels have rays"
    assert 0 < int(F.shadowed[:2].sum()) and 0 < int(F.occluded[:2, :2].sum())
    assert int((mask >> 1).astype(bool).sum()) > N // 2 and int((mask & 1 == 0).sum()) > N // 4
    F.renderer, F.ctx, F.lights2 = r, ctx, lights
    return F


class Out:
    """A call's own outputs, prefilled with the sentinels; the ids hold the triangle ids on the context's rows."""

    def __init__(self, ctx, F, torch):
        full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=ctx.device)
        self.img, self.ids = full(3 * F.N, BYTE, torch.uint8), full(F.N, ID, torch.int32)
        self.ids[ctx.p0:ctx.p0 + ctx.npix] = F.tri[ctx.p0:ctx.p0 + ctx.npix]
        self.dump, self.map = full(2 * F.N, 7.0, torch.float32), full(2 * F.N, ID, torch.int32)


def _primary(F, o):
    return [o.img, F.normal, F.t, F.dir, o.ids, F.cam_pos, F.matidx, F.matlist]


def _levels(F):
    return [F.rays, F.active, F.hit_t, F.hit_id]


def _reflect_lights(F, o, v):
    depth, L = v
    return _primary(F, o) + [F.reflect, F.nm, F.verts, F.faces, depth] + _levels(F) + [
        F.lights[:L], F.shadowed[:L], F.occluded[:, :L].contiguous()]


# name -> (stage, variants, arguments of Context.<name> for (frame, outputs, variant), positions that may be None,
# per-pixel outputs as (attribute of Out, values per pixel))
IMG, IDS = ("img", 3), ("ids", 1)
EXPORTS = {
    "shade_simple": ("shade", [None], lambda F, o, v: _primary(F, o) + [F.nm], (), (IMG, IDS)),
    "shade_spotlight": ("shade", [None], lambda F, o, v: _primary(F, o) + [F.nm, o.dump], (9,), (IMG, IDS, ("dump", 2))),
    "shade_add_shadows": ("shade", [None], lambda F, o, v: [o.img, F.shadowed[0]], (), (IMG,)),
    "shade_ao": ("shade", [1, 32], lambda F, o, v: [o.img, F.mask, v], (), (IMG,)),
    "shade_area": ("shade", [1, 32], lambda F, o, v: [o.img, F.mask, v], (), (IMG,)),
    "shade_area_vis": ("shade", [1, 32], lambda F, o, v: [o.img, F.vis, v], (), (IMG,)),
    "shade_lights": ("shade", [1, 8], lambda F, o, v: _primary(F, o) + [F.nm, F.lights[:v], F.shadowed[:v]], (10,),
                     (IMG, IDS)),
    "shade_perlin": ("shade", [None], lambda F, o, v: [o.img, F.t, F.dir, F.cam_pos, o.ids], (1, 2, 3), (IMG,)),
    "shade_reflect": ("shade", [None], lambda F, o, v: _primary(F, o) + [F.reflect, F.nm, F.verts, F.faces] + _levels(F),
                      (), (IMG, IDS)),
    "shade_reflect_depth": ("shade", [1, 8], lambda F, o, v: _primary(F, o) + [F.reflect, F.nm, F.verts, F.faces, v] +
                            _levels(F), (), (IMG, IDS)),
    "shade_reflect_depth_occluded": ("shade", [1, 8], lambda F, o, v: _primary(F, o) + [F.reflect, F.nm, F.verts, F.faces, v] +
                                     _levels(F) + [F.occluded[:, 0].contiguous()], (), (IMG, IDS)),
    "shade_reflect_lights": ("shade", [(1, 1), (8, 8), (1, 8), (8, 1)], _reflect_lights, (18, 19), (IMG, IDS)),
    "map_rays_to_light": ("map_rays", [None], lambda F, o, v: [F.t, F.dir, o.map, F.cam_pos, math.pi, math.pi], (), ()),
}
NAMES = sorted(EXPORTS)


def test_the_table_names_every_pass(ugrt):
    """CPU: the twelve ugrt_shade_* prototypes and ugrt_map_rays_to_light, and nothing else, are the table's rows."""
    assert ugrt.MAX_REFLECT_DEPTH == 8 and ugrt.MAX_LIGHTS == 8 and ugrt.MAX_AO_DIRS == 32 and ugrt.MAX_AREA_SAMPLES == 32
    shade = {n[len("ugrt_"):] for n in ugrt.PROTOTYPES if n.startswith("ugrt_shade_")}
    assert shade | {"map_rays_to_light"} == set(EXPORTS) and len(shade) == 12
    for name in EXPORTS:
        assert hasattr(ugrt.Context, name), name


@pytest.fixture(scope="module")
def CONTEXTS(ugrt, FRAME):
    """A context over the whole image and one per band of BANDS, in the frame's camera and light."""
    return [_context(ugrt, FRAME)] + [_context(ugrt, FRAME, rows=rows) for rows in BANDS]


def _run(ctx, F, torch, name, v):
    o = Out(ctx, F, torch)
    getattr(ctx, name)(*EXPORTS[name][2](F, o, v))
    return o


@pytest.mark.gpu
def test_one_bracket_of_its_stage_per_call(ugrt, FRAME, torch):
    """With the profiler on a call adds exactly one launch to its stage (`shade`; `map_rays` for map_rays_to_light) and
    none to any other; with it off prof_get() does not move."""
    F = FRAME
    ctx = _context(ugrt, F)
    counts = lambda: {k: v[1] for k, v in ctx.prof_get().items()}
    ctx.prof_enable(True)
    ctx.prof_reset()
    assert set(counts().values()) == {0}
    for name in NAMES:
        stage, variants = EXPORTS[name][:2]
        for v in variants:
            before = counts()
            _run(ctx, F, torch, name, v)
            assert counts() == dict(before, **{stage: before[stage] + 1}), (name, v)
    ctx.synchronize()
    ctx.prof_enable(False)
    before = ctx.prof_get()
    for name in NAMES:
        for v in EXPORTS[name][1]:
            _run(ctx, F, torch, name, v)
    ctx.synchronize()
    assert ctx.prof_get() == before


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_a_band_writes_its_rows_and_nothing_else(ugrt, FRAME, CONTEXTS, torch, name):
    """Every variant (1 and the most lights, depth 1 and the deepest, 1 and 32 mask bits) on the whole image, on tile rows
    4..8 of 12 and on one tile row, into arrays full of sentinels: outside the rows the sentinels stay (image, ids, the
    spot light's dump), inside them the values are the whole image's.  The ray map is indexed by the band's own pixels:
    [0, n) the pixel ids, [n, 2n) the light cells, which are the whole image's on those rows."""
    F, N = FRAME, FRAME.N
    outputs = EXPORTS[name][4]
    contexts = CONTEXTS
    assert [(c.p0, c.npix) for c in contexts] == [(0, N), (4 * 1024, 5 * 1024), (5 * 1024, 1024)]
    for v in EXPORTS[name][1]:
        runs = [_run(c, F, torch, name, v) for c in contexts]
        for c in contexts:
            c.synchronize()
        full = runs[0]
        for c, o in zip(contexts[1:], runs[1:]):
            a, b = c.p0, c.p0 + c.npix
            for attr, k in outputs:
                got, want = getattr(o, attr).cpu().numpy(), getattr(full, attr).cpu().numpy()
                np.testing.assert_array_equal(got[k * a:k * b], want[k * a:k * b], err_msg="%s %s %s" % (name, v, attr))
                sentinel = np.float32(7.0) if attr == "dump" else (BYTE if attr == "img" else ID)
                assert (got[:k * a] == sentinel).all() and (got[k * b:] == sentinel).all(), (name, v, attr)
            if name == "map_rays_to_light":
                got, want = o.map.cpu().numpy(), full.map.cpu().numpy()
                np.testing.assert_array_equal(got[:c.npix], np.arange(a, b))
                np.testing.assert_array_equal(got[c.npix:2 * c.npix], want[N + a:N + b])
                assert (got[2 * c.npix:] == ID).all()
        # the whole image: nothing of a sentinel is left where the pass writes every pixel, and the pass did something
        img, ids = full.img.cpu().numpy(), full.ids.cpu().numpy()
        if IDS in outputs:
            assert (ids != ID).all() and ((ids >= 0) == (F.tri.cpu().numpy() >= 0)).all(), (name, v)
        if IMG in outputs:  # (the passes that scale the image in place change the pixels their flags or masks name)
            assert int((img != BYTE).sum()) > (1000 if IDS in outputs or name == "shade_perlin" else 0), (name, v)
        if name == "map_rays_to_light":
            m = full.map.cpu().numpy()
            np.testing.assert_array_equal(m[:N], np.arange(N))
            assert m[N:].min() >= 0 and m[N:].max() <= (F.W // 8) * (F.H // 8) and len(np.unique(m[N:])) > 4


@pytest.mark.gpu
def test_a_null_argument_is_refused_by_name_and_the_context_goes_on(ugrt, FRAME, torch):
    """None in each pointer position that the call does not allow to be null: UGRT_EINVAL, the message begins with the
    export's own name; a position that may be null is accepted.  The context that refused all of them then renders the
    frame again, to the same bytes."""
    F = FRAME
    ctx, r = F.ctx, F.renderer
    want_img, want_ids = r.image.clone(), r.intersect_id.clone()
    for name in NAMES:
        _, variants, args_of, may_be_null, outputs = EXPORTS[name]
        o = Out(ctx, F, torch)
        args = args_of(F, o, variants[-1])
        pointers = [i for i, a in enumerate(args) if isinstance(a, (torch.Tensor, list))]
        assert len(pointers) >= 2, name
        for i in pointers:
            bad = list(args)
            bad[i] = None
            if i in may_be_null:
                getattr(ctx, name)(*bad)
                continue
            with pytest.raises(ugrt.UgrtError) as e:
                getattr(ctx, name)(*bad)
            assert e.value.code == ugrt.UGRT_EINVAL, (name, i)
            assert str(e.value).split(": ", 1)[1].startswith(name + ": "), (name, i, str(e.value))
        ctx.synchronize()
    setup = F.setup
    r.display(ugrt.FrameSetup(setup.camera, setup.light_camera, setup.shading_light, lights=F.lights2), shadows=True,
              reflect=True, bounces=2, reflect_shadows=True, reflect_lights=True)
    ctx.synchronize()
    assert torch.equal(r.image, want_img) and torch.equal(r.intersect_id, want_ids)
    assert int((want_img != 0).sum()) > 1000
