"""Area lights: ugrt_trace_dda_any_area, ugrt_trace_dda_any_area_thru, ugrt_shade_area,
scenes.area_samples and Renderer.display(..., area=S, area_radius=r).

The checker is tests/area_ref.c (built here with the oracle's flags): the explicit ray set of one sample and the integer
shading, restated on the CPU.  The any-hit walk has no restatement of its own: the expected mask is oc_trace_any of
tests/occlusion_ref.c on the explicit rays at t_max = 1, once per sample, OR-ed into bit s; for the see-through form the
same on test_refract.filtered_grid.  The origins are those of tests/ambient_ref.c's ao_rays; the frames underneath come
from the CPU frames of tests/test_lights.py, tests/test_reflect_shadows.py and tests/test_refract.py."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import test_ambient as AM
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
import test_refract as RFR
from test_ambient import AO  # noqa: F401  (fixtures)
from test_reflect_shadows import REFS, SYN  # noqa: F401
from test_refract import RF  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))

_p, _f32, _i32, bits, scene, SIZES, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.scene, RD.SIZES, RD.LG, RD.UD
CALLS = ("ugrt_trace_dda_any_area", "ugrt_trace_dda_any_area_thru", "ugrt_shade_area")
EPS = 1e-3
S_FRAME = 16  # samples per pixel in the frame tests
DEPTH = 3     # of the reflecting frames


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def low_bits(S):
    return np.uint32(0xFFFFFFFF) if S == 32 else np.uint32((1 << S) - 1)


class AreaRef:
    def __init__(self, lib):
        self.lib = lib

    def expand(self, orays, oactive, pos, p0, n, N):
        """[6N] explicit rays {o, pos - o} towards one point."""
        rays = np.zeros(6 * N, np.float32)
        self.lib.area_expand(_p(_f32(orays)), _p(_i32(oactive)), _p(_f32(pos)), C.c_int(p0), C.c_int(n), _p(rays))
        return rays

    def shade(self, img, mask, num_samples, p0, n):
        img = np.ascontiguousarray(img, np.uint8).copy()
        self.lib.area_shade(_p(img), _p(_u32(mask)), C.c_int(num_samples), C.c_int(p0), C.c_int(n))
        return img


@pytest.fixture(scope="session")
def AR(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("area_ref") / "libarea_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "area_ref.c"), "-lm"], check=True, capture_output=True)
    return AreaRef(C.CDLL(out))


def cpu_mask(OC, AR, grid, verts, faces, orays, oactive, samples, p0, n, N, fill=0, keep=None):
    """The expected mask words: per sample s the explicit rays of area_expand walked by oc_trace_any at t_max = 1, its
    flags OR-ed into bit s.  Pixels outside the band keep `fill`.  keep: a list that receives the explicit rays of
    every sample."""
    mask = np.full(N, fill, np.uint32)
    mask[p0:p0 + n] = 0
    for s, pos in enumerate(np.asarray(samples, np.float32).reshape(-1, 3)):
        rays = AR.expand(orays, oactive, pos, p0, n, N)
        occ = OC.trace_any(grid, verts, faces, rays, oactive, 1.0, p0, n, N)
        assert set(np.unique(occ[p0:p0 + n])) <= {0, 1}
        mask[p0:p0 + n] |= occ[p0:p0 + n].astype(np.uint32) << np.uint32(s)
        if keep is not None:
            keep.append(rays)
    return mask


def mask_counts(mask, oactive, S):
    hit = oactive != 0
    m = mask[hit]
    full = low_bits(S)
    return dict(lit=int((m == 0).sum()), umbra=int((m == full).sum()), penumbra=int(((m != 0) & (m != full)).sum()),
                per_bit=[int(((m >> np.uint32(s)) & 1).sum()) for s in range(S)])


def light_disk(ugrt, s, S, radius):
    """The samples of the frame's light: the disk around the light camera's eye, perpendicular to look - eye."""
    lc = ugrt.FrameSetup.from_scene(s).light_camera
    eye = np.asarray(lc["eye"], np.float64)
    return ugrt.scenes.area_samples(S, eye, np.asarray(lc["look"], np.float64) - eye, radius)


def extent(s):
    v = _f32(s["verts"]).reshape(-1, 3)
    return float((v.max(0) - v.min(0)).max())


_AREA = {}


def cpu_area(O, REFS, AO, AR, ugrt, name, RF=None):
    """The CPU side of a frame's area light at S_FRAME samples: the origins of the primary hits, the samples, the
    explicit rays per sample and the mask.  hall and crash (the frame of test_reflect_shadows): the radius is 10 % of
    the scene's largest extent; glass (the frame of test_refract): 3 %, with the plain mask ("plain") and the
    see-through one ("mask").  Computed once per scene and shared: nobody writes to it."""
    if name in _AREA:
        return _AREA[name]
    OC = REFS[1]
    if name == "glass":
        s = RFR.scene(ugrt, "glass")
        W, H = RFR.W, RFR.H
        base = RFR.cpu_frame(O, RF, REFS, ugrt, "glass", DEPTH)
        share = 0.03
    else:
        s = scene(ugrt, name)
        W, H = SIZES[name]
        base = RS.cpu_frame(O, REFS, ugrt, name, W, H, DEPTH)
        share = 0.10
    pr, N = base["primary"], W * H
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    cam_pos = base["cam"].worldori[:3].copy()
    orays, oactive = AO.rays(cam_pos, pr["t"], pr["dir"], pr["id"], verts, faces, EPS, 0, N, N)
    radius = float(np.float32(share * extent(s)))
    samples = light_disk(ugrt, s, S_FRAME, radius)
    expanded = []
    plain = cpu_mask(OC, AR, base["ugrid"], verts, faces, orays, oactive, samples, 0, N, N, keep=expanded)
    mask = plain if name != "glass" else cpu_mask(OC, AR, base["thru"], verts, faces, orays, oactive, samples, 0, N, N)
    out = dict(base=base, scene=s, orays=orays, oactive=oactive, samples=samples, radius=radius, plain=plain, mask=mask,
               counts=mask_counts(mask, oactive, S_FRAME), expanded=expanded, cam_pos=cam_pos, N=N, W=W, H=H)
    _AREA[name] = out
    return out


AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (0, .6, .8)]


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    for name in ("trace_dda_any_area", "trace_dda_any_area_thru", "shade_area"):
        assert hasattr(ugrt.Context, name), name
    assert ugrt.MAX_AREA_SAMPLES == 32


@pytest.mark.parametrize("axis", AXES)
def test_area_samples_lie_on_the_disk(ugrt, axis):
    centre, radius = np.float64([1.5, -2.0, 3.25]), 0.75
    for S in (1, 5, 16, 32):
        pos = ugrt.scenes.area_samples(S, centre, axis, radius)
        assert pos.dtype == np.float32 and pos.shape == (S, 3)
        a = np.float64(axis) / np.linalg.norm(np.float64(axis))
        rel = pos.astype(np.float64) - centre
        assert (np.abs(rel @ a) <= 1e-5 * radius).all()
        r = np.sqrt((rel * rel).sum(1))
        assert (np.diff(r) > 0).all() and (r < radius).all() and (r > 0).all()
        np.testing.assert_allclose(r, radius * np.sqrt((np.arange(S) + 0.5) / S), rtol=0, atol=1e-5 * radius)
        np.testing.assert_array_equal(bits(pos), bits(ugrt.scenes.area_samples(S, centre, axis, radius)))
    # the basis: k = the smallest |a[k]|, ties to the lowest k; T = normalize(a x e_k), B = a x T; sample 0 lies along T
    a = np.float64(axis) / np.linalg.norm(np.float64(axis))
    k = [i for i in range(3) if abs(a[i]) == np.abs(a).min()][0]
    e = np.zeros(3)
    e[k] = 1
    T = np.cross(a, e) / np.linalg.norm(np.cross(a, e))
    p0 = ugrt.scenes.area_samples(4, centre, axis, radius)[0].astype(np.float64) - centre
    np.testing.assert_allclose(p0, radius * np.sqrt(0.125) * T, rtol=0, atol=1e-6)
    # the angle of sample 1 against sample 0, seen along the axis, is the golden angle: B = a x T, not T x a
    p1 = ugrt.scenes.area_samples(4, centre, axis, radius)[1].astype(np.float64) - centre
    phi = np.pi * (3.0 - np.sqrt(5.0))
    B = np.cross(a, T)
    np.testing.assert_allclose(p1, radius * np.sqrt(0.375) * (np.cos(phi) * T + np.sin(phi) * B), rtol=0, atol=1e-6)


def np_shade(img, mask, S, p0, n):
    img = img.copy().reshape(-1, 3)
    m = mask[p0:p0 + n] & low_bits(S)
    dark = np.zeros(n, np.uint32)
    for s in range(S):
        dark += (m >> np.uint32(s)) & np.uint32(1)
    lit = np.uint32(S) - dark
    w = np.uint32(S) + np.uint32(2) * lit
    img[p0:p0 + n] = ((img[p0:p0 + n].astype(np.uint32) * w[:, None]) // np.uint32(3 * S)).astype(np.uint8)
    return img.reshape(-1)


@pytest.mark.parametrize("S", [1, 5, 32])
def test_cpu_shade_is_the_integer_restatement(O, AR, S):
    rng = np.random.RandomState(S)
    N, p0, n = 1000, 100, 800
    img = rng.randint(0, 256, 3 * N).astype(np.uint8)
    img[3 * p0:3 * p0 + 30] = 255
    mask = rng.randint(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    mask[p0:p0 + 200] &= np.uint32(0x1F)
    mask[p0 + 200:p0 + 300] = 0
    mask[p0 + 300:p0 + 320] = 0xFFFFFFFF
    got = AR.shade(img, mask, S, p0, n)
    np.testing.assert_array_equal(got, np_shade(img, mask, S, p0, n))
    np.testing.assert_array_equal(got[:3 * p0], img[:3 * p0])
    np.testing.assert_array_equal(got[3 * (p0 + n):], img[3 * (p0 + n):])
    zero = slice(3 * (p0 + 200), 3 * (p0 + 300))
    np.testing.assert_array_equal(got[zero], img[zero])               # a zero mask leaves the bytes
    full = slice(3 * (p0 + 300), 3 * (p0 + 320))
    np.testing.assert_array_equal(got[full], img[full] // 3)          # a full mask: the byte of add_shadows
    if S < 32:                                                        # bits at or above S are ignored
        high = mask.copy()
        high[p0:p0 + n] |= np.uint32((0xFFFFFFFF << S) & 0xFFFFFFFF)
        np.testing.assert_array_equal(AR.shade(img, high, S, p0, n), got)
        only_high = np.full(N, (0xFFFFFFFF << S) & 0xFFFFFFFF, np.uint32)
        np.testing.assert_array_equal(AR.shade(img, only_high, S, p0, n), img)
    if S == 1:                                                        # add_shadows with the flag in bit 0
        flags = (mask & 1).astype(np.int32)
        want = img.copy()
        O.add_shadows(want, flags, p0, n)
        np.testing.assert_array_equal(got, want)
        assert 100 < int(flags[p0:p0 + n].sum()) < n - 100


class _Rec(RS._Recorder):
    """RS._Recorder that also takes the keywords of a whole frame's calls."""

    def __getattr__(self, name):
        return lambda *a, **kw: self.calls.append((name,) + a)


def _fake_frame_renderer(ugrt):
    """A Renderer that was never constructed, with names in the place of its arrays, around a recording context: every
    call of a one-stream frame is recorded, nothing is allocated."""
    r = RLT._fake_renderer(ugrt)
    r.ctx = _Rec()
    r.__dict__.update(vars(RS._fake_frame(DEPTH)))
    r.__dict__.update(F=12, bbmin=np.zeros(3, np.float32), bbmax=np.ones(3, np.float32), shards=None, aspect=1.0, cam_pos="cam",
                      _d_map="map", _prefix="prefix", d_transmit="tr", d_ior="ior", d_continue="cont", ao_rays="aorays",
                      ao_active="aoact", ao_mask="aomask", area_mask="amask", _inline=False)
    r._upload_cam_pos = lambda worldori: None
    r._ensure_area_buffers = lambda: None
    r._ensure_reflect_buffers = lambda *a: None
    r._ensure_ao_buffers = lambda ao: "dirs"
    return r


def test_area_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    for bad in (-1, 33, 1.5, True, "4", None, np.float32(2)):
        with pytest.raises(ValueError):
            rmod.check_area(bad, 1.0)
    for bad in (None, 0, 0.0, -1.0, float("nan"), "1", True, 1e-60):
        with pytest.raises(ValueError):
            rmod.check_area(4, bad)
    with pytest.raises(ValueError):
        rmod.check_area(4, 1.0, False)                 # shadows=False
    with pytest.raises(ValueError):
        rmod.check_area(4, 1.0, True, [("cam", "pos")])  # setup.lights
    with pytest.raises(ValueError):
        rmod.check_area(4, 1.0, True, None, True)      # two streams / bands
    assert rmod.check_area(0, None) == (0, None) and rmod.check_area(0, -3.0, False, [1], True) == (0, None)
    assert rmod.check_area(16, 0.5) == (16, 0.5) and rmod.check_area(np.int64(32), np.float32(2)) == (32, 2.0)
    assert rmod.check_area(1, 3) == (1, 3.0)
    s = scene(ugrt, "hall")
    for kw in (dict(area=33, area_radius=1.0), dict(area=4), dict(area=4, area_radius=0.0), dict(area=True, area_radius=1.0),
               dict(area=-1, area_radius=1.0), dict(area=4, area_radius=1.0, shadows=False)):
        r = _fake_frame_renderer(ugrt)
        with pytest.raises(ValueError):
            r.display(TL.setup_for(ugrt, s), **kw)
        assert r.ctx.calls == []
    r = _fake_frame_renderer(ugrt)
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s, TL.lights_for(s, 2)), area=4, area_radius=1.0)
    assert r.ctx.calls == []
    r = _fake_frame_renderer(ugrt)
    r.aux = object()  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s), area=4, area_radius=1.0)
    assert r.ctx.calls == []
    r = RLT._fake_renderer(ugrt, aux=object())
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s), area=4, area_radius=1.0)
    assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    with pytest.raises(ValueError):
        br.display(TL.setup_for(ugrt, s), area=4, area_radius=1.0)


def test_area_pass_enqueues_the_rays_and_one_walk(ugrt):
    rmod = RLT._rmod(ugrt)
    f = types.SimpleNamespace(t="t", dir="d", intersect_id="ids", d_verts="v", d_faces="f", reflect_eps=1e-3, ao_rays="orays",
                              ao_active="oact", area_mask="mask")
    c = RS._Recorder()
    rmod.area_pass(c, f, "cam", "samples")
    assert c.calls == [("ao_rays", "cam", "t", "d", "ids", "v", "f", 1e-3, "orays", "oact"),
                       ("trace_dda_any_area", "value", "span", "offset", "v", "f", "orays", "oact", "samples", "mask")]
    c = RS._Recorder()
    rmod.area_pass(c, f, "cam", "samples", ("mi", "tr", 3))
    assert c.calls == [("ao_rays", "cam", "t", "d", "ids", "v", "f", 1e-3, "orays", "oact"),
                       ("trace_dda_any_area_thru", "value", "span", "offset", "v", "f", "orays", "oact", "samples", "mask",
                        "mi", "tr", 3)]


SHADOW_STAGE = ("map_rays_to_light", "grid_build_spherical", "sort_rays", "trace_shadow", "shade_add_shadows")
CAMERA_PASS = ["set_light_position", "upload_camera", "grid_build_perspective", "trace_primary", "upload_camera"]
HARD = ["map_rays_to_light", "grid_build_spherical", "sort_rays", "trace_shadow"]
LEVELS = ["trace_dda", "occlusion_rays", "trace_dda_any", "reflect_rays_next"] * 2 + ["trace_dda", "occlusion_rays", "trace_dda_any"]


def _names(r):
    return [c[0] for c in r.ctx.calls]


def test_an_area_frame_has_no_light_space_shadow_stage_and_area_0_is_the_frame_as_it_was(ugrt):
    s = RFR.scene(ugrt, "glass")
    setup = ugrt.FrameSetup.from_scene(s)
    reflect = dict(reflect=True, bounces=DEPTH, reflect_shadows=True)
    # area = 0: the calls of the frame without the keyword, which are those written out here
    for kw, want in ((dict(), CAMERA_PASS + HARD + ["shade_simple", "shade_add_shadows"]),
                     (dict(ao=4, ao_radius=1.0), CAMERA_PASS + HARD + ["grid_build_uniform", "ao_rays", "trace_dda_any_hemi",
                                                                      "shade_simple", "shade_add_shadows", "shade_ao"]),
                     (reflect, CAMERA_PASS + HARD + ["reflect_rays", "grid_build_uniform"] + LEVELS
                      + ["shade_reflect_depth_occluded", "shade_add_shadows"]),
                     (dict(shade=False), CAMERA_PASS + HARD)):
        a, b = _fake_frame_renderer(ugrt), _fake_frame_renderer(ugrt)
        a.display(setup, **kw)
        b.display(setup, area=0, area_radius=-5.0, **kw)
        assert _names(a) == want, kw
        assert [c[:1] + tuple(x for x in c[1:] if isinstance(x, (str, int))) for c in a.ctx.calls] \
            == [c[:1] + tuple(x for x in c[1:] if isinstance(x, (str, int))) for c in b.ctx.calls]
    # area > 0
    for kw, want in ((dict(), CAMERA_PASS + ["grid_build_uniform", "ao_rays", "trace_dda_any_area", "shade_simple", "shade_area"]),
                     (dict(ao=4, ao_radius=1.0), CAMERA_PASS + ["grid_build_uniform", "ao_rays", "trace_dda_any_area",
                                                              "trace_dda_any_hemi", "shade_simple", "shade_area", "shade_ao"]),
                     (reflect, CAMERA_PASS + ["reflect_rays", "grid_build_uniform"] + LEVELS
                      + ["ao_rays", "trace_dda_any_area", "shade_reflect_depth_occluded", "shade_area"]),
                     (dict(refract=True, **reflect),
                      CAMERA_PASS + ["refract_rays", "grid_build_uniform"]
                      + [{"trace_dda_any": "trace_dda_any_thru", "reflect_rays_next": "refract_rays_next"}.get(x, x) for x in LEVELS]
                      + ["ao_rays", "trace_dda_any_area_thru", "shade_reflect_depth_occluded", "shade_area"]),
                     (dict(shade=False), CAMERA_PASS)):
        r = _fake_frame_renderer(ugrt)
        r.display(setup, area=5, area_radius=0.5, **kw)
        names = _names(r)
        assert names == want, (kw, names)
        assert not set(names) & set(SHADOW_STAGE)
        if kw.get("shade", True):
            assert names.count("shade_area") == 1
            walk = [c for c in r.ctx.calls if c[0].startswith("trace_dda_any_area")][0]
            eye = np.asarray(setup.light_camera["eye"], np.float64)
            disk = ugrt.scenes.area_samples(5, eye, np.asarray(setup.light_camera["look"], np.float64) - eye, 0.5)
            np.testing.assert_array_equal(bits(walk[8]), bits(disk))
            assert walk[1:8] == ("value", "span", "offset", "v", "f", "aorays", "aoact") and walk[9] == "amask"
            if kw.get("refract"):
                assert walk[10:] == ("mi", "tr", 3)
            assert [c for c in r.ctx.calls if c[0] == "shade_area"][0][1:] == ("img", "amask", 5)


@pytest.mark.parametrize("name", ["hall", "crash"])
def test_cpu_masks_are_feasible_and_the_walk_finds_what_every_triangle_finds(ugrt, O, REFS, AO, AR, name):
    """S = 16 at 10 % of the extent on the fixtures of section 6.2: lit, umbra and penumbra each hold at least 1000 hit
    pixels, every sample is occluded on at least 1000, and oc_trace_any == oc_brute_any on every explicit ray.  The
    counts are those of DESIGN.md section 6.7."""
    a = cpu_area(O, REFS, AO, AR, ugrt, name)
    s, N, c = a["scene"], a["N"], a["counts"]
    hard = a["base"]["is_shadowed"] == 1
    full = low_bits(S_FRAME)
    print("%s: radius %r, %d hit pixels, lit %d, umbra %d, penumbra %d, per bit %s; %d hard-shadow flags, %d in the umbra, "
          "%d fully lit" % (name, a["radius"], int(a["oactive"].sum()), c["lit"], c["umbra"], c["penumbra"], c["per_bit"],
                            int(hard.sum()), int((hard & (a["mask"] == full)).sum()),
                            int((hard & (a["mask"] == 0) & (a["oactive"] != 0)).sum())))
    assert abs(a["radius"] - 2.8) < 0.05
    assert c["lit"] >= 1000 and c["umbra"] >= 1000 and c["penumbra"] >= 1000, c
    assert min(c["per_bit"]) >= 1000, c
    pr = a["base"]["primary"]
    np.testing.assert_array_equal(a["oactive"], ((pr["t"] > 0) & (pr["id"] >= 0)).astype(np.int32))
    assert not a["mask"][a["oactive"] == 0].any() and not (a["mask"] >> np.uint32(S_FRAME)).any()
    for k, rays in enumerate(a["expanded"]):
        brute = REFS[1].brute_any(s["verts"], s["faces"], rays, a["oactive"], 1.0, 0, N, N)
        np.testing.assert_array_equal(brute.astype(np.uint32), (a["mask"] >> np.uint32(k)) & 1, err_msg="sample %d" % k)


def test_cpu_glass_lets_the_light_through(ugrt, O, REFS, AO, AR, RF):
    """glass at 256 x 256, S = 16, 3 % of the extent: the see-through mask is a subset of the plain one, the two differ
    on at least 1000 pixels, and the see-through mask is non-zero on at least 100."""
    a = cpu_area(O, REFS, AO, AR, ugrt, "glass", RF)
    assert abs(a["radius"] - 0.3) < 0.01
    differ, nonzero = int((a["mask"] != a["plain"]).sum()), int((a["mask"] != 0).sum())
    print("glass: radius %r, plain and see-through masks differ on %d pixels, see-through non-zero on %d"
          % (a["radius"], differ, nonzero))
    assert not (a["mask"] & ~a["plain"]).any()
    assert differ >= 1000 and nonzero >= 100


# ------------------------------------------------------------------------------------------------- the synthetic rays

SYN_N = AM.SYN_N
SYN_SETS = (((4.0, 4.0, 3.5), 3.0), ((4.0, 4.0, 12.0), 6.0))  # inside the grid; the targets outside it
SYN_AXIS = (0.0, 0.0, -1.0)


def syn_samples(ugrt, S, k):
    centre, radius = SYN_SETS[k]
    return ugrt.scenes.area_samples(S, centre, SYN_AXIS, radius)


def syn_origins(glass=False):
    """test_ambient.syn_ambient's origins (4035 of 4096 active); glass: moved to z = 1.2, below the staggered lattices."""
    orays, oactive = AM.syn_ambient()
    if glass:
        orays = orays.copy()
        orays.reshape(-1, 6)[:, 2] = np.float32(1.2)
    return orays, oactive


_SYN_MASKS = {}


def syn_mask(O, REFS, AR, SYN, ugrt, S, k, kind="plain", p0=0, n=SYN_N, keep=None):
    """kind: "plain" on the any-hit scene of test_reflect_shadows; "glass_plain" and "glass_thru" on test_refract.syn_glass
    (all its triangles; without the see-through ones)."""
    key = (S, k, kind, p0, n)
    if key not in _SYN_MASKS or keep is not None:
        sc = SYN if kind == "plain" else RFR.syn_glass(O)
        orays, oactive = syn_origins(kind != "plain")
        grid = sc["thru"] if kind == "glass_thru" else sc["grid"]
        _SYN_MASKS[key] = cpu_mask(REFS[1], AR, grid, sc["verts"], sc["faces"], orays, oactive, syn_samples(ugrt, S, k), p0, n,
                                   SYN_N, fill=0xFFFFFFFF, keep=keep)
    return _SYN_MASKS[key]


def bit_counts(mask, act, S):
    return [int(((mask[act] >> np.uint32(s)) & 1).sum()) for s in range(S)]


def test_synthetic_masks_are_not_vacuous(ugrt, O, REFS, AR, SYN):
    """CPU: 4035 active rays (no multiple of 32) with every list length under them; at S = 32 every bit is set on at
    least 31 rays and clear on at least 31 for both sample sets, plain and through glass; plain and see-through masks
    differ on at least 1000 pixels; the walk equals brute force on the explicit rays."""
    orays, oactive = syn_origins()
    assert int(oactive.sum()) == 4035 and int(oactive.sum()) % 32
    act = oactive != 0
    lo, hi = SYN["verts"].min(0).astype(np.float64), SYN["verts"].max(0).astype(np.float64)
    cells = np.floor((orays.reshape(-1, 6)[act, :2] - lo[:2]) / ((hi[:2] - lo[:2]) / np.float64(RS.SYN_DIMS[:2]))).astype(int)
    under = set(map(tuple, cells))
    for length, ij in RS.SYN_CELLS.items():
        assert ij in under, length
    nact = int(act.sum())
    for k in range(len(SYN_SETS)):
        expanded = []
        mask = syn_mask(O, REFS, AR, SYN, ugrt, 32, k, keep=expanded)
        per = bit_counts(mask, act, 32)
        five = bit_counts(syn_mask(O, REFS, AR, SYN, ugrt, 5, k), act, 5)
        print("set %d: S = 32 rarest bit set on %d rays, commonest on %d of %d; S = 5 rarest on %d"
              % (k, min(per), max(per), nact, min(five)))
        assert min(per) >= 31 and nact - max(per) >= 31, per
        assert min(five) >= 31 and nact - max(five) >= 31, five
        assert not mask[~act].any()
        for s in (0, 13, 31):
            brute = REFS[1].brute_any(SYN["verts"], SYN["faces"], expanded[s], oactive, 1.0, 0, SYN_N, SYN_N)
            np.testing.assert_array_equal(brute.astype(np.uint32), (mask >> np.uint32(s)) & 1)
        plain = syn_mask(O, REFS, AR, SYN, ugrt, 32, k, "glass_plain")
        thru = syn_mask(O, REFS, AR, SYN, ugrt, 32, k, "glass_thru")
        pp, tt = bit_counts(plain, act, 32), bit_counts(thru, act, 32)
        print("set %d, glass: masks differ on %d pixels; rarest bit set on %d (plain) and %d (see-through) rays"
              % (k, int((plain != thru).sum()), min(pp), min(tt)))
        assert not (thru & ~plain).any() and int((plain != thru).sum()) >= 1000
        for per in (pp, tt):
            assert min(per) >= 31 and nact - max(per) >= 31, per


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_words = AM._words


def _area(ctx, grid, dv, df, d_orays, d_oactive, samples, torch, thru=None):
    mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)  # 0xFFFFFFFF
    if thru is None:
        ctx.trace_dda_any_area(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, samples, mask)
    else:
        ctx.trace_dda_any_area_thru(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, samples, mask, *thru)
    ctx.synchronize()
    return _words(mask)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 31, 32])
def test_synthetic_area_walk(ugrt, O, REFS, AR, SYN, torch, S):
    """List lengths 1, 7, 8, 9, 63, 64, 65 and 129 under 4035 origins, two sample sets, the mask pre-filled with ones:
    equal to the checker, to S launches of ugrt_trace_dda_any on the explicit rays and, up to 8 samples, to the layers
    of ugrt_trace_dda_any_lights."""
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = syn_origins()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    for k in range(len(SYN_SETS)):
        samples = syn_samples(ugrt, S, k)
        expanded = []
        want = syn_mask(O, REFS, AR, SYN, ugrt, S, k, keep=expanded)
        got = _area(ctx, grid, dv, df, d_orays, d_oactive, samples, torch)
        np.testing.assert_array_equal(got, want, err_msg="S %d set %d" % (S, k))
        assert not (got >> np.uint32(S)).any() if S < 32 else True
        assert not got[oactive == 0].any()
        composed = np.zeros(SYN_N, np.uint32)
        for s in range(S):
            occ = torch.full((SYN_N,), -7, dtype=torch.int32, device=ctx.device)
            ctx.trace_dda_any(grid[0], grid[1], grid[2], dv, df, ctx.upload(expanded[s]), d_oactive, 1.0, occ)
            composed |= occ.cpu().numpy().astype(np.uint32) << np.uint32(s)
        np.testing.assert_array_equal(got, composed, err_msg="S %d set %d" % (S, k))
        if S <= ugrt.MAX_LIGHTS:
            layers = torch.full((S, SYN_N), -7, dtype=torch.int32, device=ctx.device)
            ctx.trace_dda_any_lights(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, [tuple(p) for p in samples], layers)
            ctx.synchronize()
            packed = np.zeros(SYN_N, np.uint32)
            for s in range(S):
                packed |= layers[s].cpu().numpy().astype(np.uint32) << np.uint32(s)
            np.testing.assert_array_equal(got, packed, err_msg="S %d set %d" % (S, k))
        per = bit_counts(got, oactive != 0, S)
        assert min(per) >= 31 and int((oactive != 0).sum()) - max(per) >= 31


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 32])
def test_synthetic_see_through_walk(ugrt, O, REFS, AR, SYN, torch, S):
    """syn_glass (every third face see-through), any_coop 1 (every list by the wave), 8 and 2^30 (every list by its lane):
    equal to the checker on the filtered grid, to S launches of ugrt_trace_dda_any_thru, and with transmit all zero to
    the plain call's words."""
    G = RFR.syn_glass(O)
    ctx, dv, df, grid = RS._syn_context(ugrt, G)
    orays, oactive = syn_origins(True)
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    d_mat, d_tr, d_zero = ctx.upload(G["matidx"]), ctx.upload(RFR.SYN_TRANSMIT), ctx.upload(np.zeros(2, np.float32))
    for k in range(len(SYN_SETS)):
        samples = syn_samples(ugrt, S, k)
        expanded = []
        want = syn_mask(O, REFS, AR, SYN, ugrt, S, k, "glass_thru", keep=expanded)
        plain = syn_mask(O, REFS, AR, SYN, ugrt, S, k, "glass_plain")
        assert int((want != plain).sum()) >= (1000 if S == 32 else 100)  # (the CPU test's figures are S = 32's)
        for coop in (1, 8, 1 << 30):
            ctx.set_option("any_coop", coop)
            what = "S %d set %d any_coop %d" % (S, k, coop)
            got = _area(ctx, grid, dv, df, d_orays, d_oactive, samples, torch, (d_mat, d_tr, 2))
            np.testing.assert_array_equal(got, want, err_msg=what)
            opaque = _area(ctx, grid, dv, df, d_orays, d_oactive, samples, torch, (d_mat, d_zero, 2))
            np.testing.assert_array_equal(opaque, _area(ctx, grid, dv, df, d_orays, d_oactive, samples, torch), err_msg=what)
            np.testing.assert_array_equal(opaque, plain, err_msg=what)
        ctx.set_option("any_coop", -1)
        composed = np.zeros(SYN_N, np.uint32)
        for s in range(S):
            occ = torch.full((SYN_N,), -7, dtype=torch.int32, device=ctx.device)
            ctx.trace_dda_any_thru(grid[0], grid[1], grid[2], dv, df, ctx.upload(expanded[s]), d_oactive, 1.0, occ, d_mat, d_tr, 2)
            composed |= occ.cpu().numpy().astype(np.uint32) << np.uint32(s)
        np.testing.assert_array_equal(want, composed, err_msg="S %d set %d" % (S, k))


@pytest.mark.gpu
def test_launch_shapes_change_no_word(ugrt, O, REFS, AR, SYN, torch):
    """any_rays_per_wave (1 and 7: fewer lanes than samples, one pixel per wave; 7 and 32 at S = 5: lanes left idle) x
    any_coop, dda_blocks = 1 (every later group comes from the ticket) and a band context whose other pixels keep their
    words."""
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = syn_origins()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    for S in (5, 32):
        samples = syn_samples(ugrt, S, 0)
        want = syn_mask(O, REFS, AR, SYN, ugrt, S, 0)
        for rpw in (1, 7, 32, 64):
            for coop in (1, 8, 1 << 30):
                ctx.set_option("any_rays_per_wave", rpw)
                ctx.set_option("any_coop", coop)
                got = _area(ctx, grid, dv, df, d_orays, d_oactive, samples, torch)
                np.testing.assert_array_equal(got, want, err_msg="S %d, rays per wave %d, coop %d" % (S, rpw, coop))
        ctx.set_option("any_rays_per_wave", -1)
        ctx.set_option("any_coop", -1)
        ctx.set_option("dda_blocks", 1)
        np.testing.assert_array_equal(_area(ctx, grid, dv, df, d_orays, d_oactive, samples, torch), want)
        ctx.set_option("dda_blocks", -1)
        band, bv, bf, bgrid = RS._syn_context(ugrt, SYN, (2, 5))
        p0, n = band.p0, band.npix
        assert (p0, n) == (1024, 1536)
        got = _area(band, bgrid, bv, bf, band.upload(orays), band.upload(oactive), samples, torch)
        np.testing.assert_array_equal(got, syn_mask(O, REFS, AR, SYN, ugrt, S, 0, p0=p0, n=n))
        assert (got[:p0] == 0xFFFFFFFF).all() and (got[p0 + n:] == 0xFFFFFFFF).all()
        np.testing.assert_array_equal(got[p0:p0 + n], want[p0:p0 + n])


@pytest.mark.gpu
def test_the_walk_leaves_the_shared_dda_state_alone(ugrt, O, REFS, AO, AR, torch):
    """hall: a ugrt_trace_dda before and after an area launch gives identical hits, and the split walks' figures stay
    what they were."""
    a = cpu_area(O, REFS, AO, AR, ugrt, "hall")
    s, N = a["scene"], a["N"]
    W, H = SIZES["hall"]
    ctx, r = RD.make(ugrt, s, W, H)
    ctx.set_option("dda_split", 1)
    ctx.set_option("dda_split_load", 50)
    r.display(RD.setup_for(ugrt, s), shadows=True, reflect=True)
    g = ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3]

    def level1():
        ht = torch.full((N,), 5.0, device=ctx.device)
        hid = torch.full((N,), 5, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda(g[0], g[1], g[2], r.d_verts, r.d_faces, r.rays, r.active, ht, hid)
        ctx.synchronize()
        return ht, hid

    level1()
    ht0, hid0 = level1()
    before = ctx.stats_dda_split()
    mask = torch.full((N,), -1, dtype=torch.int32, device=ctx.device)
    ctx.trace_dda_any_area(g[0], g[1], g[2], r.d_verts, r.d_faces, ctx.upload(a["orays"]), ctx.upload(a["oactive"]),
                           a["samples"], mask)
    ctx.synchronize()
    np.testing.assert_array_equal(_words(mask), a["mask"])
    assert ctx.stats_dda_split() == before
    ht1, hid1 = level1()
    assert torch.equal(hid0, hid1) and torch.equal(ht0.view(torch.int32), ht1.view(torch.int32))
    np.testing.assert_array_equal(hid1.cpu().numpy(), a["base"]["levels"][0]["hit_id"])
    assert ctx.stats_dda_split() == before


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, REFS, AR, SYN, torch):
    fresh = ugrt.Context(64, 64, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS)
    z = torch.zeros(6 * SYN_N, dtype=torch.int32, device=fresh.device)
    samples = syn_samples(ugrt, 4, 0)
    for call, extra in ((fresh.trace_dda_any_area, ()), (fresh.trace_dda_any_area_thru, (z, z, 2))):
        with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
            call(z, z, z, z, z, z, z, samples, z, *extra)
        assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = syn_origins()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)
    d_mat = ctx.upload(np.zeros(len(SYN["faces"]), np.int32))
    d_tr = ctx.upload(np.zeros(2, np.float32))
    args = [grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, samples, mask]
    targs = args + [d_mat, d_tr, 2]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    for bad in (np.zeros((0, 3), np.float32), np.zeros((33, 3), np.float32)):
        fails(ctx.trace_dda_any_area, args[:7] + [bad] + args[8:], b"num_samples")
        fails(ctx.trace_dda_any_area_thru, targs[:7] + [bad] + targs[8:], b"num_samples")
    for h in range(9):
        fails(ctx.trace_dda_any_area, args[:h] + [None] + args[h + 1:], b"null")
    for h in list(range(9)) + [9, 10]:
        fails(ctx.trace_dda_any_area_thru, targs[:h] + [None] + targs[h + 1:], b"null")
    img = torch.full((3 * SYN_N,), 200, dtype=torch.uint8, device=ctx.device)
    for bad in (0, 33, -1):
        fails(ctx.shade_area, [img, mask, bad], b"num_samples")
    for h in (0, 1):
        a = [img, mask, 4]
        fails(ctx.shade_area, a[:h] + [None] + a[h + 1:], b"null")
    ctx.synchronize()
    assert (_words(mask) == 0xFFFFFFFF).all() and (img == 200).all()  # nothing was enqueued
    want = syn_mask(O, REFS, AR, SYN, ugrt, 4, 0)
    np.testing.assert_array_equal(_area(ctx, grid, dv, df, d_orays, d_oactive, samples, torch), want)
    # the shading on the device against the checker (bits at or above S are ignored)
    rng = np.random.RandomState(3)
    h_img = rng.randint(0, 256, 3 * SYN_N).astype(np.uint8)
    h_mask = rng.randint(0, 1 << 32, SYN_N, dtype=np.uint64).astype(np.uint32)
    h_mask[::3] = 0
    h_mask[1::7] = 0xFFFFFFFF
    for S in (1, 4, 5, 32):
        d_img = ctx.upload(h_img)
        ctx.shade_area(d_img, ctx.upload(h_mask.view(np.int32)), S)
        ctx.synchronize()
        np.testing.assert_array_equal(d_img.cpu().numpy(), AR.shade(h_img, h_mask, S, 0, SYN_N))
        np.testing.assert_array_equal(d_img.cpu().numpy(), np_shade(h_img, h_mask, S, 0, SYN_N))


def _unshadowed_depth(REFS, want, s, weights, depth, N):
    """The occluded depth shading of a CPU frame WITHOUT add_shadows."""
    pr, st = want["primary"], want["stack"]
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    img, ids = REFS[1].shade_depth_occluded(want["lcam"].cc, s["shading_light"], pr["normal"], pr["t"], pr["dir"], pr["id"],
                                            want["cam"].worldori[:3], s["matidx"], s["mat_list"], weights, verts, faces, depth,
                                            st["rays"], st["active"], st["hit_t"], st["hit_id"], st["occluded"], 0, N, N)
    return img, ids


def _frames(O, REFS, AO, AR, RF, ugrt, name):
    """(what, display keywords, unshadowed CPU image, hard-shadow CPU image, CPU material ids, ao) of the frames an area
    light renders in."""
    a = cpu_area(O, REFS, AO, AR, ugrt, name, RF)
    s, N, W, H = a["scene"], a["N"], a["W"], a["H"]
    base = a["base"]
    if name == "glass":
        img, ids = _unshadowed_depth(REFS, base, s, s["continue"], DEPTH, N)
        return [("refract", dict(shadows=True, reflect=True, refract=True, bounces=DEPTH, reflect_shadows=True), img,
                 base["image_occluded"], ids, None)]
    plain = TL.cpu_frame(O, ugrt, name, W, H)
    amb = AM.cpu_ambient(O, REFS, AO, ugrt, name)
    img, ids = _unshadowed_depth(REFS, base, s, s["reflect"], DEPTH, N)
    np.testing.assert_array_equal(ids, base["mat_ids_occluded"])
    reflect = dict(shadows=True, reflect=True, bounces=DEPTH, reflect_shadows=True)
    return [("plain", dict(shadows=True), plain["image_unshadowed"], plain["image"], plain["mat_ids"], None),
            ("plain, ao", dict(shadows=True), plain["image_unshadowed"], plain["image"], plain["mat_ids"], amb),
            ("reflect", reflect, img, base["image_occluded"], ids, None),
            ("reflect, ao", reflect, img, base["image_occluded"], ids, amb)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "crash", "glass"])
def test_frames_with_an_area_light_equal_the_cpu_frames(ugrt, O, REFS, AO, AR, RF, torch, name):
    """Plain, with ao = 16, reflections of depth 3 with reflect_shadows, that with ao = 16 (hall, crash); the refract
    frame of depth 3 with reflect_shadows (glass: the see-through mask).  area_mask is the CPU mask, the material ids
    are the frame's own, the image is the frame's shading without add_shadows, then area_shade with the CPU mask, then
    ao_shade; it differs from the hard-shadow frame; area = 0 before and behind an area frame is the CPU frame."""
    a = cpu_area(O, REFS, AO, AR, ugrt, name, RF)
    s, N, W, H = a["scene"], a["N"], a["W"], a["H"]
    setup = ugrt.FrameSetup.from_scene(s)
    for what, kw, w_plain, w_hard, w_ids, amb in _frames(O, REFS, AO, AR, RF, ugrt, name):
        ctx, r = RFR.make(ugrt, s) if name == "glass" else RD.make(ugrt, s, W, H)
        ao_kw = dict(ao=AM.S_FRAME, ao_radius=amb["radius"]) if amb else {}
        hard = AO.shade(w_hard, amb["mask"], AM.S_FRAME, 0, N) if amb else w_hard
        r.display(setup, area=0, **kw, **ao_kw)
        ctx.synchronize()
        assert r.area_mask is None
        np.testing.assert_array_equal(r.image.cpu().numpy(), hard, err_msg=what)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), a["base"]["is_shadowed"], err_msg=what)
        r.display(setup, area=S_FRAME, area_radius=a["radius"], **kw, **ao_kw)
        ctx.synchronize()
        np.testing.assert_array_equal(_words(r.area_mask), a["mask"], err_msg=what)
        np.testing.assert_array_equal(r.ao_active.cpu().numpy(), a["oactive"], err_msg=what)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        shaded = AR.shade(w_plain, a["mask"], S_FRAME, 0, N)
        if amb:
            np.testing.assert_array_equal(_words(r.ao_mask), amb["mask"], err_msg=what)
            shaded = AO.shade(shaded, amb["mask"], AM.S_FRAME, 0, N)
        np.testing.assert_array_equal(r.image.cpu().numpy(), shaded, err_msg=what)
        assert int((shaded != hard).sum()) > 1000, what
        r.display(setup, **kw, **ao_kw)
        ctx.synchronize()
        np.testing.assert_array_equal(r.image.cpu().numpy(), hard, err_msg=what + ", behind an area frame")
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), a["base"]["is_shadowed"], err_msg=what)
