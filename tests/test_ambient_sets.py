"""Ambient occlusion over interleaved direction sets: ugrt_trace_dda_any_hemi_sets,
ugrt_ao_shade_vis, scenes.ao_direction_sets and Renderer.display(..., ao_sets=, ao_filter=, ao_filter_cos=,
ao_filter_plane=).

The walk has no restatement of its own: the expected words are test_ambient.cpu_mask once per set (oc_trace_any on the
explicit rays), selected per pixel by sets_select of tests/area_sets_ref.c; the gather is that file's sets_filter
(tests/test_filter_visibility.py checks it) and the shading behind it is tests/ambient_sets_ref.c, built here with the
oracle's flags.  The frames underneath are those of tests/test_ambient.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_ambient as AM
import test_area_light as TA
import test_area_sets as TS
import test_filter_visibility as FV
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
import test_refract as RFR
from test_ambient import AO  # noqa: F401  (fixtures)
from test_area_light import AR  # noqa: F401
from test_filter_visibility import SR, open_of  # noqa: F401
from test_lights import LT  # noqa: F401
from test_reflect_lights import RL  # noqa: F401
from test_reflect_shadows import REFS, SYN  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, _u32, bits, scene, SIZES = RD._p, RD._f32, RD._i32, AM._u32, RD.bits, RD.scene, RD.SIZES
CALLS = ("ugrt_trace_dda_any_hemi_sets", "ugrt_ao_shade_vis")
S_SETS, SETS, R_FRAME = 8, 16, 2  # the frames: ao=8, ao_sets=16, ao_filter=2
TILES = {1: (1, 1), 4: (2, 2), 16: (4, 4)}
DEPTH = AM.DEPTH
SYN_N, SYN_RADII = AM.SYN_N, AM.SYN_RADII


class AmbientSetsRef:
    def __init__(self, lib):
        self.lib = lib

    def shade(self, img, vis, num_dirs, p0, n):
        img = np.ascontiguousarray(img, np.uint8).copy()
        self.lib.ao_sets_shade(_p(img), _p(_u32(vis)), C.c_int(num_dirs), C.c_int(p0), C.c_int(n))
        return img


@pytest.fixture(scope="session")
def ASR(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ambient_sets_ref") / "libambient_sets_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "ambient_sets_ref.c"), "-lm"], check=True, capture_output=True)
    return AmbientSetsRef(C.CDLL(out))


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    for name in ("trace_dda_any_hemi_sets", "shade_ao_vis"):
        assert hasattr(ugrt.Context, name), name
    assert (ugrt.MAX_AO_SET_TILE, ugrt.MAX_AO_SET_DIRS) == (4, 512)
    assert ugrt.lib.ugrt_version() == 105


def test_ao_direction_sets(ugrt):
    for S in (1, 4, 8, 31, 32):
        fixed = ugrt.scenes.ao_directions(S)
        for sets in (1, 4, 16):
            d = ugrt.scenes.ao_direction_sets(S, sets)
            assert d.dtype == np.float32 and d.shape == (sets, S, 3)
            np.testing.assert_array_equal(bits(d[0]), bits(fixed))
            d64 = d.astype(np.float64)
            np.testing.assert_allclose((d64 ** 2).sum(2), 1.0, rtol=0, atol=1e-6)
            assert (d[:, :, 2] > 0).all()
            for j in range(sets):
                for k in range(j):
                    assert np.abs(d[j] - d[k]).max() > 1e-3, (S, sets, j, k)
            # set k is set 0 turned by 2 pi rank[k] / sets about z, counter-clockwise seen from +z
            rank = ugrt.scenes.AREA_SET_RANK[sets]
            for k in range(sets):
                phi = 2.0 * np.pi * rank[k] / sets
                turned = np.stack([d64[0, :, 0] * np.cos(phi) - d64[0, :, 1] * np.sin(phi),
                                   d64[0, :, 0] * np.sin(phi) + d64[0, :, 1] * np.cos(phi), d64[0, :, 2]], 1)
                np.testing.assert_allclose(d64[k], turned, rtol=0, atol=1e-6)
    for bad in (0, 2, 3, 8, 17, None):
        with pytest.raises(ValueError):
            ugrt.scenes.ao_direction_sets(4, bad)


class _Rows:
    """shadowed_lights of a frame that was never allocated: its rows are names."""

    def __getitem__(self, k):
        return self if isinstance(k, slice) else "shl%d" % k

    def zero_(self):
        pass


def _old_fake(ugrt):
    """test_area_sets' fake frame renderer with what the frames under several lights read besides: it has none of the
    attributes this feature adds."""
    r = TS._fake(ugrt)
    r.__dict__.update(shadowed_lights=_Rows(), occluded_lights=["ocl%d" % (j + 1) for j in range(DEPTH)])
    r._ensure_light_buffers = lambda n: None
    r._ensure_reflect_lights_buffers = lambda *a: None
    return r


def _fake(ugrt):
    r = _old_fake(ugrt)
    r.__dict__.update(ao_vis="aovis", _ao_set_tables={})
    r._ensure_ao_buffers = lambda ao: ugrt.scenes.ao_directions(ao)
    r._ensure_ao_filter_buffers = lambda: None
    r._upload_ao_sets = lambda table: ("aotable", table)
    return r


def test_the_new_keywords_are_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    chk = rmod.check_ao_filter
    assert chk(0) == (1, 0, None, None) and chk(8) == (1, 0, None, None)
    assert chk(8, 16, 2, 0.9, None) == (16, 2, float(np.float32(0.9)), None)
    assert chk(8, np.int64(4), np.int32(8), 1, 0) == (4, 8, 1.0, 0.0)
    assert chk(8, 1, 0, "junk", "junk") == (1, 0, None, None)  # (not looked at without a gather)
    for bad in (0, 2, 3, 8, 17, 16.0, True, "4", None):
        with pytest.raises(ValueError):
            chk(8, bad)
    for bad in (-1, 9, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            chk(8, 1, bad)
    for bad in (None, "x", True, float("nan")):
        with pytest.raises(ValueError):
            chk(8, 1, 2, bad)
    for bad in (-1e-9, float("nan"), "x", True):
        with pytest.raises(ValueError):
            chk(8, 1, 2, 0.9, bad)
    for kw in (dict(ao_sets=4), dict(ao_filter=1), dict(ao_sets=16, ao_filter=2)):
        with pytest.raises(ValueError):
            chk(0, **kw)
    # check_area_filter, which shares the rules, still says what it said
    assert rmod.check_area_filter(8, 16, 2, 0.9, None) == (16, 2, float(np.float32(0.9)), None)
    with pytest.raises(ValueError, match="area_sets must be 1, 4 or 16"):
        rmod.check_area_filter(8, 3)
    s = scene(ugrt, "hall")
    ao = dict(ao=8, ao_radius=1.0)
    for kw in (dict(ao_sets=16), dict(ao_filter=2), dict(ao_sets=3, **ao), dict(ao_filter=9, **ao),
               dict(ao_filter=2, ao_filter_plane=-1.0, **ao), dict(ao_filter=2, ao_filter_cos=None, **ao),
               dict(ao_sets=16, ao=8), dict(ao_sets=16.0, **ao), dict(ao_filter=True, **ao)):
        for lights in (None, TL.lights_for(s, 2)):
            r = _fake(ugrt)
            with pytest.raises(ValueError):
                r.display(TL.setup_for(ugrt, s, lights), **kw)
            assert r.ctx.calls == [], kw
    for kw in (dict(ao_sets=16, **ao), dict(ao_filter=2, **ao)):
        r = _fake(ugrt)
        r.aux = object()  # a two-stream renderer
        with pytest.raises(ValueError):
            r.display(TL.setup_for(ugrt, s), **kw)
        assert r.ctx.calls == []
        br = object.__new__(ugrt.BandedRenderer)
        with pytest.raises(ValueError):
            br.display(TL.setup_for(ugrt, s), **kw)
    for kw in (dict(ao_sets=16), dict(ao_filter=2)):  # without ao, too
        br = object.__new__(ugrt.BandedRenderer)
        with pytest.raises(ValueError):
            br.display(TL.setup_for(ugrt, s), **kw)


_plain, _names = TS._plain, TA._names
NEW = {"trace_dda_any_hemi_sets", "filter_visibility", "shade_ao_vis"}


def _kinds(ugrt):
    """(setup, display keywords, takes area) of the four frame kinds that take ao."""
    s = scene(ugrt, "hall")
    lights = TL.lights_for(s, 2)
    reflect = dict(reflect=True, bounces=DEPTH, reflect_shadows=True)
    return [(TL.setup_for(ugrt, s), dict(), True), (TL.setup_for(ugrt, s), reflect, True),
            (TL.setup_for(ugrt, s, lights), dict(), False),
            (TL.setup_for(ugrt, s, lights), dict(reflect_lights=True, **reflect), False)]


def test_default_frames_are_call_for_call_the_old_frames(ugrt):
    """Plain, reflect, lights and reflect_lights, with and without area: the defaults written out change no call, the
    names are the old frames', and a renderer without any attribute of this feature renders them."""
    defaults = dict(ao_sets=1, ao_filter=0, ao_filter_cos=0.9, ao_filter_plane=None)
    ao = dict(ao=4, ao_radius=1.0)  # (the old fake's directions are a name of four letters)
    walk = ["grid_build_uniform", "ao_rays", "trace_dda_any_hemi"]
    old = {0: TA.CAMERA_PASS + TA.HARD + walk + ["shade_simple", "shade_add_shadows", "shade_ao"],
           1: TA.CAMERA_PASS + TA.HARD + ["reflect_rays", "grid_build_uniform"] + TA.LEVELS
           + ["ao_rays", "trace_dda_any_hemi", "shade_reflect_depth_occluded", "shade_add_shadows", "shade_ao"]}
    for j, (setup, kw, takes_area) in enumerate(_kinds(ugrt)):
        for area in (dict(), dict(area=5, area_radius=0.5)) if takes_area else (dict(),):
            for amb in (dict(), ao):
                a, b = _old_fake(ugrt), _old_fake(ugrt)
                a.display(setup, **area, **amb, **kw)
                b.display(setup, **area, **amb, **defaults, **kw)
                assert [_plain(c) for c in a.ctx.calls] == [_plain(c) for c in b.ctx.calls], (kw, area, amb)
                assert not NEW & set(_names(a))
                assert _names(a).count("trace_dda_any_hemi") == _names(a).count("shade_ao") == (1 if amb else 0)
                if amb and not area and j in old:
                    assert _names(a) == old[j], kw
                if amb:
                    assert a.ctx.calls[-1] == ("shade_ao", "img", "aomask", 4)
    shade_off = _old_fake(ugrt)
    shade_off.display(_kinds(ugrt)[0][0], shade=False, ao_sets=16, ao_filter=2, **ao)
    assert _names(shade_off) == TA.CAMERA_PASS + TA.HARD


def test_recorded_call_lists(ugrt):
    """ao_sets=16 swaps the walk alone; ao_filter=2 swaps shade_ao alone for the gather and shade_ao_vis; in all four
    frame kinds, and beside an area light with its own sets and gather."""
    ao = dict(ao=8, ao_radius=0.75)
    table16 = ugrt.scenes.ao_direction_sets(8, 16)
    for setup, kw, takes_area in _kinds(ugrt):
        for area in (dict(), dict(area=8, area_radius=0.5, area_sets=16, area_filter=2)) if takes_area else (dict(),):
            base, sets, filt, both = _fake(ugrt), _fake(ugrt), _fake(ugrt), _fake(ugrt)
            base.display(setup, **ao, **area, **kw)
            sets.display(setup, ao_sets=16, **ao, **area, **kw)
            filt.display(setup, ao_filter=2, **ao, **area, **kw)
            both.display(setup, ao_sets=4, ao_filter=3, ao_filter_cos=0.5, ao_filter_plane=0.25, **ao, **area, **kw)
            old, new = "trace_dda_any_hemi", "trace_dda_any_hemi_sets"
            assert _names(base).count(old) == 1 and not {new, "shade_ao_vis"} & set(_names(base))
            # ao_sets: the walk alone
            assert _names(sets) == [new if n == old else n for n in _names(base)]
            for cb, cs in zip(base.ctx.calls, sets.ctx.calls):
                if cb[0] != old:
                    assert _plain(cb) == _plain(cs)
                    continue
                assert cs[1:8] == cb[1:8] == ("value", "span", "offset", "v", "f", "aorays", "aoact")
                np.testing.assert_array_equal(bits(cb[8]), bits(table16[0]))
                assert cb[9:] == (0.75, "aomask")
                assert cs[8:11] == (8, 4, 4) and cs[11][0] == "aotable" and cs[12:] == (0.75, "aomask")
                np.testing.assert_array_equal(bits(cs[11][1]), bits(table16))
            # ao_filter: shade_ao alone
            assert base.ctx.calls[-1] == ("shade_ao", "img", "aomask", 8)
            assert _names(filt) == _names(base)[:-1] + ["filter_visibility", "shade_ao_vis"]
            assert [_plain(c) for c in filt.ctx.calls[:-2]] == [_plain(c) for c in base.ctx.calls[:-1]]
            plane = float(np.float32(0.01))  # (the fake's box is the unit cube)
            assert filt.ctx.calls[-2] == ("filter_visibility", "aomask", 8, "aorays", "aoact", 2, float(np.float32(0.9)), plane, "aovis")
            assert filt.ctx.calls[-1] == ("shade_ao_vis", "img", "aovis", 8)
            # both
            assert _names(both) == [new if n == old else n for n in _names(filt)]
            assert both.ctx.calls[-2] == ("filter_visibility", "aomask", 8, "aorays", "aoact", 3, 0.5, 0.25, "aovis")
            walk = [c for c in both.ctx.calls if c[0] == new][0]
            assert walk[8:11] == (8, 2, 2)
            np.testing.assert_array_equal(bits(walk[11][1]), bits(ugrt.scenes.ao_direction_sets(8, 4)))
            if area:  # the area light's gather keeps its own buffer and comes first
                at = _names(both).index("filter_visibility")
                assert both.ctx.calls[at][1:3] == ("amask", 8) and both.ctx.calls[at][-1] == "avis"
                assert _names(both)[at + 1] == "shade_area_vis" and at < len(both.ctx.calls) - 2
    # the table is uploaded once per (S, sets)
    r, uploads = _fake(ugrt), []
    r._upload_ao_sets = lambda table: uploads.append(table) or len(uploads)
    setup = _kinds(ugrt)[0][0]
    for kw in (dict(ao=8, ao_sets=16), dict(ao=8, ao_sets=16), dict(ao=8, ao_sets=4), dict(ao=4, ao_sets=16),
               dict(ao=8, ao_sets=16, ao_radius=0.25), dict(ao=8, ao_sets=1, ao_filter=1)):
        r.display(setup, **dict(dict(ao_radius=0.5), **kw))
    assert [u.shape for u in uploads] == [(16, 8, 3), (4, 8, 3), (16, 4, 3)]
    walks = [c for c in r.ctx.calls if c[0] == "trace_dda_any_hemi_sets"]
    assert [w[11] for w in walks] == [1, 1, 2, 3, 1]


def np_shade_vis(img, vis, S, p0, n):
    img = img.copy().reshape(-1, 3)
    num, den = vis[0::2][p0:p0 + n].astype(np.uint32), vis[1::2][p0:p0 + n].astype(np.uint32)
    on = den != 0
    px = img[p0:p0 + n].astype(np.uint32)
    px[on] = (px[on] * num[on, None]) // (np.uint32(S) * den[on, None])
    img[p0:p0 + n] = px.astype(np.uint8)
    return img.reshape(-1)


def random_vis(rng, N, S):
    """Sums as the gather leaves them: den in 0..6561 (a sixth of them 0), num in 0..S * den, both ends included."""
    den = rng.randint(1, 6562, N).astype(np.uint32)
    den[::6] = 0
    den[1::6] = 6561
    num = (rng.uniform(size=N) * (S * den.astype(np.float64) + 1)).astype(np.uint32)
    num = np.minimum(num, np.uint32(S) * den)
    num[1::12] = np.uint32(S) * den[1::12]
    num[2::12] = 0
    vis = np.empty(2 * N, np.uint32)
    vis[0::2], vis[1::2] = num, den
    return vis


@pytest.mark.parametrize("S", [1, 5, 32])
def test_cpu_shade_is_the_integer_restatement(AO, SR, ASR, S):
    rng = np.random.RandomState(S)
    N, p0, n = 1000, 100, 800
    img = rng.randint(0, 256, 3 * N).astype(np.uint8)
    img[3 * p0:3 * p0 + 60] = 255
    vis = random_vis(rng, N, S)
    got = ASR.shade(img, vis, S, p0, n)
    np.testing.assert_array_equal(got, np_shade_vis(img, vis, S, p0, n))
    np.testing.assert_array_equal(got[:3 * p0], img[:3 * p0])
    np.testing.assert_array_equal(got[3 * (p0 + n):], img[3 * (p0 + n):])
    px, g = img.reshape(-1, 3), got.reshape(-1, 3)
    num, den = vis[0::2], vis[1::2]
    band = np.zeros(N, bool)
    band[p0:p0 + n] = True
    np.testing.assert_array_equal(g[band & (den == 0)], px[band & (den == 0)])     # den = 0: the pixel as it is
    full = band & (den != 0) & (num == np.uint32(S) * den)
    assert full.sum() > 30
    np.testing.assert_array_equal(g[full], px[full])                                # every ray open: unchanged
    assert (band & (den != 0) & (num == 0)).sum() > 30 and not g[band & (den != 0) & (num == 0)].any()
    assert int(255 * S * 6561) < 2 ** 32
    # behind a gather of radius 0 the bytes are ao_shade's (the walk leaves the words of inactive pixels 0)
    W, H = 40, 25
    orays, oactive = FV.gbuffer(W, H, S)
    mask = FV.random_masks(rng, N)
    mask[oactive == 0] = 0
    vis0 = SR.filter(mask, S, orays, oactive, 0, 0.9, 0.01, W, H)
    np.testing.assert_array_equal(ASR.shade(img, vis0, S, 0, N), AO.shade(img, mask, S, 0, N))
    assert int((AO.shade(img, mask, S, 0, N) != img).sum()) > 500


# ----------------------------------------------------------------------------------------------------- the fixtures' sets

_AMB_SETS = {}


def cpu_ambient_sets(O, REFS, AO, SR, ugrt, name, S=S_SETS, sets=SETS, share=None):
    """The CPU side of a frame's ambient occlusion over direction sets: test_ambient.cpu_ambient's origins, normals and
    radius, the table of scenes.ao_direction_sets, the mask of every set ("per_set" [sets, N]) and the per-pixel
    selection ("mask").  share: the radius as a share of the scene's largest extent instead of cpu_ambient's 5 %.
    Computed once per key and shared: nobody writes to it."""
    key = (name, S, sets, share)
    if key in _AMB_SETS:
        return _AMB_SETS[key]
    a = AM.cpu_ambient(O, REFS, AO, ugrt, name)
    s, N = a["scene"], a["N"]
    W, H = SIZES[name]
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    radius = a["radius"] if share is None else float(np.float32(share * TA.extent(s)))
    table = ugrt.scenes.ao_direction_sets(S, sets)
    per_set = np.stack([AM.cpu_mask(REFS[1], AO, a["base"]["ugrid"], verts, faces, a["orays"], a["oactive"], table[k], radius,
                                    0, N, N) for k in range(sets)])
    tile = TILES[sets]
    out = dict(a=a, table=table, per_set=per_set, tile=tile, mask=SR.select(per_set, tile[0], tile[1], W, H), radius=radius,
               W=W, H=H, N=N)
    _AMB_SETS[key] = out
    return out


def _errors(O, REFS, AO, SR, ugrt, name, part):
    """The mean absolute error of the open share over the partly occluded hit pixels of the 16 x 32-direction truth."""
    rmod = RLT._rmod(ugrt)
    c = cpu_ambient_sets(O, REFS, AO, SR, ugrt, name, share=part)
    a, W, H = c["a"], c["W"], c["H"]
    truth = TS.share(cpu_ambient_sets(O, REFS, AO, SR, ugrt, name, S=32, share=part)["per_set"], 32)
    hit = a["oactive"] != 0
    partly = hit & (truth > 0) & (truth < 1)
    v = _f32(a["scene"]["verts"]).reshape(-1, 3)
    plane = rmod.default_filter_plane(v.min(0), v.max(0))
    assert plane == float(np.float32(0.01 * TA.extent(a["scene"])))
    out = {}
    for what, mask, R in (("fixed", c["per_set"][0], 0), ("interleaved, gather", c["mask"], R_FRAME),
                          ("interleaved", c["mask"], 0), ("fixed, gather", c["per_set"][0], R_FRAME)):
        vis = SR.filter(mask, S_SETS, a["orays"], a["oactive"], R, 0.9, plane, W, H).astype(np.float64)
        out[what] = float(np.abs(vis[0::2][partly] / (S_SETS * vis[1::2][partly]) - truth[partly]).mean())
    return c, int(partly.sum()), out


@pytest.mark.parametrize("name,part,cap", [("crash", 0.05, 0.5), ("hall", 0.05, 0.5), ("crash", 0.02, 0.8), ("hall", 0.02, 0.8)])
def test_interleaved_sets_with_the_gather_cut_the_error(ugrt, O, REFS, AO, SR, name, part, cap):
    """crash 256 x 144 and hall 256 x 256, S = 8, 16 sets, gather of radius 2, cosine 0.9, plane 1 % of the extent: the
    error of the interleaved sets with the gather is below 0.5 of that of the fixed eight directions unfiltered at a
    radius of 5 % of the extent (measured on the CPU: 0.41 and 0.29; the cap leaves room only for rounding differences
    of the table) and below 0.8 at 2 % (measured: 0.59 and 0.64); every set index is used by at least 1000 hit pixels
    and the fixed and the interleaved masks differ on at least 1000 pixels.  The row of DESIGN.md section 6.9 is
    printed."""
    c, npx, err = _errors(O, REFS, AO, SR, ugrt, name, part)
    a, W, H = c["a"], c["W"], c["H"]
    assert (W, H) == SIZES[name] and abs(c["radius"] - part * 28.0) < 0.05 * part * 28.0
    if part == 0.05:
        assert c["radius"] == a["radius"]
    hit = (a["oactive"] != 0).reshape(H, W)
    used = [int(hit[j // 4::4, j % 4::4].sum()) for j in range(16)]
    differ = int((c["mask"] != c["per_set"][0]).sum())
    print("%s, radius %.2f: %d partly occluded pixels; hit pixels per set %s; fixed and interleaved masks differ on %d pixels; "
          "errors %s; ratio %.3f" % (name, c["radius"], npx, used, differ, {k: round(v, 4) for k, v in err.items()},
                                     err["interleaved, gather"] / err["fixed"]))
    assert min(used) >= 1000, used
    assert differ >= 1000
    assert not c["mask"][a["oactive"] == 0].any() and not (c["mask"] >> np.uint32(S_SETS)).any()
    assert err["interleaved, gather"] < cap * err["fixed"], err


# ------------------------------------------------------------------------------------------------- the synthetic rays

# (S, (set_w, set_h)); the sets are the first set_w * set_h of the 16 turned ones, so set j is the same for every tile
WALK_CASES = [(5, (4, 4)), (8, (4, 4)), (8, (3, 2)), (8, (2, 2)), (31, (2, 2)), (32, (4, 4))]


def syn_table(ugrt, S, K):
    return np.ascontiguousarray(ugrt.scenes.ao_direction_sets(S, 16)[:K])


_SYN_PER_SET = {}


def syn_per_set(REFS, AO, SYN, ugrt, S, K, radius):
    """[K, SYN_N] CPU masks of the sets of syn_table on test_ambient.syn_ambient's rays (whole frame), cached per set."""
    orays, oactive = AM.syn_ambient()
    table = syn_table(ugrt, S, K)
    for j in range(K):
        if (S, j, radius) not in _SYN_PER_SET:
            _SYN_PER_SET[(S, j, radius)] = AM.cpu_mask(REFS[1], AO, SYN["grid"], SYN["verts"], SYN["faces"], orays, oactive,
                                                       table[j], radius, 0, SYN_N, SYN_N)
    return np.stack([_SYN_PER_SET[(S, j, radius)] for j in range(K)])


syn_want = TS.syn_want


def test_synthetic_selections_are_not_vacuous(ugrt, O, REFS, AO, SR, SYN):
    """CPU: on the 64 x 64 image of the 4096 synthetic origins the per-pixel selection differs from every single set's
    mask on at least 100 pixels, for every case and radius (the least is 194); set 0 is test_ambient's mask."""
    least = SYN_N
    for S, tile in WALK_CASES:
        K = tile[0] * tile[1]
        for radius in SYN_RADII:
            per = syn_per_set(REFS, AO, SYN, ugrt, S, K, radius)
            want = syn_want(SR, per, tile)
            differ = [int((want != per[j]).sum()) for j in range(K)]
            least = min(least, min(differ))
            assert min(differ) >= 100, (S, tile, radius, differ)
            x, y = np.arange(SYN_N) % 64, np.arange(SYN_N) // 64
            j = (y % tile[1]) * tile[0] + x % tile[0]
            np.testing.assert_array_equal(want, per[j, np.arange(SYN_N)])
    print("the least number of pixels on which a selection differs from a single set: %d" % least)
    np.testing.assert_array_equal(syn_per_set(REFS, AO, SYN, ugrt, 32, 1, 3.0)[0], AM.syn_mask(REFS, AO, SYN, ugrt, 32, 3.0))


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_words, _hemi = AM._words, AM._hemi


def _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, radius, torch):
    mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)  # 0xFFFFFFFF
    d_table = ctx.upload(table.reshape(-1))
    ctx.trace_dda_any_hemi_sets(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, table.shape[1], tile[0], tile[1], d_table,
                                radius, mask)
    ctx.synchronize()
    return _words(mask)


@pytest.mark.gpu
@pytest.mark.parametrize("S,tile", WALK_CASES + [(8, (1, 1))])
def test_synthetic_sets_walk(ugrt, O, REFS, AO, SR, SYN, torch, S, tile):
    """The any-hit scene's 4096 origins and normals as a 64 x 64 image, three radii, the mask pre-filled with ones: equal
    to the CPU masks of the sets selected per pixel and to ugrt_trace_dda_any_hemi per set selected per pixel; at the
    radius of three cells to ugrt_trace_dda_any on the explicit rays of every (set, direction) selected per pixel;
    1 x 1 is ugrt_trace_dda_any_hemi's words."""
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = AM.syn_ambient()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    K = tile[0] * tile[1]
    table = syn_table(ugrt, S, K)
    for radius in SYN_RADII:
        what = "S %d tile %r radius %g" % (S, tile, radius)
        want = syn_want(SR, syn_per_set(REFS, AO, SYN, ugrt, S, K, radius), tile)
        got = _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, radius, torch)
        np.testing.assert_array_equal(got, want, err_msg=what)
        assert not got[oactive == 0].any() and (S == 32 or not (got >> np.uint32(S)).any())
        assert int((got != 0).sum()) >= 31
        by_hemi = np.stack([_hemi(ctx, grid, dv, df, d_orays, d_oactive, table[j], radius, torch) for j in range(K)])
        np.testing.assert_array_equal(got, syn_want(SR, by_hemi, tile), err_msg=what)
        if K == 1:
            np.testing.assert_array_equal(got, by_hemi[0], err_msg=what)
        if radius != SYN_RADII[1]:
            continue
        by_ray = np.zeros((K, SYN_N), np.uint32)
        for j in range(K):
            for s in range(S):
                occ = torch.full((SYN_N,), -7, dtype=torch.int32, device=ctx.device)
                rays = AO.expand(orays, oactive, table[j, s], 0, SYN_N, SYN_N)
                ctx.trace_dda_any(grid[0], grid[1], grid[2], dv, df, ctx.upload(rays), d_oactive, radius, occ)
                by_ray[j] |= occ.cpu().numpy().astype(np.uint32) << np.uint32(s)
        np.testing.assert_array_equal(got, syn_want(SR, by_ray, tile), err_msg=what)


@pytest.mark.gpu
def test_launch_shapes_change_no_word(ugrt, O, REFS, AO, SR, SYN, torch):
    """any_rays_per_wave 1, 7, 32, 64 x any_coop 1, 8, 2^30, dda_blocks = 1 (every later group comes from the ticket: each
    workgroup still copies the table once), a table that is not 16-byte aligned, and a band context (rows 2-5 of 8),
    whose sets are those of the full image's coordinates -- its first row is row 16, which a tile three rows high does
    not divide -- and whose other pixels keep their words."""
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = AM.syn_ambient()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    radius = SYN_RADII[1]
    for S, tile in ((8, (4, 4)), (5, (4, 4)), (32, (4, 4)), (8, (3, 2)), (8, (2, 3))):
        K = tile[0] * tile[1]
        table = syn_table(ugrt, S, K)
        per = syn_per_set(REFS, AO, SYN, ugrt, S, K, radius)
        want = syn_want(SR, per, tile)
        for rpw in (1, 7, 32, 64):
            for coop in (1, 8, 1 << 30):
                ctx.set_option("any_rays_per_wave", rpw)
                ctx.set_option("any_coop", coop)
                got = _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, radius, torch)
                np.testing.assert_array_equal(got, want, err_msg="S %d, rays per wave %d, coop %d" % (S, rpw, coop))
        ctx.set_option("any_rays_per_wave", -1)
        ctx.set_option("any_coop", -1)
        ctx.set_option("dda_blocks", 1)
        np.testing.assert_array_equal(_sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, radius, torch), want)
        ctx.set_option("dda_blocks", -1)
        # the table one float into an allocation: the copy's single-float path
        shifted = ctx.upload(np.concatenate([np.zeros(1, np.float32), table.reshape(-1)]))[1:]
        assert shifted.data_ptr() % 16 == 4
        mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda_any_hemi_sets(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, S, tile[0], tile[1], shifted, radius, mask)
        ctx.synchronize()
        np.testing.assert_array_equal(_words(mask), want)
        band, bv, bf, bgrid = RS._syn_context(ugrt, SYN, (2, 5))
        p0, n = band.p0, band.npix
        assert (p0, n) == (1024, 1536)
        got = _sets(band, bgrid, bv, bf, band.upload(orays), band.upload(oactive), table, tile, radius, torch)
        np.testing.assert_array_equal(got, syn_want(SR, per, tile, (2, 5)))
        assert (got[:p0] == 0xFFFFFFFF).all() and (got[p0 + n:] == 0xFFFFFFFF).all()
        np.testing.assert_array_equal(got[p0:p0 + n], want[p0:p0 + n])
    # (2, 3): sets taken from the band's own rows would be other words
    per = syn_per_set(REFS, AO, SYN, ugrt, 8, 6, radius)
    moved = SR.select(per, 2, 3, 64, 48)[:1536]
    assert int((moved != syn_want(SR, per, (2, 3))[1024:2560]).sum()) >= 100


@pytest.mark.gpu
def test_the_walk_leaves_the_shared_dda_state_alone(ugrt, O, REFS, AO, SR, torch):
    """hall: a ugrt_trace_dda before and after a launch over direction sets gives identical hits, and the split walks'
    figures stay what they were (test_ambient's test of the direction-major walk)."""
    c = cpu_ambient_sets(O, REFS, AO, SR, ugrt, "hall")
    a = c["a"]
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
    ctx.trace_dda_any_hemi_sets(g[0], g[1], g[2], r.d_verts, r.d_faces, ctx.upload(a["orays"]), ctx.upload(a["oactive"]),
                                S_SETS, 4, 4, ctx.upload(c["table"].reshape(-1)), c["radius"], mask)
    ctx.synchronize()
    np.testing.assert_array_equal(_words(mask), c["mask"])
    assert ctx.stats_dda_split() == before
    ht1, hid1 = level1()
    assert torch.equal(hid0, hid1) and torch.equal(ht0.view(torch.int32), ht1.view(torch.int32))
    np.testing.assert_array_equal(hid1.cpu().numpy(), a["base"]["levels"][0]["hit_id"])
    assert ctx.stats_dda_split() == before


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, REFS, AO, SR, SYN, torch):
    fresh = ugrt.Context(64, 64, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS)
    z = torch.zeros(6 * SYN_N, dtype=torch.int32, device=fresh.device)
    with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
        fresh.trace_dda_any_hemi_sets(z, z, z, z, z, z, z, 4, 2, 2, z, 1.0, z)
    assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = AM.syn_ambient()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)
    img = torch.full((3 * SYN_N,), 200, dtype=torch.uint8, device=ctx.device)
    table = syn_table(ugrt, 8, 16)
    d_table = ctx.upload(np.concatenate([table.reshape(-1), np.zeros(3 * 512, np.float32)]))
    args = [grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, 8, 4, 4, d_table, 3.0, mask]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    walk = ctx.trace_dda_any_hemi_sets
    for bad in (0, 33, -1):
        fails(walk, args[:7] + [bad] + args[8:], b"num_dirs")
    for bad in (0, 5, -1):
        fails(walk, args[:8] + [bad] + args[9:], b"set_w")
        fails(walk, args[:9] + [bad] + args[10:], b"set_h")
    for bad in (0.0, -1.0, float("nan")):
        fails(walk, args[:11] + [bad] + args[12:], b"radius")
    for h in (0, 1, 2, 3, 4, 5, 6, 10, 12):
        fails(walk, args[:h] + [None] + args[h + 1:], b"null")
    for bad in (0, 33, -1):
        fails(ctx.shade_ao_vis, [img, mask, bad], b"num_dirs")
    for h in (0, 1):
        a = [img, mask, 4]
        fails(ctx.shade_ao_vis, a[:h] + [None] + a[h + 1:], b"null")
    ctx.synchronize()
    assert (_words(mask) == 0xFFFFFFFF).all() and (img == 200).all()  # nothing was enqueued
    want = syn_want(SR, syn_per_set(REFS, AO, SYN, ugrt, 8, 16, 3.0), (4, 4))
    np.testing.assert_array_equal(_sets(ctx, grid, dv, df, d_orays, d_oactive, table, (4, 4), 3.0, torch), want)
    walk(*(args[:7] + [32, 4, 4] + args[10:]))  # 512 directions, the most a call takes, are accepted
    ctx.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [None, (2, 5)])
def test_shade_ao_vis_equals_the_checker(ugrt, ASR, torch, rows):
    """The whole frame and a band context (rows 2-5 of 8), S = 1, 5, 8 and 32: the band's bytes are the checker's, the
    other pixels keep theirs."""
    ctx = ugrt.Context(64, 64, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS, rows=rows)
    p0, n = ctx.p0, ctx.npix
    assert (p0, n) == ((0, SYN_N) if rows is None else (1024, 1536))
    rng = np.random.RandomState(9)
    h_img = rng.randint(0, 256, 3 * SYN_N).astype(np.uint8)
    h_img[3 * p0:3 * p0 + 300] = 255
    for S in (1, 5, 8, 32):
        vis = random_vis(rng, SYN_N, S)
        d_img = ctx.upload(h_img)
        ctx.shade_ao_vis(d_img, ctx.upload(vis.view(np.int32)), S)
        ctx.synchronize()
        want = ASR.shade(h_img, vis, S, p0, n)
        np.testing.assert_array_equal(d_img.cpu().numpy(), want)
        assert int((want != h_img).sum()) > 1000
        np.testing.assert_array_equal(want[:3 * p0], h_img[:3 * p0])
    # what test_shade_calls asks of every pass over a band's pixels: one bracket of its stage per call and none with
    # profiling off; a null argument refused under the export's own name
    d_img, d_vis = ctx.upload(h_img), ctx.upload(vis.view(np.int32))
    counts = lambda: {k: v[1] for k, v in ctx.prof_get().items()}  # noqa: E731
    ctx.prof_enable(True)
    ctx.prof_reset()
    assert set(counts().values()) == {0}
    for S in (1, 32):
        before = counts()
        ctx.shade_ao_vis(d_img, d_vis, S)
        assert counts() == dict(before, shade=before["shade"] + 1), S
    ctx.prof_enable(False)
    before = ctx.prof_get()
    ctx.shade_ao_vis(d_img, d_vis, 32)
    ctx.synchronize()
    assert ctx.prof_get() == before
    for bad in ([None, d_vis, 4], [d_img, None, 4], [d_img, d_vis, 0]):
        with pytest.raises(ugrt.UgrtError) as e:
            ctx.shade_ao_vis(*bad)
        assert e.value.code == ugrt.UGRT_EINVAL and str(e.value).split(": ", 1)[1].startswith("ao_shade_vis: "), str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "crash"])
def test_frames_with_sets_and_the_gather_equal_the_cpu_frames(ugrt, O, REFS, AO, AR, SR, ASR, LT, RL, torch, name):
    """Plain with shadows, reflections of depth 3 with shadows, three lights, reflections under three lights, all with
    ao=8, ao_sets=16, ao_filter=2: ao_mask is the per-pixel selection of the sets' CPU masks, ao_vis the checker's
    gather over the CPU origins and normals, the image the CPU frame's followed by the checker's shading, byte for byte;
    the frame without ao before it and the frame with the default ao=8 behind it are the CPU frames.  crash: the plain
    frame once more beside area=8, area_sets=16, area_filter=2, each gather in its own buffer."""
    rmod = RLT._rmod(ugrt)
    c = cpu_ambient_sets(O, REFS, AO, SR, ugrt, name)
    a, N, W, H = c["a"], c["N"], c["W"], c["H"]
    s = a["scene"]
    v = _f32(s["verts"]).reshape(-1, 3)
    plane = rmod.default_filter_plane(v.min(0), v.max(0))
    vis = SR.filter(c["mask"], S_SETS, a["orays"], a["oactive"], R_FRAME, 0.9, plane, W, H)
    assert int((vis[0::2] != open_of(c["mask"], S_SETS) * vis[1::2]).sum()) > 1000  # the gather does mix shares
    new = dict(ao=S_SETS, ao_radius=c["radius"], ao_sets=SETS, ao_filter=R_FRAME)
    lights = TL.lights_for(s, 3)
    for what, kw, with_lights, w_img, w_ids in AM._frames(O, REFS, LT, RL, ugrt, name):
        setup = TL.setup_for(ugrt, s, lights if with_lights else None)
        ctx, r = RD.make(ugrt, s, W, H)
        r.display(setup, **kw)
        ctx.synchronize()
        assert r.ao_mask is None and r.ao_vis is None and r._ao_set_tables == {}
        np.testing.assert_array_equal(r.image.cpu().numpy(), w_img, err_msg=what)
        r.display(setup, **new, **kw)
        ctx.synchronize()
        np.testing.assert_array_equal(_words(r.ao_mask), c["mask"], err_msg=what)
        np.testing.assert_array_equal(r.ao_active.cpu().numpy(), a["oactive"], err_msg=what)
        np.testing.assert_array_equal(bits(r.ao_rays.cpu().numpy()), bits(a["orays"]), err_msg=what)
        np.testing.assert_array_equal(_words(r.ao_vis), vis, err_msg=what)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        shaded = ASR.shade(w_img, vis, S_SETS, 0, N)
        fixed = AO.shade(w_img, c["per_set"][0], S_SETS, 0, N)
        np.testing.assert_array_equal(r.image.cpu().numpy(), shaded, err_msg=what)
        assert int((shaded != w_img).sum()) > 1000 and int((shaded != fixed).sum()) > 1000, what
        assert list(r._ao_set_tables) == [(S_SETS, SETS)] and r.area_vis is None
        r.display(setup, ao=S_SETS, ao_radius=c["radius"], **kw)
        ctx.synchronize()
        np.testing.assert_array_equal(_words(r.ao_mask), c["per_set"][0], err_msg=what)
        np.testing.assert_array_equal(r.image.cpu().numpy(), fixed, err_msg=what + ", behind a frame with sets")
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
    if name != "crash":
        return
    area = TS.cpu_sets(O, REFS, AO, AR, SR, ugrt, name)
    what, kw, w_plain, w_hard, w_ids, _ = TA._frames(O, REFS, AO, AR, None, ugrt, name)[0]
    np.testing.assert_array_equal(bits(area["a"]["orays"]), bits(a["orays"]))
    area_vis = SR.filter(area["mask"], TS.S_SETS, a["orays"], a["oactive"], TS.R_FRAME, 0.9, plane, W, H)
    setup = ugrt.FrameSetup.from_scene(s)
    ctx, r = RD.make(ugrt, s, W, H)
    r.display(setup, area=TS.S_SETS, area_radius=area["radius"], area_sets=TS.SETS, area_filter=TS.R_FRAME, **new, **kw)
    ctx.synchronize()
    np.testing.assert_array_equal(_words(r.area_mask), area["mask"])
    np.testing.assert_array_equal(_words(r.area_vis), area_vis)
    np.testing.assert_array_equal(_words(r.ao_mask), c["mask"])
    np.testing.assert_array_equal(_words(r.ao_vis), vis)
    assert r.ao_vis.data_ptr() != r.area_vis.data_ptr()
    both = ASR.shade(SR.shade(w_plain, area_vis, TS.S_SETS, 0, N), vis, S_SETS, 0, N)
    np.testing.assert_array_equal(r.image.cpu().numpy(), both)
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids)
    r.display(setup, **kw)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), w_hard)
