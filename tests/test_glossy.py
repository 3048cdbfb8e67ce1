"""Glossy reflections: ugrt_scene_sharpnesslist, ugrt_glossy_gather, ugrt_glossy_apply and
display(glossy=...).

The checker is tests/glossy_ref.c, a plain-C restatement with one loop per sample.  Its closest hit and its occlusion bit
are compared with the checkers that exist (the oracle's orc_trace_dda, oc_trace_any of tests/occlusion_ref.c) on its own
expanded rays, and the kernel is compared with it exactly, and with the composition of existing kernels on the same rays.
The gather over the sums is ugrt_gi_filter, whose checker is test_indirect's.

The synthetic fixture is test_indirect.syn()'s scene and {o', n} at 64 x 128 with, per pixel, a seeded mirror direction R in
n's upper half-space (length 0.5 to 2, a quarter of them within 0.1 rad of the surface: their lobes cross the horizon), a
seeded primary triangle and a reflect list that activates about half of the pixels."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import test_ambient as AM
import test_ambient_sets as TS
import test_indirect as TI
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
from test_ambient import AO  # noqa: F401  (fixtures)
from test_indirect import IR  # noqa: F401
from test_reflect_shadows import REFS  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, bits, SIZES, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.SIZES, RD.LG, RD.UD
_u32 = TI._u32
CALLS = ("ugrt_scene_sharpnesslist", "ugrt_glossy_gather", "ugrt_glossy_apply")
EPS = 1e-3
INF = float("inf")
RADII = AM.SYN_RADII + (INF,)
SYN_W, SYN_H, SYN_N = TI.SYN_W, TI.SYN_H, TI.SYN_N
TILE = TI.TILE
SPREADS = np.float32([0.0, 0.05, 0.3, 1.0])
ODD_SPREADS = np.float32([np.nan, -1.0, -0.0, 7.0])   # count as 0, 0, 0 and UGRT_MAX_GLOSSY_SPREAD
ODD_AS = np.float32([0.0, 0.0, 0.0, 1.0])
GLOSSY_FRAME = dict(glossy=8, glossy_sets=16, glossy_filter=2)


class GlossyRef:
    def __init__(self, lib):
        self.lib = lib

    def expand(self, rays, active, orays, ids, mat_idx, spread, S, tile, points, width, s, p0, n, N):
        out = np.zeros(6 * N, np.float32)
        spread = _f32(spread)
        self.lib.glossy_expand(_p(_f32(rays)), _p(_i32(active)), _p(_f32(orays)), _p(_i32(ids)), _p(_i32(mat_idx)), _p(spread),
                               C.c_int(len(spread)), C.c_int(S), C.c_int(tile[0]), C.c_int(tile[1]), _p(_f32(points).reshape(-1)),
                               C.c_int(width), C.c_int(s), C.c_int(p0), C.c_int(n), _p(out))
        return out

    def gather(self, ugrid, verts, faces, rays, active, orays, ids, mat_idx, spread, S, tile, points, width, radius, mat_list,
               cc, light, shadow_light, eps, p0, n, N, fill=0, detail=False):
        """[4N] sums; detail: also (hit_t, hit_id, occ, mirrored), each [S, N]."""
        sums = np.full(4 * N, fill, np.uint32)
        mat_list = _f32(mat_list).reshape(-1)
        det = [np.zeros(S * N, t) for t in (np.float32, np.int32, np.int32, np.int32)] if detail else [None] * 4
        self.lib.glossy_gather(_p(_f32(ugrid["ug"])), _p(_i32(ugrid["dims"])), _p(_u32(ugrid["vals"])), _p(_u32(ugrid["span"])),
                               _p(_u32(ugrid["offset"])), _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)),
                               _p(_f32(rays)), _p(_i32(active)), _p(_f32(orays)), _p(_i32(ids)), _p(_i32(mat_idx)),
                               _p(_f32(spread)), C.c_int(S), C.c_int(tile[0]), C.c_int(tile[1]), _p(_f32(points).reshape(-1)),
                               C.c_int(width), C.c_float(radius), _p(mat_list), C.c_int(len(mat_list) // 6), _p(_f32(cc)),
                               _p(_f32(light)), None if shadow_light is None else _p(_f32(shadow_light)), C.c_float(eps),
                               C.c_int(p0), C.c_int(n), C.c_longlong(N), _p(sums), *[None if d is None else _p(d) for d in det])
        return (sums, [d.reshape(S, N) for d in det]) if detail else sums

    def apply(self, img, acc, S, ids, reflect, p0, n):
        img = np.ascontiguousarray(img, np.uint8).copy()
        reflect = _f32(reflect)
        self.lib.glossy_apply(_p(img), _p(_u32(acc)), C.c_int(S), _p(_i32(ids)), _p(reflect), C.c_int(len(reflect)), C.c_int(p0),
                              C.c_int(n))
        return img


@pytest.fixture(scope="session")
def GL(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("glossy_ref") / "libglossy_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "glossy_ref.c"), "-lm"], check=True, capture_output=True)
    return GlossyRef(C.CDLL(out))


# ------------------------------------------------------------------------------------------------ the synthetic fixture

_GSYN = {}
SYN_REFLECT = np.float32([0.5, 0.0, 0.8, 0.0])  # materials 0 and 2 reflect: about half of the pixels carry a lobe


def gsyn(O, ugrt):
    """test_indirect.syn() with the lobe's inputs.  The mirror directions: a quarter of the pixels get a random one within
    0.1 rad of the surface; the others aim at a seeded point of one of the six wide triangles where that lies more than
    0.1 rad above the surface (random directions almost never meet a triangle of this scene), and get a random one above
    0.1 rad elsewhere.  The flags: the reflect list's pixels, and every fifth of the other pixels with an origin -- the gather
    takes the flags as given --, so that all four spreads, pixels without a primary triangle and pixels whose material is
    out of range carry a lobe.  Computed once and shared: nobody writes to it."""
    if _GSYN:
        return _GSYN
    y = TI.syn(O, ugrt)
    rng = np.random.RandomState(613)
    o = y["orays"].reshape(-1, 6)[:, :3].astype(np.float64)
    n = y["orays"].reshape(-1, 6)[:, 3:].astype(np.float64)
    e = np.eye(3)[np.argmin(np.abs(n), 1)]
    T = np.cross(n, e)
    T /= np.maximum(np.sqrt((T * T).sum(1)), 1e-30)[:, None]
    B = np.cross(n, T)
    phi = rng.uniform(0, 2 * np.pi, SYN_N)
    low = rng.uniform(size=SYN_N) < 0.25
    el = np.where(low, rng.uniform(0.0, 0.1, SYN_N), rng.uniform(0.1, np.pi / 2, SYN_N))
    R = (np.cos(el) * np.cos(phi))[:, None] * T + (np.cos(el) * np.sin(phi))[:, None] * B + np.sin(el)[:, None] * n
    wide = y["verts"].reshape(-1, 3, 3)[-7:-1].astype(np.float64)
    first = rng.randint(0, 6, SYN_N)
    todo = ~low
    for turn in range(6):  # the first of the six, from a seeded one on, with a seeded point high enough above the surface
        aim = (rng.dirichlet([2, 2, 2], SYN_N)[:, :, None] * wide[(first + turn) % 6]).sum(1) - o
        aim /= np.maximum(np.sqrt((aim * aim).sum(1)), 1e-30)[:, None]
        aimed = todo & ((aim * n).sum(1) > np.sin(0.1))
        R[aimed] = aim[aimed]
        todo &= ~aimed
    R *= rng.uniform(0.5, 2.0, SYN_N)[:, None]
    rays = np.concatenate([o, R], 1).astype(np.float32).reshape(-1)
    nf = len(y["faces"])
    # the primary triangles: seeded among those of a seeded material, the wide lobes' materials (2 and 3) more often
    by_material = [np.flatnonzero(y["mat_idx"] == k) for k in range(4)] + [np.flatnonzero((y["mat_idx"] < 0) | (y["mat_idx"] > 3))]
    which = rng.choice(5, SYN_N, p=[0.15, 0.15, 0.35, 0.25, 0.10])
    ids = np.asarray([by_material[k][j % len(by_material[k])] for k, j in zip(which, rng.randint(0, nf, SYN_N))], np.int32)
    ids[rng.choice(SYN_N, SYN_N // 16, replace=False)] = rng.choice([-1, -2], SYN_N // 16)
    m = np.where(ids >= 0, y["mat_idx"][np.maximum(ids, 0)], -1)
    ok = (m >= 0) & (m < 4)
    active = ((y["oactive"] != 0) & ok & (SYN_REFLECT[np.clip(m, 0, 3)] > 0)).astype(np.int32)
    others = np.flatnonzero((y["oactive"] != 0) & (active == 0))
    active[others[::5]] = 1
    _GSYN.update(y=y, rays=rays, ids=ids, active=active, material=m, sums={})
    return _GSYN


def _points(ugrt, S, sets):
    return ugrt.scenes.glossy_point_sets(S, sets)


def syn_sums(GL, z, S, tile, points, radius, shadow, spread=SPREADS, p0=0, n=SYN_N, fill=0, detail=False):
    y = z["y"]
    key = (S, tile, bits(_f32(points)).tobytes(), radius, shadow, bits(_f32(spread)).tobytes(), p0, n, fill)
    if detail or key not in z["sums"]:
        out = GL.gather(y["grid"], y["verts"], y["faces"], z["rays"], z["active"], y["orays"], z["ids"], y["mat_idx"], spread, S,
                        tile, points, SYN_W, radius, y["mat_list"], y["cc"], y["light"], y["shadow_light"] if shadow else None,
                        EPS, p0, n, SYN_N, fill, detail)
        if detail:
            return out
        z["sums"][key] = out
    return z["sums"][key]


def _expand(GL, z, S, tile, points, s, spread=SPREADS):
    y = z["y"]
    return GL.expand(z["rays"], z["active"], y["orays"], z["ids"], y["mat_idx"], spread, S, tile, points, SYN_W, s, 0, SYN_N,
                     SYN_N)


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name) and name in ugrt.PROTOTYPES
    for name in ("glossy_gather", "glossy_apply"):
        assert callable(getattr(ugrt.Context, name))
    assert lib.ugrt_version() == 105
    assert not [n for n in CALLS if n.startswith("ugrt_shade_") or n.startswith("ugrt_trace_dda_any")]
    header = open(os.path.join(RD.ROOT, "include", "ugrt.h")).read()
    assert "#define UGRT_MAX_GLOSSY_SAMPLES 32" in header and "#define UGRT_MAX_GLOSSY_SPREAD 1.0f" in header
    assert (ugrt.MAX_GLOSSY_SAMPLES, ugrt.MAX_GLOSSY_SPREAD) == (32, 1.0)
    for name in CALLS:
        assert name + "(" in header


def test_the_loader_reads_the_sharpness_and_a_cache_reports_mirrors(ugrt, tmp_path):
    s = ugrt.scenes.glossy(str(tmp_path / "glossy"), scale=0.1)
    m = ugrt.Model()
    m.some_material(s["mat"])
    m.load_model(s["obj"])
    np.testing.assert_array_equal(m.h_sharpnesslist, s["sharpness"])
    np.testing.assert_array_equal(m.h_sharpnesslist, np.float32([1000, 700, 300, 98, 98, 98, 98, 98]))
    np.testing.assert_array_equal(m.h_reflectlist, s["reflect"])
    np.testing.assert_array_equal(ugrt.scenes.spread_from_sharpness(m.h_sharpnesslist), s["spread"])
    assert s["spread"][0] == 0 and s["reflect"][0] == s["reflect"][1] == s["reflect"][2] == np.float32(0.6)
    assert (s["mat_list"][0] == s["mat_list"][1]).all() and (s["mat_list"][0] == s["mat_list"][2]).all()
    cache = str(tmp_path / "glossy.cache")
    m.save_cache(cache)
    again = ugrt.Model()
    again.load_cache(cache)
    np.testing.assert_array_equal(again.h_sharpnesslist, np.full(8, 1000, np.float32))
    np.testing.assert_array_equal(again.h_reflectlist, s["reflect"])
    c = ugrt.scenes.cornell(str(tmp_path / "cornell"))
    m = ugrt.Model()
    m.load_model(c["obj"])
    np.testing.assert_array_equal(m.h_sharpnesslist, np.full(len(c["materials"]), 98, np.float32))
    # with sharpness=None the text is what it was: no line names it
    assert "sharpness" not in open(c["mtl"]).read() and open(s["mtl"]).read().count("sharpness") == 3


def test_spreads_and_points(ugrt):
    f = ugrt.scenes.spread_from_sharpness
    for sh, want in ((0, 0.5), (98, 0.5 * (1 - 0.098) ** 2), (700, 0.5 * 0.3 ** 2), (1000, 0.0), (-5, 0.5), (-1e30, 0.5),
                     (1000.5, 0.0), (1e30, 0.0)):
        got = f(sh)
        assert got.dtype == np.float32 and got == np.float32(0.5 * (1.0 - min(max(float(sh), 0.0), 1000.0) / 1000.0) ** 2)
        assert abs(float(got) - want) < 1e-7
    arr = f(np.linspace(-100, 1100, 241))
    assert arr.dtype == np.float32 and not np.isnan(arr).any() and arr.max() == np.float32(0.5) and arr.min() == 0
    assert (np.diff(arr) <= 0).all()
    for S in (1, 5, 8, 32):
        pts = ugrt.scenes.glossy_points(S)
        assert pts.dtype == np.float32 and pts.shape == (S, 2) and pts.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(bits(pts), bits(np.ascontiguousarray(ugrt.scenes.ao_directions(S)[:, :2])))
        for sets in (1, 4, 16):
            t = ugrt.scenes.glossy_point_sets(S, sets)
            assert t.dtype == np.float32 and t.shape == (sets, S, 2) and t.flags["C_CONTIGUOUS"]
            np.testing.assert_array_equal(bits(t[0]), bits(pts))
            np.testing.assert_array_equal(bits(t), bits(np.ascontiguousarray(ugrt.scenes.ao_direction_sets(S, sets)[:, :, :2])))
            assert ((t.astype(np.float64) ** 2).sum(2) < 1.0).all()
    with pytest.raises(ValueError):
        ugrt.scenes.glossy_point_sets(8, 3)


def _fake(ugrt):
    r = TI._fake(ugrt)
    r.__dict__.update(glossy_sum="glsum", glossy_acc="glacc", _glossy_tables={}, d_spread="spread")
    r._ensure_glossy_buffers = lambda gather: None
    r._upload_glossy_points = lambda table: ("gltable", table)
    return r


def test_glossy_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    chk = rmod.check_glossy
    assert chk(0) is None
    assert chk(8) == (8, INF, True, 1, 0, None, None)
    assert chk(np.int64(32), 16, 2, 0.9, None, np.float32(2), False) == (32, 2.0, False, 16, 2, float(np.float32(0.9)), None)
    assert chk(4, 4, 8, 1, 0, 3, np.bool_(True)) == (4, 3.0, True, 4, 8, 1.0, 0.0)
    for bad in (-1, 33, 1.5, True, "4", None, np.float32(2)):
        with pytest.raises(ValueError):
            chk(bad)
    for bad in (0, 2, 3, 17, 16.0, True, "4", None):
        with pytest.raises(ValueError):
            chk(4, glossy_sets=bad)
    for bad in (-1, 9, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            chk(4, glossy_filter=bad)
    for bad in (None, "x", True, float("nan")):
        with pytest.raises(ValueError):
            chk(4, glossy_filter=2, glossy_filter_cos=bad)
    for bad in (-1e-9, float("nan"), "x", True):
        with pytest.raises(ValueError):
            chk(4, glossy_filter=2, glossy_filter_plane=bad)
    for bad in (0, 0.0, -1.0, float("nan"), "1", True, 1e-60):
        with pytest.raises(ValueError):
            chk(4, glossy_radius=bad)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError):
            chk(4, glossy_shadows=bad)
    # a value away from its default needs glossy > 0
    for kw in (dict(glossy_sets=4), dict(glossy_filter=1), dict(glossy_radius=1.0), dict(glossy_shadows=False)):
        with pytest.raises(ValueError):
            chk(0, **kw)
    # the frames that stay open; with glossy = 0 they are what they were
    for kw in (dict(reflect=True), dict(reflect=True, refract=True), dict(aa=4), dict(temporal=4), dict(lights=[("cam", "pos")]),
               dict(reflect_lights=True), dict(two_streams=True)):
        with pytest.raises(ValueError):
            chk(4, **kw)
        assert chk(0, **kw) is None
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    for kw in (dict(glossy=33), dict(glossy=True), dict(glossy_sets=16), dict(glossy=4, glossy_sets=3), dict(glossy=4, glossy_filter=9),
               dict(glossy=4, glossy_radius=0.0), dict(glossy=4, glossy_shadows=1), dict(glossy_radius=2.0),
               dict(glossy=4, reflect=True), dict(glossy=4, reflect=True, refract=True), dict(glossy=4, aa=4),
               dict(glossy=4, ao=4, ao_radius=1.0, temporal=4), dict(glossy=4, reflect=True, bounces=3, reflect_shadows=True)):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(setup, **kw)
        assert r.ctx.calls == [], kw
    for lights_setup, kw in ((TL.setup_for(ugrt, s, TL.lights_for(s, 2)), dict()),
                             (TL.setup_for(ugrt, s, TL.lights_for(s, 2)), dict(reflect=True, reflect_lights=True))):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(lights_setup, glossy=4, **kw)
        assert r.ctx.calls == []
    r = _fake(ugrt)
    r.aux = object()  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(setup, glossy=4)
    assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    for kw in (dict(glossy=4), dict(glossy=4, reflect=False), dict(glossy_sets=16), dict(glossy_shadows=False)):
        with pytest.raises(ValueError):
            br.display(setup, **kw)


CAMERA_PASS, HARD, _names = TS.TA.CAMERA_PASS, TS.TA.HARD, TS.TA._names


def test_a_glossy_frame_enqueues_its_calls_in_order_and_the_default_frame_none_of_them(ugrt):
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    reflect = dict(reflect=True, bounces=AM.DEPTH, reflect_shadows=True)
    new = {"glossy_gather", "glossy_apply"}
    # the defaults, written out or not: the frame as it was, on a renderer that has none of the new attributes
    for kw in (dict(), reflect, dict(ao=4, ao_radius=1.0), dict(area=5, area_radius=0.5), dict(shade=False)):
        a, b = TS._fake(ugrt), TS._fake(ugrt)
        a.display(setup, **kw)
        b.display(setup, glossy=0, glossy_sets=1, glossy_filter=0, glossy_filter_cos=0.5, glossy_filter_plane=3.0,
                  glossy_radius=None, glossy_shadows=True, **kw)
        assert _names(a) == _names(b) and not set(_names(a)) & new
        assert [c[1:] for c in a.ctx.calls if c[0].startswith("shade") or c[0] == "ao_rays"] \
            == [c[1:] for c in b.ctx.calls if c[0].startswith("shade") or c[0] == "ao_rays"]
        assert not [k for k in vars(b) if "glossy" in k]
    head = CAMERA_PASS + HARD + ["reflect_rays", "grid_build_uniform", "ao_rays", "glossy_gather"]
    for kw, gl, want in (
            (dict(), dict(glossy=8), head + ["shade_simple", "glossy_apply", "shade_add_shadows"]),
            (dict(), GLOSSY_FRAME, head + ["shade_simple", "gi_filter", "glossy_apply", "shade_add_shadows"]),
            (dict(frame_cnt=2), GLOSSY_FRAME, head + ["shade_spotlight", "gi_filter", "glossy_apply", "shade_add_shadows"]),
            (dict(shadows=False), dict(glossy=8), CAMERA_PASS + head[len(CAMERA_PASS + HARD):] + ["shade_simple", "glossy_apply"]),
            (dict(ao=4, ao_radius=1.0), GLOSSY_FRAME, head + ["trace_dda_any_hemi", "shade_simple", "gi_filter", "glossy_apply",
                                                              "shade_add_shadows", "shade_ao"]),
            (dict(area=5, area_radius=0.5), dict(glossy=8), CAMERA_PASS + head[len(CAMERA_PASS + HARD):]
             + ["trace_dda_any_area", "shade_simple", "glossy_apply", "shade_area"]),
            (dict(gi=8, gi_filter=2), GLOSSY_FRAME, head + ["gi_gather", "shade_simple", "gi_filter", "glossy_apply",
                                                           "shade_add_shadows", "gi_filter", "gi_apply"]),
            (dict(shade=False), GLOSSY_FRAME, CAMERA_PASS + HARD)):
        r = _fake(ugrt)
        r.display(setup, **gl, **kw)
        assert _names(r) == want, (kw, gl, _names(r))
        if not kw.get("shade", True):
            continue
        S, sets = gl["glossy"], gl.get("glossy_sets", 1)
        calls = r.ctx.calls
        rr = [c for c in calls if c[0] == "reflect_rays"][0]
        assert rr[1:] == ("cam", "t", "d", "ids", "mi", "refl", 3, "v", "f", 1e-3, "rays1", "active1")
        g = [c for c in calls if c[0] == "glossy_gather"][0]
        assert g[1:12] == ("value", "span", "offset", "v", "f", "rays1", "active1", "aorays", "ids", "mi", "spread")
        assert g[12:15] == (S,) + TILE[sets]
        assert g[15][0] == "gltable" and bits(g[15][1]).tobytes() == bits(_points(ugrt, S, sets)).tobytes()
        assert g[16] == INF and g[17:19] == ("ml", 3) and g[20:] == (1e-3, "glsum")
        lcam = RLT._rmod(ugrt).make_camera(setup.light_camera, setup.fovy, 1.0)
        np.testing.assert_array_equal(np.float32(g[19]), np.float32(lcam.worldori[:3]))
        acc = "glsum"
        shade_at = [i for i, c in enumerate(calls) if c[0] in ("shade_simple", "shade_spotlight")][0]
        if gl.get("glossy_filter"):
            plane = RLT._rmod(ugrt).default_filter_plane(r.bbmin, r.bbmax)
            assert calls[shade_at + 1] == ("gi_filter", "glsum", "aorays", "active1", 2, float(np.float32(0.9)), plane, "glacc")
            acc, shade_at = "glacc", shade_at + 1
        assert calls[shade_at + 1] == ("glossy_apply", "img", acc, S, "ids", "refl", 3)
        assert list(r._glossy_tables) == [(S, sets)]
        assert [c[0] for c in calls].count("ao_rays") == 1
    r = _fake(ugrt)
    r.display(setup, glossy=8, glossy_radius=2.5, glossy_shadows=False)
    g = [c for c in r.ctx.calls if c[0] == "glossy_gather"][0]
    assert g[16] == 2.5 and g[19] is None
    r.display(setup, glossy=8)  # the table is kept
    assert list(r._glossy_tables) == [(8, 1)]


def test_the_restatement_agrees_with_the_walks_that_exist(ugrt, O, REFS, GL):
    """S = 8, sixteen sets: the closest hit is orc_trace_dda's on the restatement's own explicit rays at radius +inf and, at
    the finite radii, that hit where its t is below the radius and a miss elsewhere; the occlusion bit is oc_trace_any's on
    the explicit occlusion rays."""
    z, OC = gsyn(O, ugrt), REFS[1]
    y = z["y"]
    S, tile, pts = 8, (4, 4), _points(ugrt, 8, 16)
    v, f = y["verts"], y["faces"]
    oracle = []
    for s in range(S):
        rays = _expand(GL, z, S, tile, pts, s)
        assert np.isfinite(rays).all()
        ht, hid, _ = O.trace_dda(y["grid"], v, f, rays, z["active"], 0, SYN_N, SYN_N)
        oracle.append((rays, ht, hid))
    for radius in RADII:
        _, (g_t, g_id, g_occ, _) = syn_sums(GL, z, S, tile, pts, radius, True, detail=True)
        for s, (rays, ht, hid) in enumerate(oracle):
            keep = (hid >= 0) & (ht < np.float32(min(radius, 3.4e38)))
            np.testing.assert_array_equal(g_id[s], np.where(keep, hid, -2), err_msg="radius %g sample %d" % (radius, s))
            np.testing.assert_array_equal(bits(g_t[s]), bits(np.where(keep, ht, np.float32(-1.0))))
            orays, oact = OC.occlusion_rays(rays, z["active"], g_t[s], g_id[s], v, f, y["shadow_light"], EPS, 0, SYN_N, SYN_N)
            np.testing.assert_array_equal(oact, (g_id[s] >= 0).astype(np.int32))
            occ = OC.trace_any(y["grid"], v, f, orays, oact, 1.0, 0, SYN_N, SYN_N)
            np.testing.assert_array_equal(g_occ[s], occ, err_msg="radius %g sample %d" % (radius, s))
    lit, shadowed = syn_sums(GL, z, S, tile, pts, 3.0, False), syn_sums(GL, z, S, tile, pts, 3.0, True)
    assert (lit >= shadowed).all() and int((lit != shadowed).sum()) > 500


def test_the_lobe_is_what_the_section_says(ugrt, O, GL):
    """The expanded rays against a float64 statement of the section: the spread 0 gives the normalised mirror direction,
    every direction lies on or above the surface, and within atan(spread) of the mirror direction unless it was turned."""
    z = gsyn(O, ugrt)
    y = z["y"]
    S, pts = 8, _points(ugrt, 8, 1)
    act = z["active"] != 0
    R = z["rays"].reshape(-1, 6)[:, 3:].astype(np.float64)
    r = R / np.sqrt((R * R).sum(1))[:, None]
    n = y["orays"].reshape(-1, 6)[:, 3:].astype(np.float64)
    m = np.where(z["ids"] >= 0, y["mat_idx"][np.maximum(z["ids"], 0)], -1)
    a = np.where((m >= 0) & (m < 4), SPREADS[np.clip(m, 0, 3)], 0.0).astype(np.float64)
    _, (_, _, _, mirrored) = syn_sums(GL, z, S, (1, 1), pts, 3.0, False, detail=True)
    for s in range(S):
        rays = _expand(GL, z, S, (1, 1), pts, s).reshape(-1, 6)
        np.testing.assert_array_equal(rays[~act], 0)
        np.testing.assert_array_equal(rays[act, :3], z["rays"].reshape(-1, 6)[act, :3])
        D = rays[:, 3:].astype(np.float64)
        zero = act & (a == 0)
        assert np.abs(D[zero] - r[zero]).max() < 1e-6
        assert ((D[act] * n[act]).sum(1) > -1e-6).all()
        straight = act & (mirrored[s] == 0)
        cosine = (D[straight] * r[straight]).sum(1) / np.sqrt((D[straight] ** 2).sum(1))
        reach = a[straight] * np.sqrt(float((pts[0, s].astype(np.float64) ** 2).sum()))
        assert np.abs(cosine - 1.0 / np.sqrt(1.0 + reach * reach)).max() < 1e-5


FEASIBLE_RADIUS = INF


def test_synthetic_sums_are_feasible(ugrt, O, GL):
    """The conditions of section 6.13 at S = 8, radius FEASIBLE_RADIUS, on the checker alone."""
    z = gsyn(O, ugrt)
    y = z["y"]
    S = 8
    pts = _points(ugrt, S, 1)
    sums, (g_t, g_id, g_occ, mirrored) = syn_sums(GL, z, S, (1, 1), pts, FEASIBLE_RADIUS, True, detail=True)
    sums, act = sums.reshape(-1, 4), z["active"] != 0
    assert not sums[~act].any() and (sums[act, 3] == 1).all()
    hit = g_id >= 0
    mats = np.where(hit, y["mat_idx"][np.maximum(g_id, 0)], 0)
    out_of_range = hit & ((mats < 0) | (mats >= 4))
    figures = dict(active=int(act.sum()), share=float(act.sum()) / float((y["oactive"] != 0).sum()),
                   mirrored=int(mirrored.sum()), missed=int(((g_id < 0) & act[None, :]).sum()),
                   occluded=int((g_occ[hit] == 1).sum()), lit=int((g_occ[hit] == 0).sum()),
                   out_of_range=int(out_of_range.sum()), nonzero=int((sums[:, :3].sum(1) > 0).sum()))
    sums16 = syn_sums(GL, z, S, (4, 4), _points(ugrt, S, 16), FEASIBLE_RADIUS, True).reshape(-1, 4)
    figures["other_sets"] = int((sums16 != sums).any(1).sum())
    per_spread = [int((act & (z["material"] == k)).sum()) for k in range(4)]
    figures.update(per_spread=per_spread, no_triangle=int((act & (z["ids"] < 0)).sum()),
                   no_material=int((act & (z["ids"] >= 0) & ((z["material"] < 0) | (z["material"] > 3))).sum()))
    print(figures)
    assert 0.4 <= figures["share"] <= 0.6 and min(per_spread) >= 200
    assert figures["no_triangle"] >= 50 and figures["no_material"] >= 50
    assert figures["mirrored"] >= 500 and figures["lit"] >= 200 and figures["occluded"] >= 200
    assert figures["missed"] >= 1000 and figures["out_of_range"] >= 100 and figures["other_sets"] >= 1000
    assert int(sums[:, :3].max()) <= S * 255
    # the second spread table: NaN, -1 and -0.0 give the sums of spread 0, and 7.0 those of 1.0
    for shadow in (True, False):
        np.testing.assert_array_equal(syn_sums(GL, z, S, (1, 1), pts, FEASIBLE_RADIUS, shadow, ODD_SPREADS),
                                      syn_sums(GL, z, S, (1, 1), pts, FEASIBLE_RADIUS, shadow, ODD_AS))
    assert int((syn_sums(GL, z, S, (1, 1), pts, FEASIBLE_RADIUS, True, ODD_AS) != sums.reshape(-1)).sum()) > 1000
    # points outside the unit square are clamped and a NaN counts as 0
    odd = pts.copy()
    odd[0, 0], odd[0, 1], odd[0, 2] = (np.nan, 0.25), (-FEASIBLE_RADIUS, 9.0), (0.5, np.nan)
    clean = pts.copy()
    clean[0, 0], clean[0, 1], clean[0, 2] = (0.0, 0.25), (-1.0, 1.0), (0.5, 0.0)
    np.testing.assert_array_equal(syn_sums(GL, z, S, (1, 1), odd, FEASIBLE_RADIUS, True), syn_sums(GL, z, S, (1, 1), clean, FEASIBLE_RADIUS, True))


def test_cpu_apply_is_the_rounded_blend(GL):
    rng = np.random.RandomState(9)
    N, S = 4096, 8
    img = rng.randint(0, 256, 3 * N).astype(np.uint8)
    acc = np.zeros((N, 4), np.uint32)
    acc[:, :3] = rng.randint(0, S * 255 + 1, (N, 3))
    acc[:, 3] = 1
    ids = rng.randint(0, 3, N).astype(np.int32)
    reflect = np.float32([0.0, 0.25, 1.0])
    got = GL.apply(img, acc.reshape(-1), S, ids, reflect, 0, N).reshape(N, 3)
    k = reflect[ids].astype(np.float64)[:, None]
    want = (1 - k) * img.reshape(N, 3) + k * acc[:, :3] / float(S)
    assert np.abs(got - want).max() <= 0.5 + 1e-3
    np.testing.assert_array_equal(got[ids == 0], img.reshape(N, 3)[ids == 0])


# ------------------------------------------------------------------------------------------- the frames' CPU side

_SCENE = {}
GLOSSY_CAM = "ref"


def cpu_scene(O, REFS, AO, ugrt, name):
    """The CPU side of a glossy frame's inputs: the oracle's plain frame, its reflect frame of depth 1 with the reflected
    hits shadowed (level 1's rays are ugrt_reflect_rays'), {o', n} of the primary hits and the spreads.  name "glossy":
    scenes.glossy() at 128 x 128; "crash": test_reflect_depth's at 256 x 144 with seeded spreads.  Computed once and shared:
    nobody writes to it."""
    if name in _SCENE:
        return _SCENE[name]
    REF, OC = REFS
    if name == "glossy":
        s, (W, H) = ugrt.scenes.glossy(), (128, 128)
        spread = s["spread"]
    else:
        s, (W, H) = RD.scene(ugrt, name), SIZES[name]
        spread = np.float32([0.05, 0.0, 0.0, 0.0, 0.3, 0.0])
    N = W * H
    setup = ugrt.FrameSetup.from_scene(s, cam=GLOSSY_CAM)
    base = RD.cpu_frame(O, REF, s, setup, W, H, 1, lg=LG, ud=UD)
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    light = base["lcam"].worldori[:3].copy()
    lv = base["levels"][0]
    orays1, oact1 = OC.occlusion_rays(lv["rays"], lv["active"], lv["hit_t"], lv["hit_id"], verts, faces, light, EPS, 0, N, N)
    occluded = OC.trace_any(base["ugrid"], verts, faces, orays1, oact1, 1.0, 0, N, N)
    pr = base["primary"]
    cam_pos = base["cam"].worldori[:3].copy()
    mirror, _ = OC.shade_depth_occluded(base["lcam"].cc, setup.shading_light, pr["normal"], pr["t"], pr["dir"], pr["id"], cam_pos,
                                        s["matidx"], s["mat_list"], s["reflect"], verts, faces, 1, lv["rays"], lv["active"],
                                        lv["hit_t"], lv["hit_id"], occluded, 0, N, N)
    O.add_shadows(mirror, base["is_shadowed"], 0, N)
    plain = O.frame(s, setup, W, H, light_grid=LG, all_chunks=True, shadows=True)
    np.testing.assert_array_equal(plain["primary"]["id"], pr["id"])
    orays, oactive = AO.rays(cam_pos, pr["t"], pr["dir"], pr["id"], verts, faces, EPS, 0, N, N)
    _SCENE[name] = dict(scene=s, setup=setup, W=W, H=H, N=N, spread=spread, base=base, plain=plain, mirror=mirror, rays=lv["rays"],
                        active=lv["active"], orays=orays, oactive=oactive, ugrid=base["ugrid"], lcam=base["lcam"], light=light,
                        ids=pr["id"], frames={})
    return _SCENE[name]


def cpu_glossy(O, GL, IR, ugrt, c, S=8, sets=16, filt=2, radius=INF, shadows=True):
    """A glossy frame's calls on the CPU up to the shadows: (sums, acc, the image behind shade_add_shadows)."""
    key = (S, sets, filt, radius, shadows)
    if key in c["frames"]:
        return c["frames"][key]
    s, W, H, N = c["scene"], c["W"], c["H"], c["N"]
    rmod = RLT._rmod(ugrt)
    v3 = _f32(s["verts"]).reshape(-1, 3)
    sums = GL.gather(c["ugrid"], s["verts"], s["faces"], c["rays"], c["active"], c["orays"], c["ids"], s["matidx"], c["spread"], S,
                     TILE[sets], _points(ugrt, S, sets), W, radius, s["mat_list"], c["lcam"].cc, c["setup"].shading_light,
                     c["light"] if shadows else None, EPS, 0, N, N)
    acc = sums
    if filt:
        acc = IR.filter(sums, c["orays"], c["active"], filt, float(np.float32(0.9)),
                        rmod.default_filter_plane(v3.min(0), v3.max(0)), W, 0, H)
    img = GL.apply(c["plain"]["image_unshadowed"], acc, S, c["plain"]["mat_ids"], s["reflect"], 0, N)
    O.add_shadows(img, c["plain"]["is_shadowed"], 0, N)
    c["frames"][key] = dict(sums=sums, acc=acc, image=img)
    return c["frames"][key]


def test_a_rougher_strip_shows_a_softer_reflection_and_the_sharp_strip_the_mirror_frame(ugrt, O, REFS, AO, GL, IR):
    """scenes.glossy() at 128 x 128 on the restatement alone.  The reflected term (the lobe's mean byte, glossy=16, one set,
    no gather) has, within each floor strip, a mean absolute horizontal gradient that falls strictly from sharpness 1000
    to 700 to 300; and on the sharpness-1000 strip the glossy=1 frame is the oracle's reflect frame of depth 1 with
    shadowed reflections up to the normalised direction and the blend on bytes: more than 1 per byte apart on at most
    1 % of that strip's pixels."""
    c = cpu_scene(O, REFS, AO, ugrt, "glossy")
    W, H, N = c["W"], c["H"], c["N"]
    mats = c["plain"]["mat_ids"].reshape(H, W)
    lobe = c["active"].reshape(H, W) != 0
    g = cpu_glossy(O, GL, IR, ugrt, c, S=16, sets=1, filt=0)
    mean = g["sums"].reshape(H, W, 4)[:, :, :3].astype(np.float64) / 16.0
    grads, counts = [], []
    for m in (0, 1, 2):
        strip = (mats == m) & lobe
        pair = strip[:, 1:] & strip[:, :-1]
        grads.append(float(np.abs(mean[:, 1:] - mean[:, :-1])[pair].mean()))
        counts.append(int(strip.sum()))
    print(dict(gradients=grads, pixels=counts))
    assert min(counts) >= 500
    assert grads[0] > grads[1] > grads[2] > 0
    one = cpu_glossy(O, GL, IR, ugrt, c, S=1, sets=1, filt=0)
    sharp = (mats == 0).reshape(-1)
    apart = np.abs(one["image"].reshape(N, 3).astype(int) - c["mirror"].reshape(N, 3).astype(int)).max(1)
    share = float((apart[sharp] > 1).sum()) / float(sharp.sum())
    print(dict(sharp_pixels=int(sharp.sum()), apart=int((apart[sharp] > 1).sum()), share=share))
    assert share <= 0.01
    # and the reflection is there: the strip differs from the plain frame on most of its pixels
    moved = (one["image"].reshape(N, 3) != c["plain"]["image"].reshape(N, 3)).any(1)
    assert int(moved[sharp].sum()) * 2 >= int(sharp.sum())


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _syn_context(ugrt, z, rows=None):
    d = TI._syn_context(ugrt, z["y"], rows)
    d.rays, d.active, d.ids = d.ctx.upload(z["rays"]), d.ctx.upload(z["active"]), d.ctx.upload(z["ids"])
    d.spread, d.odd_spread = d.ctx.upload(SPREADS), d.ctx.upload(ODD_SPREADS)
    return d


def _gather(torch, d, z, S, tile, table, radius, shadow, dv=None, df=None, sentinel=-1, spread=None):
    sums = torch.full((4 * SYN_N,), sentinel, dtype=torch.int32, device=d.ctx.device)
    d.ctx.glossy_gather(d.grid[0], d.grid[1], d.grid[2], d.dv if dv is None else dv, d.df if df is None else df, d.rays, d.active,
                        d.orays, d.ids, d.mat_idx, d.spread if spread is None else spread, S, tile[0], tile[1], table, radius,
                        d.mat_list, 4, z["y"]["shadow_light"] if shadow else None, EPS, sums)
    d.ctx.synchronize()
    return _words(sums)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 8, 32])
def test_synthetic_gather(ugrt, O, GL, torch, S):
    """Tiles of 1, 4 and 16 sets, four radii, with and without the shadow phase, through the triangle records and through
    the gather of vertices, both spread tables: the words of the checker, exactly."""
    z = gsyn(O, ugrt)
    d = _syn_context(ugrt, z)
    dv2, df2 = d.dv.clone(), d.df.clone()  # not the arrays the grid was built from: no triangle records
    for sets in (1, 4, 16):
        pts = _points(ugrt, S, sets)
        table = d.ctx.upload(pts.reshape(-1))
        for radius in RADII:
            for shadow in (True, False):
                want = syn_sums(GL, z, S, TILE[sets], pts, radius, shadow)
                what = "S %d sets %d radius %g shadow %s" % (S, sets, radius, shadow)
                got = _gather(torch, d, z, S, TILE[sets], table, radius, shadow)
                np.testing.assert_array_equal(got, want, err_msg=what)
                got = _gather(torch, d, z, S, TILE[sets], table, radius, shadow, dv2, df2)
                np.testing.assert_array_equal(got, want, err_msg=what + ", no records")
        want = syn_sums(GL, z, S, TILE[sets], pts, 3.0, True, ODD_SPREADS)
        np.testing.assert_array_equal(_gather(torch, d, z, S, TILE[sets], table, 3.0, True, spread=d.odd_spread), want,
                                      err_msg="S %d sets %d, the odd spreads" % (S, sets))
        np.testing.assert_array_equal(want, syn_sums(GL, z, S, TILE[sets], pts, 3.0, True, ODD_AS))
    assert int((want.reshape(-1, 4)[:, :3].sum(1) > 0).sum()) >= 100


@pytest.mark.gpu
def test_launch_shapes_and_a_band_change_no_word(ugrt, O, GL, torch):
    """any_rays_per_wave x any_coop, dda_blocks = 1 (every later group comes from the ticket), and a band context whose
    first row (16) is no multiple of the 2 x 3 tile's height: the other pixels keep their words."""
    z = gsyn(O, ugrt)
    d = _syn_context(ugrt, z)
    S, radius = 8, 3.0
    pts = _points(ugrt, S, 16)
    table = d.ctx.upload(pts.reshape(-1))
    want = syn_sums(GL, z, S, (4, 4), pts, radius, True)
    for rpw in (1, 7, 32, 64):
        for coop in (1, 8, 1000):
            d.ctx.set_option("any_rays_per_wave", rpw)
            d.ctx.set_option("any_coop", coop)
            np.testing.assert_array_equal(_gather(torch, d, z, S, (4, 4), table, radius, True), want,
                                          err_msg="rays per wave %d, coop %d" % (rpw, coop))
    d.ctx.set_option("any_rays_per_wave", -1)
    d.ctx.set_option("any_coop", -1)
    d.ctx.set_option("dda_blocks", 1)
    np.testing.assert_array_equal(_gather(torch, d, z, S, (4, 4), table, radius, True), want)
    d.ctx.set_option("dda_blocks", -1)
    b = _syn_context(ugrt, z, (2, 5))
    p0, n = b.ctx.p0, b.ctx.npix
    assert (p0, n) == (1024, 1536) and (p0 // SYN_W) % 3
    six = np.ascontiguousarray(pts[:6])  # a 2 x 3 tile
    for S5, tile, tab in ((8, (2, 3), six), (5, (4, 4), _points(ugrt, 5, 16))):
        for shadow in (True, False):
            got = _gather(torch, b, z, S5, tile, b.ctx.upload(tab.reshape(-1)), radius, shadow, sentinel=-7)
            w = syn_sums(GL, z, S5, tile, tab, radius, shadow, p0=p0, n=n, fill=0xFFFFFFF9)
            np.testing.assert_array_equal(got, w)
            assert (got[:4 * p0] == 0xFFFFFFF9).all() and (got[4 * (p0 + n):] == 0xFFFFFFF9).all()
            np.testing.assert_array_equal(got[4 * p0:4 * (p0 + n)],
                                          syn_sums(GL, z, S5, tile, tab, radius, shadow)[4 * p0:4 * (p0 + n)])


@pytest.mark.gpu
def test_a_table_that_is_not_16_byte_aligned_changes_no_word(ugrt, O, GL, torch):
    """The copy of the point table to LDS goes float4 by float4 where the table is 16-byte aligned and float by float
    elsewhere: the table 0, 4, 8 and 12 bytes into an allocation.  Its 2 S set_w set_h floats leave 0 or 2 behind the last
    float4 (an even count leaves neither 1 nor 3): S = 2 and 4 and the 2 x 3 tile leave 0, S = 1, 3 and 5 leave 2; S = 5 on
    the 4 x 4 tile is 160 floats, three rounds of the float-by-float loop."""
    z = gsyn(O, ugrt)
    d = _syn_context(ugrt, z)
    radius = 3.0
    for S, tile in ((2, (1, 1)), (4, (1, 1)), (1, (1, 1)), (3, (1, 1)), (5, (1, 1)), (8, (2, 3)), (5, (4, 4))):
        pts = np.ascontiguousarray(_points(ugrt, S, 16)[:tile[0] * tile[1]])
        count = 2 * S * tile[0] * tile[1]
        assert count % 4 == (2 if tile == (1, 1) and S % 2 else 0)
        want = syn_sums(GL, z, S, tile, pts, radius, True)
        for shift in (0, 1, 2, 3):
            room = torch.full((count + 8,), float("nan"), dtype=torch.float32, device=d.ctx.device)
            base = (-room.data_ptr() // 4) % 4  # floats up to the next 16-byte boundary
            table = room[base + shift:base + shift + count]
            table.copy_(d.ctx.upload(pts.reshape(-1)))
            assert table.data_ptr() % 16 == 4 * shift
            # first the same points in the reverse order from an aligned table: what a launch finds in LDS is not its table
            turned = d.ctx.upload(np.ascontiguousarray(pts[:, ::-1]).reshape(-1))
            np.testing.assert_array_equal(_gather(torch, d, z, S, tile, turned, radius, True), want)
            np.testing.assert_array_equal(_gather(torch, d, z, S, tile, table, radius, True), want,
                                          err_msg="S %d tile %s, %d bytes into the allocation" % (S, tile, 4 * shift))


@pytest.mark.gpu
def test_the_gather_is_the_composition_of_the_kernels_that_exist(ugrt, O, GL, torch):
    """S = 8, radius +inf, one set: per sample the restatement's explicit rays through ugrt_trace_dda, ugrt_occlusion_rays,
    ugrt_trace_dda_any and ugrt_shade_reflect_depth_occluded at depth 1 with every material's reflect = 1 over a black
    primary hit -- that image is the level's colour bytes --, the eight images summed on the host."""
    z = gsyn(O, ugrt)
    y = z["y"]
    d = _syn_context(ugrt, z)
    ctx, N, S = d.ctx, SYN_N, 8
    pts = _points(ugrt, S, 1)
    got = _gather(torch, d, z, S, (1, 1), ctx.upload(pts.reshape(-1)), INF, True).reshape(N, 4)
    i32, f32 = torch.int32, torch.float32
    reflect = ctx.upload(np.ones(4, np.float32))
    good = int(np.flatnonzero((y["mat_idx"] >= 0) & (y["mat_idx"] < 4))[0])
    zeros3, t0, cam_pos = torch.zeros(3 * N, dtype=f32, device=ctx.device), torch.zeros(N, dtype=f32, device=ctx.device), \
        torch.zeros(3, dtype=f32, device=ctx.device)
    total = np.zeros((N, 3), np.uint32)
    for s in range(S):
        rays = ctx.upload(_expand(GL, z, S, (1, 1), pts, s))
        ht, hid = torch.empty(N, dtype=f32, device=ctx.device), torch.empty(N, dtype=i32, device=ctx.device)
        ctx.trace_dda(d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, rays, d.active, ht, hid)
        orays, oact = torch.empty(6 * N, dtype=f32, device=ctx.device), torch.empty(N, dtype=i32, device=ctx.device)
        ctx.occlusion_rays(rays, d.active, ht, hid, d.dv, d.df, y["shadow_light"], EPS, orays, oact)
        occ = torch.empty(N, dtype=i32, device=ctx.device)
        ctx.trace_dda_any(d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, orays, oact, 1.0, occ)
        img = torch.zeros(3 * N, dtype=torch.uint8, device=ctx.device)
        ids = torch.full((N,), good, dtype=i32, device=ctx.device)
        ctx.shade_reflect_depth_occluded(img, zeros3, t0, zeros3, ids, cam_pos, d.mat_idx, d.mat_list, reflect, 4, d.dv, d.df, 1,
                                         rays, d.active, ht, hid, occ)
        ctx.synchronize()
        total += img.cpu().numpy().reshape(N, 3)
    act = z["active"] != 0
    np.testing.assert_array_equal(got[act, :3], total[act])
    assert (got[act, 3] == 1).all() and not got[~act].any() and int((total[act].sum(1) > 0).sum()) >= 500


@pytest.mark.gpu
def test_apply_equals_the_restatement(ugrt, O, GL, IR, torch):
    """ugrt_glossy_apply on random bytes with den = 0, materials out of range, reflect 0, -1, NaN, 0.3, 1 and 2, bytes at 0
    and 255, S = 8 and 32, over the raw sums and over ugrt_gi_filter's output (on the device and from the checker), on the
    full frame and on a band."""
    z = gsyn(O, ugrt)
    y = z["y"]
    S = 8
    pts = _points(ugrt, S, 16)
    sums = syn_sums(GL, z, S, (4, 4), pts, 3.0, True)
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, 3 * SYN_N).astype(np.uint8)
    img[::5], img[1::7] = 255, 0
    ids = rng.randint(-2, 8, SYN_N).astype(np.int32)  # -2, -1, 6, 7: out of range
    reflect = np.float32([0.0, -1.0, np.nan, 0.3, 1.0, 2.0])
    for rows in (None, (2, 5)):
        d = _syn_context(ugrt, z, rows)
        p0, n = d.ctx.p0, d.ctx.npix
        acc_dev = torch.zeros(4 * SYN_N, dtype=torch.int32, device=d.ctx.device)
        d.ctx.gi_filter(d.ctx.upload(sums.view(np.int32)), d.orays, d.active, 2, -1.0, 100.0, acc_dev)
        d.ctx.synchronize()
        acc = IR.filter(sums, y["orays"], z["active"], 2, -1.0, 100.0, SYN_W, p0 // SYN_W, (p0 + n) // SYN_W)
        np.testing.assert_array_equal(_words(acc_dev)[4 * p0:4 * (p0 + n)], acc[4 * p0:4 * (p0 + n)])
        assert int((acc.reshape(-1, 4)[:, 3] > 1).sum()) > 500
        holes = acc.copy()
        holes.reshape(-1, 4)[::7, 3] = 0                    # den = 0
        for S_, a in ((S, holes), (S, sums), (32, holes), (32, acc)):
            d_img = d.ctx.upload(img)
            d.ctx.glossy_apply(d_img, d.ctx.upload(a.view(np.int32)), S_, d.ctx.upload(ids), d.ctx.upload(reflect), 6)
            d.ctx.synchronize()
            want = GL.apply(img, a, S_, ids, reflect, p0, n)
            np.testing.assert_array_equal(d_img.cpu().numpy(), want, err_msg="S %d rows %s" % (S_, rows))
            w3, i3 = want.reshape(-1, 3), img.reshape(-1, 3)
            still = (ids < 3) | (ids > 5) | (a.reshape(-1, 4)[:, 3] == 0)
            still[:p0], still[p0 + n:] = True, True
            np.testing.assert_array_equal(w3[still], i3[still])
            assert int((w3 != i3).any(1).sum()) > 200
    # reflect 1 and 2 put the mean itself there
    full = (ids >= 4) & (ids <= 5) & (sums.reshape(-1, 4)[:, 3] == 1)
    want = GL.apply(img, sums, S, ids, reflect, 0, SYN_N).reshape(-1, 3)
    np.testing.assert_array_equal(want[full], np.floor(sums.reshape(-1, 4)[full, :3] / np.float32(S) + np.float32(0.5)).astype(np.uint8))


def _make(ugrt, c):
    return RD.make(ugrt, c["scene"], c["W"], c["H"], spread=c["spread"])


def _check_frames(ugrt, O, REFS, AO, GL, IR, torch, name):
    """display(glossy=8, glossy_sets=16, glossy_filter=2) plain, under ao=8 and under gi=8: the CPU frame byte for byte, with
    glossy_sum and glossy_acc; behind each the option off gives the frame as it was; and a reflect=True frame behind them
    is that frame on a fresh renderer."""
    c = cpu_scene(O, REFS, AO, ugrt, name)
    s, W, H, N = c["scene"], c["W"], c["H"], c["N"]
    g = cpu_glossy(O, GL, IR, ugrt, c)
    v3 = _f32(s["verts"]).reshape(-1, 3)
    radius = float(np.float32(0.05 * float((v3.max(0) - v3.min(0)).max())))
    mask = AM.cpu_mask(REFS[1], AO, c["ugrid"], s["verts"], s["faces"], c["orays"], c["oactive"], ugrt.scenes.ao_directions(8),
                       radius, 0, N, N)
    gi = TI.cpu_gi(IR, ugrt, c, g["image"], c["plain"]["mat_ids"], c["lcam"], S=8, sets=1, filt=0)
    assert int((g["image"] != c["plain"]["image"]).sum()) > 1000
    ctx, r = _make(ugrt, c)
    for what, kw, want in (("plain", dict(), g["image"]),
                           ("ao", dict(ao=8, ao_radius=radius), AO.shade(g["image"], mask, 8, 0, N)),
                           ("gi", dict(gi=8), gi["image_gi"])):
        r.display(c["setup"], shadows=True, **kw)
        ctx.synchronize()
        off = r.image.cpu().numpy().copy()
        if what == "plain":
            assert r.glossy_sum is None and r.glossy_acc is None
            np.testing.assert_array_equal(off, c["plain"]["image"])
        r.display(c["setup"], shadows=True, **GLOSSY_FRAME, **kw)
        ctx.synchronize()
        np.testing.assert_array_equal(r.active.cpu().numpy(), c["active"], err_msg=what)
        np.testing.assert_array_equal(bits(r.rays.cpu().numpy()), bits(c["rays"]), err_msg=what)
        np.testing.assert_array_equal(r.ao_active.cpu().numpy(), c["oactive"], err_msg=what)
        np.testing.assert_array_equal(_words(r.glossy_sum), g["sums"], err_msg=what)
        np.testing.assert_array_equal(_words(r.glossy_acc), g["acc"], err_msg=what)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), c["plain"]["mat_ids"], err_msg=what)
        np.testing.assert_array_equal(r.image.cpu().numpy(), want, err_msg=what)
        r.display(c["setup"], shadows=True, **kw)  # the option off, behind a glossy frame on the same renderer
        ctx.synchronize()
        np.testing.assert_array_equal(r.image.cpu().numpy(), off, err_msg=what + ", behind a glossy frame")
    mirror = dict(shadows=True, reflect=True, bounces=1, reflect_shadows=True)
    r.display(c["setup"], **mirror)
    ctx.synchronize()
    ctx2, fresh = _make(ugrt, c)
    fresh.display(c["setup"], **mirror)
    ctx2.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), fresh.image.cpu().numpy())
    np.testing.assert_array_equal(r.image.cpu().numpy(), c["mirror"])


@pytest.mark.gpu
def test_glossy_scene_frames_equal_the_cpu_frames(ugrt, O, REFS, AO, GL, IR, torch):
    _check_frames(ugrt, O, REFS, AO, GL, IR, torch, "glossy")


@pytest.mark.gpu
def test_crash_frames_equal_the_cpu_frames(ugrt, O, REFS, AO, GL, IR, torch):
    _check_frames(ugrt, O, REFS, AO, GL, IR, torch, "crash")


PROF_STAGES = TI.PROF_STAGES


@pytest.mark.gpu
def test_the_calls_open_one_bracket_per_stage_and_none_with_profiling_off(ugrt, O, GL, torch):
    z = gsyn(O, ugrt)
    d = _syn_context(ugrt, z)
    ctx = d.ctx
    table = ctx.upload(_points(ugrt, 8, 4).reshape(-1))
    sums = torch.zeros(4 * SYN_N, dtype=torch.int32, device=ctx.device)
    img = torch.zeros(3 * SYN_N, dtype=torch.uint8, device=ctx.device)
    ids = torch.zeros(SYN_N, dtype=torch.int32, device=ctx.device)
    reflect = ctx.upload(SYN_REFLECT)
    light = z["y"]["shadow_light"]
    front = (d.dv, d.df, d.rays, d.active, d.orays, d.ids, d.mat_idx, d.spread, 8, 2, 2, table, 3.0, d.mat_list, 4)
    calls = [
        ("glossy_gather", lambda: ctx.glossy_gather(*d.grid, *front, light, EPS, sums), {"worklist": 1, "trace_dda": 1}),
        ("glossy_gather, no shadow phase", lambda: ctx.glossy_gather(*d.grid, *front, None, EPS, sums),
         {"worklist": 1, "trace_dda": 1}),
        ("glossy_apply", lambda: ctx.glossy_apply(img, sums, 8, ids, reflect, 4), {"shade": 1})]
    counts = lambda: {k: v[1] for k, v in ctx.prof_get().items() if k in PROF_STAGES}
    ctx.prof_enable(True, stages=PROF_STAGES)
    ctx.prof_reset()
    for name, call, adds in calls:
        before = counts()
        call()
        assert counts() == {k: before[k] + adds.get(k, 0) for k in PROF_STAGES}, name
    ctx.prof_enable(False)
    before = ctx.prof_get()
    for name, call, adds in calls:
        call()
    assert ctx.prof_get() == before


@pytest.mark.gpu
def test_the_gather_leaves_the_shared_dda_state_alone(ugrt, O, REFS, AO, GL, torch):
    """hall: a ugrt_trace_dda before and after a gather gives identical hits, and the split walks' figures stay what they
    were; the gather's words are the checker's."""
    a = AM.cpu_ambient(O, REFS, AO, ugrt, "hall")
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
    S, pts = 4, _points(ugrt, 4, 4)
    base = a["base"]
    lv = base["levels"][0]
    spread = np.float32([0.3, 0.0, 0.0, 0.0, 0.05, 0.0])
    sums = torch.full((4 * N,), -1, dtype=torch.int32, device=ctx.device)
    ctx.glossy_gather(g[0], g[1], g[2], r.d_verts, r.d_faces, r.rays, r.active, ctx.upload(a["orays"]),
                      ctx.upload(base["primary"]["id"]), r.d_matidx, ctx.upload(spread), S, 2, 2, ctx.upload(pts.reshape(-1)),
                      a["radius"], r.d_matlist, r.num_materials, base["light"], EPS, sums)
    ctx.synchronize()
    want = GL.gather(base["ugrid"], s["verts"], s["faces"], lv["rays"], lv["active"], a["orays"], base["primary"]["id"],
                     s["matidx"], spread, S, (2, 2), pts, W, a["radius"], s["mat_list"], base["lcam"].cc,
                     RD.setup_for(ugrt, s).shading_light, base["light"], EPS, 0, N, N)
    np.testing.assert_array_equal(_words(sums), want)
    assert int((want.reshape(-1, 4)[:, :3].sum(1) > 0).sum()) > 1000
    assert ctx.stats_dda_split() == before
    ht1, hid1 = level1()
    assert torch.equal(hid0, hid1) and torch.equal(ht0.view(torch.int32), ht1.view(torch.int32))
    np.testing.assert_array_equal(hid1.cpu().numpy(), base["levels"][0]["hit_id"])
    assert ctx.stats_dda_split() == before


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, GL, torch):
    z = gsyn(O, ugrt)
    fresh = ugrt.Context(SYN_W, SYN_H, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS)
    w = torch.zeros(6 * SYN_N, dtype=torch.int32, device=fresh.device)
    with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
        fresh.glossy_gather(w, w, w, w, w, w, w, w, w, w, w, 4, 1, 1, w, 1.0, w, 4, None, EPS, w)
    assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    d = _syn_context(ugrt, z)
    ctx = d.ctx
    pts = _points(ugrt, 4, 4)
    table = ctx.upload(pts.reshape(-1))
    sums = torch.full((4 * SYN_N + 4,), -1, dtype=torch.int32, device=ctx.device)
    img = torch.full((3 * SYN_N,), 200, dtype=torch.uint8, device=ctx.device)
    ids = torch.zeros(SYN_N, dtype=torch.int32, device=ctx.device)
    reflect = ctx.upload(np.ones(4, np.float32))
    args = [d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, d.rays, d.active, d.orays, d.ids, d.mat_idx, d.spread, 4, 2, 2, table, 3.0,
            d.mat_list, 4, z["y"]["shadow_light"], EPS, sums]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    def swap(a, h, v):
        return a[:h] + [v] + a[h + 1:]

    for bad in (0, 33, -1):
        fails(ctx.glossy_gather, swap(args, 11, bad), b"num_samples")
    for bad in (0, 5):
        fails(ctx.glossy_gather, swap(args, 12, bad), b"set_w")
        fails(ctx.glossy_gather, swap(args, 13, bad), b"set_h")
    for bad in (0.0, -1.0, float("nan")):
        fails(ctx.glossy_gather, swap(args, 15, bad), b"radius")
    fails(ctx.glossy_gather, swap(args, 19, float("nan")), b"eps")
    for bad in (0, -3):
        fails(ctx.glossy_gather, swap(args, 17, bad), b"num_materials")
    fails(ctx.glossy_gather, swap(args, 20, sums[1:]), b"d_sum")
    for h in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 16, 20):
        fails(ctx.glossy_gather, swap(args, h, None), b"null")
    a_args = [img, sums, 4, ids, reflect, 4]
    for bad in (0, 33):
        fails(ctx.glossy_apply, swap(a_args, 2, bad), b"num_samples")
    fails(ctx.glossy_apply, swap(a_args, 1, sums[1:]), b"d_acc")
    for h in (0, 1, 3, 4):
        fails(ctx.glossy_apply, swap(a_args, h, None), b"null")
    ctx.synchronize()
    assert (_words(sums) == 0xFFFFFFFF).all() and (img == 200).all()  # nothing ran
    want = syn_sums(GL, z, 4, (2, 2), pts, 3.0, True)
    np.testing.assert_array_equal(_gather(torch, d, z, 4, (2, 2), table, 3.0, True), want)
