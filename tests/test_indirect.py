"""Indirect diffuse light: ugrt_gi_gather, ugrt_gi_filter, ugrt_gi_apply and display(gi=...).

The checker is tests/indirect_ref.c, a plain-C restatement with one loop per sample.  Its closest hit and its occlusion bit
are compared with the checkers that exist (the oracle's orc_trace_dda, oc_trace_any of tests/occlusion_ref.c) on the explicit
rays, and the kernel is compared with it exactly, and with the composition of existing kernels on the same rays.

The synthetic origins are test_ambient.syn_ambient()'s 4096 (64 x 64) extended by 4096 seeded ones (rows 64..127 of a
64 x 128 frame): with the first set alone the feasibility conditions of the section do not hold (399 pixels gather
anything, 5 samples hit a triangle that is not the first accepted one).  Half of the added origins are random points in the
layer of the wide triangles with random normals; the others are placed in front of one wide triangle on a line through a
second one of lower id that their cell lists too, with the normal that turns one of the eight local directions onto that
line: the walk accepts the farther triangle first."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import test_ambient as AM
import test_ambient_sets as TS
import test_area_light as TAL
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
from test_ambient import AO  # noqa: F401  (fixtures)
from test_area_light import AR  # noqa: F401
from test_reflect_shadows import REFS  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, bits, SIZES, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.SIZES, RD.LG, RD.UD
CALLS = ("ugrt_gi_gather", "ugrt_gi_filter", "ugrt_gi_apply")
EPS = 1e-3
INF = float("inf")
RADII = AM.SYN_RADII + (INF,)
SYN_W, SYN_H = 64, 128
SYN_N = SYN_W * SYN_H
SYN_LIGHT = (3.0, 5.0, 3.9)          # ugrt_set_light_position's
SYN_SHADOW_LIGHT = (4.0, 4.0, 3.95)  # above the wide triangles: they shadow what lies below
GI_FRAME = dict(gi=8, gi_sets=16, gi_filter=2)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class IndirectRef:
    def __init__(self, lib):
        self.lib = lib

    def expand(self, orays, oactive, S, tile, dirs, width, s, p0, n, N):
        rays = np.zeros(6 * N, np.float32)
        self.lib.gi_expand(_p(_f32(orays)), _p(_i32(oactive)), C.c_int(S), C.c_int(tile[0]), C.c_int(tile[1]),
                           _p(_f32(dirs).reshape(-1)), C.c_int(width), C.c_int(s), C.c_int(p0), C.c_int(n), _p(rays))
        return rays

    def gather(self, ugrid, verts, faces, orays, oactive, S, tile, dirs, width, radius, mat_idx, mat_list, cc, light,
               shadow_light, eps, p0, n, N, fill=0, detail=False):
        """[4N] sums; detail: also (hit_t, hit_id, occ, later), each [S, N]."""
        sums = np.full(4 * N, fill, np.uint32)
        mat_list = _f32(mat_list).reshape(-1)
        det = [np.zeros(S * N, t) for t in (np.float32, np.int32, np.int32, np.int32)] if detail else [None] * 4
        self.lib.gi_gather(_p(_f32(ugrid["ug"])), _p(_i32(ugrid["dims"])), _p(_u32(ugrid["vals"])), _p(_u32(ugrid["span"])),
                           _p(_u32(ugrid["offset"])), _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)),
                           _p(_f32(orays)), _p(_i32(oactive)), C.c_int(S), C.c_int(tile[0]), C.c_int(tile[1]),
                           _p(_f32(dirs).reshape(-1)), C.c_int(width), C.c_float(radius), _p(_i32(mat_idx)), _p(mat_list),
                           C.c_int(len(mat_list) // 6), _p(_f32(cc)), _p(_f32(light)),
                           None if shadow_light is None else _p(_f32(shadow_light)), C.c_float(eps), C.c_int(p0), C.c_int(n),
                           C.c_longlong(N), _p(sums), *[None if d is None else _p(d) for d in det])
        return (sums, [d.reshape(S, N) for d in det]) if detail else sums

    def filter(self, sums, orays, oactive, R, cos, tol, W, row0, row1, fill=0):
        acc = np.full(len(sums), fill, np.uint32)
        self.lib.gi_filter(_p(_u32(sums)), _p(_f32(orays)), _p(_i32(oactive)), C.c_int(R), C.c_float(cos), C.c_float(tol),
                           C.c_int(W), C.c_int(row0), C.c_int(row1), _p(acc))
        return acc

    def apply(self, img, acc, S, gain, ids, mat_list, p0, n):
        img = np.ascontiguousarray(img, np.uint8).copy()
        mat_list = _f32(mat_list).reshape(-1)
        self.lib.gi_apply(_p(img), _p(_u32(acc)), C.c_int(S), C.c_float(gain), _p(_i32(ids)), _p(mat_list),
                          C.c_int(len(mat_list) // 6), C.c_int(p0), C.c_int(n))
        return img


@pytest.fixture(scope="session")
def IR(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("indirect_ref") / "libindirect_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "indirect_ref.c"), "-lm"], check=True, capture_output=True)
    return IndirectRef(C.CDLL(out))


# ------------------------------------------------------------------------------------------------ the synthetic fixture


def _normals_for(u, loc):
    """Unit normals [n, 3] over which the local directions loc [n, 3] point along u [n, 3]: the fixed point of
    n = (u - x T - y B) / z, T and B the basis rule's tangents over n."""
    n = u.copy()
    for _ in range(30):
        e = np.eye(3)[np.argmin(np.abs(n), 1)]  # (the first of equal minima)
        T = np.cross(n, e)
        T /= np.sqrt((T * T).sum(1))[:, None]
        B = np.cross(n, T)
        n = (u - loc[:, :1] * T - loc[:, 1:2] * B) / loc[:, 2:]
        n /= np.sqrt((n * n).sum(1))[:, None]
    return n


def _seeded_origins(ugrt, verts, faces, grid, n=4096, seed=4242):
    r = np.random.RandomState(seed)
    wide, wide0 = verts.reshape(-1, 3, 3)[-7:-1].astype(np.float64), len(faces) - 7
    dirs = ugrt.scenes.ao_directions(8).astype(np.float64)
    ug, dims = np.asarray(grid["ug"], np.float64), grid["dims"]
    o = r.uniform([1.0, 1.0, 2.0], [7.0, 7.0, 3.9], (n, 3))
    nn = r.normal(size=(n, 3))
    nn /= np.sqrt((nn * nn).sum(1))[:, None]
    # which of the six wide triangles every cell lists
    lists = np.zeros((int(np.prod(dims)), 6), bool)
    for cell in range(len(lists)):
        ids = grid["vals"][grid["offset"][cell]:grid["offset"][cell] + grid["span"][cell]].astype(np.int64) - wide0
        lists[cell, ids[(ids >= 0) & (ids < 6)]] = True
    # candidates: b on triangle B, a on a triangle A of lower id, the origin a little in front of b on the line from a
    M = 60 * n
    pair = np.sort(np.stack([r.randint(0, 6, M), r.randint(0, 6, M)], 1), 1)
    a = (r.dirichlet([2, 2, 2], M)[:, :, None] * wide[pair[:, 0]]).sum(1)
    b = (r.dirichlet([2, 2, 2], M)[:, :, None] * wide[pair[:, 1]]).sum(1)
    u = (a - b) / np.maximum(np.sqrt(((a - b) ** 2).sum(1)), 1e-9)[:, None]
    cand = b - u * r.uniform(0.05, 0.4, M)[:, None]
    c = np.clip(np.floor((cand - ug[:3]) * ug[6:9]).astype(int), 0, np.asarray(dims) - 1)
    cell = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    ok = (pair[:, 0] != pair[:, 1]) & (cand > 0.05).all(1) & (cand < np.array([7.95, 7.95, 3.95])).all(1) \
        & (np.sqrt(((a - cand) ** 2).sum(1)) < 2.8) & lists[cell, pair[:, 0]] & lists[cell, pair[:, 1]]
    pick = np.flatnonzero(ok)[:n // 2]
    assert len(pick) == n // 2
    o[0::2] = cand[pick]
    nn[0::2] = _normals_for(u[pick], dirs[np.arange(n // 2) % 8])
    act = np.ones(n, np.int32)
    act[r.choice(n, 37, replace=False)] = 0
    return np.concatenate([o, nn], 1).astype(np.float32).reshape(-1), act


_SYN = {}


def syn(O, ugrt):
    """The synthetic scene of test_reflect_shadows with 8192 origins (64 x 128), a seeded table of four materials (an
    eighth of the triangles and two of the six wide ones carry an index out of range), a camera block and the two
    lights.  Computed once and shared: nobody writes to it."""
    if _SYN:
        return _SYN
    verts, faces, _ = RS.synthetic_scene()
    grid = O.grid_uniform(faces, verts, verts.min(0), verts.max(0), RS.SYN_DIMS)
    orays, oactive = AM.syn_ambient()
    more, more_active = _seeded_origins(ugrt, verts, faces, grid)
    nf = len(faces)
    rng = np.random.RandomState(2024)
    mat_idx = rng.randint(0, 4, nf).astype(np.int32)
    bad = rng.choice(nf, nf // 8, replace=False)
    mat_idx[bad] = rng.choice([-1, 4, 9], len(bad))
    mat_idx[-7:-1] = [0, 1, 2, 3, 4, -1]
    mat_list = rng.uniform(0.1, 0.9, (4, 6)).astype(np.float32)
    cam = O.Cam((4, 4, 14), (4, 4, 0), (0, 1, 0), 1.0, 50.0)
    _SYN.update(verts=verts, faces=faces, grid=grid, orays=np.concatenate([orays, more]),
                oactive=np.concatenate([oactive, more_active]), mat_idx=mat_idx, mat_list=mat_list, cc=cam.cc.copy(),
                light=np.float32(SYN_LIGHT), shadow_light=np.float32(SYN_SHADOW_LIGHT), sums={})
    return _SYN


def syn_sums(IR, y, S, tile, dirs, radius, shadow, p0=0, n=SYN_N, fill=0, detail=False):
    key = (S, tile, bits(_f32(dirs)).tobytes(), radius, shadow, p0, n, fill)
    if detail or key not in y["sums"]:
        out = IR.gather(y["grid"], y["verts"], y["faces"], y["orays"], y["oactive"], S, tile, dirs, SYN_W, radius, y["mat_idx"],
                        y["mat_list"], y["cc"], y["light"], y["shadow_light"] if shadow else None, EPS, p0, n, SYN_N, fill,
                        detail)
        if detail:
            return out
        y["sums"][key] = out
    return y["sums"][key]


def _table(ugrt, S, sets):
    return ugrt.scenes.ao_direction_sets(S, sets)


TILE = {1: (1, 1), 4: (2, 2), 16: (4, 4)}

# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name) and name in ugrt.PROTOTYPES
    for name in ("gi_gather", "gi_filter", "gi_apply"):
        assert callable(getattr(ugrt.Context, name))
    assert lib.ugrt_version() == 105
    assert not [n for n in CALLS if n.startswith("ugrt_shade_") or n.startswith("ugrt_trace_dda_any")]


def test_gi_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    chk = rmod.check_gi
    assert chk(0) is None
    assert chk(8) == (8, INF, 1.0, True, 1, 0, None, None)
    assert chk(np.int64(32), np.float32(2), 0, False, 16, 2, 0.9, None) == (32, 2.0, 0.0, False, 16, 2, float(np.float32(0.9)), None)
    assert chk(4, 3, 2.5, np.bool_(True), 4, 8, 1, 0) == (4, 3.0, 2.5, True, 4, 8, 1.0, 0.0)
    for bad in (-1, 33, 1.5, True, "4", None, np.float32(2)):
        with pytest.raises(ValueError):
            chk(bad)
    for bad in (0, 0.0, -1.0, float("nan"), "1", True, 1e-60):
        with pytest.raises(ValueError):
            chk(4, bad)
    for bad in (-1.0, float("nan"), "1", True, None):
        with pytest.raises(ValueError):
            chk(4, None, bad)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError):
            chk(4, None, 1.0, bad)
    for bad in (0, 2, 3, 17, 16.0, True, "4", None):
        with pytest.raises(ValueError):
            chk(4, gi_sets=bad)
    for bad in (-1, 9, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            chk(4, gi_filter=bad)
    for bad in (None, "x", True, float("nan")):
        with pytest.raises(ValueError):
            chk(4, gi_filter=2, gi_filter_cos=bad)
    for bad in (-1e-9, float("nan"), "x", True):
        with pytest.raises(ValueError):
            chk(4, gi_filter=2, gi_filter_plane=bad)
    # a value away from its default needs gi > 0
    for kw in (dict(gi_radius=1.0), dict(gi_gain=2.0), dict(gi_shadows=False), dict(gi_sets=4), dict(gi_filter=1)):
        with pytest.raises(ValueError):
            chk(0, **kw)
    # where check_area rejects
    for kw in (dict(lights=[("cam", "pos")]), dict(reflect_lights=True), dict(two_streams=True)):
        with pytest.raises(ValueError):
            chk(4, **kw)
        assert chk(0, **kw) is None
    s = RD.scene(ugrt, "hall")
    for kw in (dict(gi=33), dict(gi=True), dict(gi_sets=16), dict(gi=4, gi_radius=0.0), dict(gi=4, gi_gain=-1.0),
               dict(gi=4, gi_shadows=1), dict(gi=4, gi_filter=9), dict(gi=4, gi_sets=3), dict(gi_gain=0.5)):
        for lights in (None, TL.lights_for(s, 2)):
            r = TS._fake(ugrt)
            with pytest.raises(ValueError):
                r.display(TL.setup_for(ugrt, s, lights), **kw)
            assert r.ctx.calls == [], kw
    for setup, kw in ((TL.setup_for(ugrt, s, TL.lights_for(s, 2)), dict()),
                      (TL.setup_for(ugrt, s, TL.lights_for(s, 2)), dict(reflect=True, reflect_lights=True))):
        r = TS._fake(ugrt)
        with pytest.raises(ValueError):
            r.display(setup, gi=4, **kw)
        assert r.ctx.calls == []
    r = TS._fake(ugrt)
    r.aux = object()  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s), gi=4)
    assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    for kw in (dict(gi=4), dict(gi_sets=16), dict(gi_gain=2.0)):
        with pytest.raises(ValueError):
            br.display(TL.setup_for(ugrt, s), **kw)


def _fake(ugrt):
    r = TS._fake(ugrt)
    r.__dict__.update(gi_sum="gisum", gi_acc="giacc", _gi_set_tables={})
    r._ensure_gi_buffers = lambda gather: None
    return r


CAMERA_PASS, HARD, LEVELS, _names = TS.TA.CAMERA_PASS, TS.TA.HARD, TS.TA.LEVELS, TS.TA._names


def test_a_gi_frame_enqueues_its_calls_in_order_and_the_default_frame_none_of_them(ugrt):
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    reflect = dict(reflect=True, bounces=AM.DEPTH, reflect_shadows=True)
    new = {"gi_gather", "gi_filter", "gi_apply"}
    # the defaults, written out or not: the frame as it was, on a renderer that has none of the new attributes
    for kw in (dict(), reflect, dict(ao=4, ao_radius=1.0), dict(area=5, area_radius=0.5), dict(shade=False)):
        a, b = TS._fake(ugrt), TS._fake(ugrt)
        a.display(setup, **kw)
        b.display(setup, gi=0, gi_radius=None, gi_gain=1.0, gi_shadows=True, gi_sets=1, gi_filter=0, gi_filter_cos=0.5,
                  gi_filter_plane=3.0, **kw)
        assert _names(a) == _names(b) and not set(_names(a)) & new
        assert not [k for k in vars(a) if k.startswith("gi_") or k.startswith("_gi_")]
    plain = ["shade_simple", "shade_add_shadows"]
    for kw, gi, want in (
            (dict(), dict(gi=8), CAMERA_PASS + HARD + ["grid_build_uniform", "ao_rays", "gi_gather"] + plain + ["gi_apply"]),
            (dict(), GI_FRAME, CAMERA_PASS + HARD + ["grid_build_uniform", "ao_rays", "gi_gather"] + plain + ["gi_filter", "gi_apply"]),
            (reflect, GI_FRAME, CAMERA_PASS + HARD + ["reflect_rays", "grid_build_uniform"] + LEVELS
             + ["ao_rays", "gi_gather", "shade_reflect_depth_occluded", "shade_add_shadows", "gi_filter", "gi_apply"]),
            (dict(ao=4, ao_radius=1.0), GI_FRAME, CAMERA_PASS + HARD + ["grid_build_uniform", "ao_rays", "trace_dda_any_hemi",
                                                                       "gi_gather"] + plain + ["gi_filter", "gi_apply", "shade_ao"]),
            (dict(area=5, area_radius=0.5), dict(gi=8), CAMERA_PASS + ["grid_build_uniform", "ao_rays", "trace_dda_any_area",
                                                                      "gi_gather", "shade_simple", "shade_area", "gi_apply"]),
            (dict(shade=False), GI_FRAME, CAMERA_PASS + HARD)):
        r = _fake(ugrt)
        r.display(setup, **gi, **kw)
        assert _names(r) == want, (kw, gi, _names(r))
        if not kw.get("shade", True):
            continue
        S, sets = gi["gi"], gi.get("gi_sets", 1)
        call = {c[0]: c for c in r.ctx.calls}
        g = call["gi_gather"]
        assert g[1:8] == ("value", "span", "offset", "v", "f", "aorays", "aoact") and g[8:11] == (S,) + TILE[sets]
        assert g[11][0] == "aotable" and bits(g[11][1]).tobytes() == bits(_table(ugrt, S, sets)).tobytes()
        assert g[12] == INF and g[13:16] == ("mi", "ml", 3) and g[17:] == (1e-3, "gisum")
        lcam = RLT._rmod(ugrt).make_camera(setup.light_camera, setup.fovy, 1.0)
        np.testing.assert_array_equal(np.float32(g[16]), np.float32(lcam.worldori[:3]))
        acc = "gisum"
        if "gi_filter" in call:
            plane = RLT._rmod(ugrt).default_filter_plane(r.bbmin, r.bbmax)
            assert call["gi_filter"][1:] == ("gisum", "aorays", "aoact", 2, float(np.float32(0.9)), plane, "giacc")
            acc = "giacc"
        assert call["gi_apply"][1:] == ("img", acc, S, 1.0, "ids", "ml", 3)
        assert list(r._gi_set_tables) == [(S, sets)]
    r = _fake(ugrt)
    r.display(setup, gi=8, gi_radius=2.5, gi_gain=0.5, gi_shadows=False)
    call = {c[0]: c for c in r.ctx.calls}
    assert call["gi_gather"][12] == 2.5 and call["gi_gather"][16] is None and call["gi_apply"][4] == 0.5
    r.display(setup, gi=8)  # the table is kept
    assert list(r._gi_set_tables) == [(8, 1)]


def test_the_restatement_agrees_with_the_walks_that_exist(ugrt, O, REFS, IR):
    """S = 8, sixteen sets: the closest hit is orc_trace_dda's on the explicit rays at radius +inf and, at the finite radii,
    that hit where its t is below the radius and a miss elsewhere; the occlusion bit is oc_trace_any's on the explicit
    occlusion rays."""
    y, OC = syn(O, ugrt), REFS[1]
    S, tile, dirs = 8, (4, 4), _table(ugrt, 8, 16)
    v, f = y["verts"], y["faces"]
    oracle = []
    for s in range(S):
        rays = IR.expand(y["orays"], y["oactive"], S, tile, dirs, SYN_W, s, 0, SYN_N, SYN_N)
        ht, hid, _ = O.trace_dda(y["grid"], v, f, rays, y["oactive"], 0, SYN_N, SYN_N)
        oracle.append((rays, ht, hid))
    for radius in RADII:
        _, (g_t, g_id, g_occ, _) = syn_sums(IR, y, S, tile, dirs, radius, True, detail=True)
        for s, (rays, ht, hid) in enumerate(oracle):
            keep = (hid >= 0) & (ht < np.float32(min(radius, 3.4e38)))
            np.testing.assert_array_equal(g_id[s], np.where(keep, hid, -2), err_msg="radius %g sample %d" % (radius, s))
            np.testing.assert_array_equal(bits(g_t[s]), bits(np.where(keep, ht, np.float32(-1.0))))
            orays, oact = OC.occlusion_rays(rays, y["oactive"], g_t[s], g_id[s], v, f, y["shadow_light"], EPS, 0, SYN_N, SYN_N)
            np.testing.assert_array_equal(oact, (g_id[s] >= 0).astype(np.int32))
            occ = OC.trace_any(y["grid"], v, f, orays, oact, 1.0, 0, SYN_N, SYN_N)
            np.testing.assert_array_equal(g_occ[s], occ, err_msg="radius %g sample %d" % (radius, s))
    # without a shadow light nothing is occluded and no sum is smaller
    lit, shadowed = syn_sums(IR, y, S, tile, dirs, 3.0, False), syn_sums(IR, y, S, tile, dirs, 3.0, True)
    assert (lit >= shadowed).all() and int((lit != shadowed).sum()) > 1000


def test_synthetic_sums_are_feasible(ugrt, O, IR):
    """The conditions of section 6.10 at S = 8, radius 3.0, on the checker alone."""
    y = syn(O, ugrt)
    S = 8
    sums, (g_t, g_id, g_occ, later) = syn_sums(IR, y, S, (1, 1), _table(ugrt, S, 1), 3.0, True, detail=True)
    sums, act = sums.reshape(-1, 4), y["oactive"] != 0
    assert int(act.sum()) == 4035 + 4059 and not sums[~act].any() and (sums[act, 3] == 1).all()
    hit = g_id >= 0
    mats = np.where(hit, y["mat_idx"][np.maximum(g_id, 0)], 0)
    out_of_range = hit & ((mats < 0) | (mats >= 4))
    figures = dict(nonzero=int((sums[:, :3].sum(1) > 0).sum()), missed=int(((g_id < 0).any(0) & act).sum()),
                   later=int(later.sum()), occluded=int((g_occ[hit] == 1).sum()), lit=int((g_occ[hit] == 0).sum()),
                   out_of_range=int(out_of_range.sum()))
    sums16 = syn_sums(IR, y, S, (4, 4), _table(ugrt, S, 16), 3.0, True).reshape(-1, 4)
    figures["other_sets"] = int((sums16 != sums).any(1).sum())
    print(figures)
    assert figures["nonzero"] >= 1000 and figures["missed"] >= 1000 and figures["later"] >= 500
    assert figures["occluded"] >= 200 and figures["lit"] >= 200 and figures["out_of_range"] >= 100
    assert figures["other_sets"] >= 1000
    assert int(sums[:, :3].max()) <= S * 255


_CORNELL = {}
CORNELL_CAM = "A"


def cornell(O, IR, AO, ugrt):
    """The CPU side of the Cornell box at 128 x 128: the oracle's plain frame, {o', n} of its primary hits, the sums of
    GI_FRAME's gather, its filter and the image.  Computed once and shared: nobody writes to it."""
    if _CORNELL:
        return _CORNELL
    W = H = 128
    N = W * H
    s = ugrt.scenes.cornell()
    setup = ugrt.FrameSetup.from_scene(s, cam=CORNELL_CAM)
    want = O.frame(s, setup, W, H, light_grid=LG, all_chunks=True, shadows=True)
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    v3 = verts.reshape(-1, 3)
    ugrid = O.grid_uniform(s["faces"], s["verts"], v3.min(0), v3.max(0), UD)
    pr = want["primary"]
    cam_pos = want["cam"].worldori[:3].copy()
    orays, oactive = AO.rays(cam_pos, pr["t"], pr["dir"], pr["id"], verts, faces, EPS, 0, N, N)
    _CORNELL.update(scene=s, setup=setup, W=W, H=H, N=N, want=want, ugrid=ugrid, orays=orays, oactive=oactive)
    _CORNELL.update(cpu_gi(IR, ugrt, _CORNELL, want["image"], want["mat_ids"], want["lcam"]))
    return _CORNELL


def cpu_gi(IR, ugrt, c, image, mat_ids, lcam, S=8, sets=16, filt=2, gain=1.0, radius=INF, shadows=True):
    """GI_FRAME's three calls on the CPU, on top of a frame's image and material ids."""
    s, W, H, N = c["scene"], c["W"], c["H"], c["N"]
    rmod = RLT._rmod(ugrt)
    v3 = _f32(s["verts"]).reshape(-1, 3)
    sums = IR.gather(c["ugrid"], s["verts"], s["faces"], c["orays"], c["oactive"], S, TILE[sets], _table(ugrt, S, sets), W,
                     radius, s["matidx"], s["mat_list"], lcam.cc, c["setup"].shading_light,
                     lcam.worldori[:3].copy() if shadows else None, EPS, 0, N, N)
    acc = sums
    if filt:
        acc = IR.filter(sums, c["orays"], c["oactive"], filt, float(np.float32(0.9)),
                        rmod.default_filter_plane(v3.min(0), v3.max(0)), W, 0, H)
    return dict(sums=sums, acc=acc, image_gi=IR.apply(image, acc, S, gain, mat_ids, s["mat_list"], 0, N))


def test_cornell_walls_bleed_their_colours(ugrt, O, IR, AO):
    c = cornell(O, IR, AO, ugrt)
    N, want = c["N"], c["want"]
    hit = c["oactive"] != 0
    before, after = want["image"].reshape(N, 3).astype(int), c["image_gi"].reshape(N, 3).astype(int)
    changed = (before != after).any(1)
    white = hit & (want["mat_ids"] == 0)
    acc = c["acc"].reshape(N, 4)
    figures = dict(hit=int(hit.sum()), changed=int((changed & hit).sum()), white=int(white.sum()),
                   redder=int((white & (acc[:, 0] * 1.0 > acc[:, 1])).sum()), greener=int((white & (acc[:, 1] > acc[:, 0])).sum()))
    print(figures)
    assert (after >= before).all() and not changed[~hit].any()
    assert figures["changed"] * 4 >= figures["hit"] and figures["hit"] > 1000
    assert figures["redder"] >= 100 and figures["greener"] >= 100
    # the filter at radius 0 reproduces its input, and gain 0 changes no byte
    same = IR.filter(c["sums"], c["orays"], c["oactive"], 0, 0.9, 0.0, c["W"], 0, c["H"])
    np.testing.assert_array_equal(same, c["sums"])
    np.testing.assert_array_equal(IR.apply(want["image"], c["acc"], 8, 0.0, want["mat_ids"], c["scene"]["mat_list"], 0, N),
                                  want["image"])


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _syn_context(ugrt, y, rows=None):
    ctx = ugrt.Context(SYN_W, SYN_H, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS, rows=rows)
    dv, df = ctx.upload(y["verts"].reshape(-1)), ctx.upload(y["faces"].reshape(-1))
    ctx.grid_build_uniform(df, dv, len(y["faces"]), y["verts"].min(0), y["verts"].max(0))
    ctx.upload_camera(y["cc"])
    ctx.set_light_position(y["light"])
    dev = types.SimpleNamespace(ctx=ctx, dv=dv, df=df, grid=ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3], orays=ctx.upload(y["orays"]),
                                oactive=ctx.upload(y["oactive"]), mat_idx=ctx.upload(y["mat_idx"]),
                                mat_list=ctx.upload(y["mat_list"].reshape(-1)))
    return dev


def _gather(torch, d, y, S, tile, table, radius, shadow, dv=None, df=None, sentinel=-1):
    sums = torch.full((4 * SYN_N,), sentinel, dtype=torch.int32, device=d.ctx.device)
    d.ctx.gi_gather(d.grid[0], d.grid[1], d.grid[2], d.dv if dv is None else dv, d.df if df is None else df, d.orays, d.oactive,
                    S, tile[0], tile[1], table, radius, d.mat_idx, d.mat_list, 4, y["shadow_light"] if shadow else None, EPS, sums)
    d.ctx.synchronize()
    return _words(sums)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 8, 32])
def test_synthetic_gather(ugrt, O, IR, torch, S):
    """Lists of 1 to 129 triangles, 8094 active pixels, tiles of 1, 4 and 16 sets, four radii, with and without the shadow
    phase, through the triangle records and through the gather of vertices: the words of the checker, exactly."""
    y = syn(O, ugrt)
    d = _syn_context(ugrt, y)
    dv2, df2 = d.dv.clone(), d.df.clone()  # not the arrays the grid was built from: no triangle records
    for sets in (1, 4, 16):
        if S * sets > 512:
            continue
        dirs = _table(ugrt, S, sets)
        table = d.ctx.upload(dirs.reshape(-1))
        for radius in RADII:
            for shadow in (True, False):
                want = syn_sums(IR, y, S, TILE[sets], dirs, radius, shadow)
                what = "S %d sets %d radius %g shadow %s" % (S, sets, radius, shadow)
                got = _gather(torch, d, y, S, TILE[sets], table, radius, shadow)
                np.testing.assert_array_equal(got, want, err_msg=what)
                got = _gather(torch, d, y, S, TILE[sets], table, radius, shadow, dv2, df2)
                np.testing.assert_array_equal(got, want, err_msg=what + ", no records")
    assert int((want.reshape(-1, 4)[:, :3].sum(1) > 0).sum()) >= 100


@pytest.mark.gpu
def test_launch_shapes_and_a_band_change_no_word(ugrt, O, IR, torch):
    """any_rays_per_wave x any_coop, dda_blocks = 1 (every later group comes from the ticket), and a band context whose
    first row (16) is no multiple of the 2 x 3 tile's height: the other pixels keep their words."""
    y = syn(O, ugrt)
    d = _syn_context(ugrt, y)
    S, radius = 8, 3.0
    dirs = _table(ugrt, S, 16)
    table = d.ctx.upload(dirs.reshape(-1))
    want = syn_sums(IR, y, S, (4, 4), dirs, radius, True)
    for rpw in (1, 7, 32, 64):
        for coop in (1, 8, 1000):
            d.ctx.set_option("any_rays_per_wave", rpw)
            d.ctx.set_option("any_coop", coop)
            np.testing.assert_array_equal(_gather(torch, d, y, S, (4, 4), table, radius, True), want,
                                          err_msg="rays per wave %d, coop %d" % (rpw, coop))
    d.ctx.set_option("any_rays_per_wave", -1)
    d.ctx.set_option("any_coop", -1)
    d.ctx.set_option("dda_blocks", 1)
    np.testing.assert_array_equal(_gather(torch, d, y, S, (4, 4), table, radius, True), want)
    d.ctx.set_option("dda_blocks", -1)
    b = _syn_context(ugrt, y, (2, 5))
    p0, n = b.ctx.p0, b.ctx.npix
    assert (p0, n) == (1024, 1536) and (p0 // SYN_W) % 3
    six = np.ascontiguousarray(dirs[:6])  # a 2 x 3 tile
    for S5, tile, tab in ((8, (2, 3), six), (5, (4, 4), _table(ugrt, 5, 16))):
        for shadow in (True, False):
            got = _gather(torch, b, y, S5, tile, b.ctx.upload(tab.reshape(-1)), radius, shadow, sentinel=-7)
            w = syn_sums(IR, y, S5, tile, tab, radius, shadow, p0, n, fill=0xFFFFFFF9)
            np.testing.assert_array_equal(got, w)
            assert (got[:4 * p0] == 0xFFFFFFF9).all() and (got[4 * (p0 + n):] == 0xFFFFFFF9).all()
            np.testing.assert_array_equal(got[4 * p0:4 * (p0 + n)],
                                          syn_sums(IR, y, S5, tile, tab, radius, shadow)[4 * p0:4 * (p0 + n)])


@pytest.mark.gpu
def test_a_table_that_is_not_16_byte_aligned_changes_no_word(ugrt, O, IR, torch):
    """The copy of the direction table to LDS goes float4 by float4 where the table is 16-byte aligned and float by float
    elsewhere: the table 0, 4, 8 and 12 bytes into an allocation, with 3 S floats that leave 0, 1, 2 and 3 behind the last
    float4 (S = 4, 3, 2, 5) and with more than 64 of them (S = 32: a second round of the float-by-float loop)."""
    y = syn(O, ugrt)
    d = _syn_context(ugrt, y)
    radius = 3.0
    for S in (4, 3, 2, 5, 32):
        dirs = _table(ugrt, S, 1)
        assert (3 * S) % 4 == {4: 0, 3: 1, 2: 2, 5: 3, 32: 0}[S]
        want = syn_sums(IR, y, S, (1, 1), dirs, radius, True)
        for shift in (0, 1, 2, 3):
            room = torch.full((3 * S + 8,), float("nan"), dtype=torch.float32, device=d.ctx.device)
            base = (-room.data_ptr() // 4) % 4  # floats up to the next 16-byte boundary
            table = room[base + shift:base + shift + 3 * S]
            table.copy_(d.ctx.upload(dirs.reshape(-1)))
            assert table.data_ptr() % 16 == 4 * shift
            # first the same directions in the reverse order from an aligned table: what a launch finds in LDS is not its table
            turned = d.ctx.upload(np.ascontiguousarray(dirs[:, ::-1]).reshape(-1))
            np.testing.assert_array_equal(_gather(torch, d, y, S, (1, 1), turned, radius, True), want)
            np.testing.assert_array_equal(_gather(torch, d, y, S, (1, 1), table, radius, True), want,
                                          err_msg="S %d, %d bytes into the allocation" % (S, 4 * shift))


@pytest.mark.gpu
def test_the_gather_is_the_composition_of_the_kernels_that_exist(ugrt, O, IR, torch):
    """S = 8, radius +inf, one set: per direction the explicit rays through ugrt_trace_dda, ugrt_occlusion_rays,
    ugrt_trace_dda_any and ugrt_shade_reflect_depth_occluded at depth 1 with every material's reflect = 1 over a black
    primary hit -- that image is the level's colour bytes --, the eight images summed on the host."""
    y = syn(O, ugrt)
    d = _syn_context(ugrt, y)
    ctx, N, S = d.ctx, SYN_N, 8
    dirs = _table(ugrt, S, 1)
    got = _gather(torch, d, y, S, (1, 1), ctx.upload(dirs.reshape(-1)), INF, True).reshape(N, 4)
    i32, f32 = torch.int32, torch.float32
    reflect = ctx.upload(np.ones(4, np.float32))
    good = int(np.flatnonzero((y["mat_idx"] >= 0) & (y["mat_idx"] < 4))[0])
    zeros3, t0, cam_pos = torch.zeros(3 * N, dtype=f32, device=ctx.device), torch.zeros(N, dtype=f32, device=ctx.device), \
        torch.zeros(3, dtype=f32, device=ctx.device)
    total = np.zeros((N, 3), np.uint32)
    for s in range(S):
        rays = ctx.upload(IR.expand(y["orays"], y["oactive"], S, (1, 1), dirs, SYN_W, s, 0, N, N))
        ht, hid = torch.empty(N, dtype=f32, device=ctx.device), torch.empty(N, dtype=i32, device=ctx.device)
        ctx.trace_dda(d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, rays, d.oactive, ht, hid)
        orays, oact = torch.empty(6 * N, dtype=f32, device=ctx.device), torch.empty(N, dtype=i32, device=ctx.device)
        ctx.occlusion_rays(rays, d.oactive, ht, hid, d.dv, d.df, y["shadow_light"], EPS, orays, oact)
        occ = torch.empty(N, dtype=i32, device=ctx.device)
        ctx.trace_dda_any(d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, orays, oact, 1.0, occ)
        img = torch.zeros(3 * N, dtype=torch.uint8, device=ctx.device)
        ids = torch.full((N,), good, dtype=i32, device=ctx.device)
        ctx.shade_reflect_depth_occluded(img, zeros3, t0, zeros3, ids, cam_pos, d.mat_idx, d.mat_list, reflect, 4, d.dv, d.df, 1,
                                         rays, d.oactive, ht, hid, occ)
        ctx.synchronize()
        total += img.cpu().numpy().reshape(N, 3)
    act = y["oactive"] != 0
    np.testing.assert_array_equal(got[act, :3], total[act])
    assert (got[act, 3] == 1).all() and not got[~act].any() and int((total[act].sum(1) > 0).sum()) >= 1000


@pytest.mark.gpu
def test_filter_and_apply_equal_the_restatement(ugrt, O, IR, torch):
    """The gather over the synthetic sums at radii 0, 1, 2 and 8 (full frame and band), and gi_apply on random bytes with
    den = 0, materials out of range and bytes that saturate."""
    y = syn(O, ugrt)
    S = 8
    dirs = _table(ugrt, S, 16)
    sums = syn_sums(IR, y, S, (4, 4), dirs, 3.0, True)
    for rows in (None, (2, 5)):
        d = _syn_context(ugrt, y, rows)
        p0, n = d.ctx.p0, d.ctx.npix
        d_sums = d.ctx.upload(sums.view(np.int32))
        for R, cos, tol in ((0, 0.9, 0.0), (1, 0.9, 0.05), (2, -1.0, 100.0), (8, 0.5, 0.3)):
            acc = torch.full((4 * SYN_N,), -7, dtype=torch.int32, device=d.ctx.device)
            d.ctx.gi_filter(d_sums, d.orays, d.oactive, R, cos, tol, acc)
            d.ctx.synchronize()
            want = IR.filter(sums, y["orays"], y["oactive"], R, cos, tol, SYN_W, p0 // SYN_W, (p0 + n) // SYN_W, fill=0xFFFFFFF9)
            np.testing.assert_array_equal(_words(acc), want, err_msg="radius %d rows %s" % (R, rows))
            if R == 0:
                np.testing.assert_array_equal(want[4 * p0:4 * (p0 + n)], sums[4 * p0:4 * (p0 + n)])
    d = _syn_context(ugrt, y)
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, 3 * SYN_N).astype(np.uint8)
    img[::5] = 250                                    # saturates
    ids = rng.randint(-2, 6, SYN_N).astype(np.int32)  # -2, -1, 4, 5: out of range
    acc = IR.filter(sums, y["orays"], y["oactive"], 2, -1.0, 100.0, SYN_W, 0, SYN_H)
    acc.reshape(-1, 4)[::7, 3] = 0                    # den = 0
    for gain in (0.0, 1.0, 2.5, 40.0):
        for S_, a in ((S, acc), (S, sums), (32, acc)):
            d_img = d.ctx.upload(img)
            d.ctx.gi_apply(d_img, d.ctx.upload(a.view(np.int32)), S_, gain, d.ctx.upload(ids), d.mat_list, 4)
            d.ctx.synchronize()
            want = IR.apply(img, a, S_, gain, ids, y["mat_list"], 0, SYN_N)
            np.testing.assert_array_equal(d_img.cpu().numpy(), want, err_msg="gain %g" % gain)
            if gain == 0.0:
                np.testing.assert_array_equal(want, img)
    assert int((want == 255).sum()) > 1000 and int((want != img).sum()) > 1000


def _check_frame(ugrt, IR, torch, c, kinds):
    """kinds: (what, display keywords, CPU image, CPU material ids, light camera, a pass over the image behind gi_apply)."""
    s, W, H = c["scene"], c["W"], c["H"]
    for what, kw, w_img, w_ids, lcam, last in kinds:
        ctx, r = RD.make(ugrt, s, W, H)
        r.display(c["setup"], **kw)
        ctx.synchronize()
        off = r.image.cpu().numpy().copy()
        assert r.gi_sum is None and r.gi_acc is None
        if last is None:
            np.testing.assert_array_equal(off, w_img, err_msg=what)
        g = cpu_gi(IR, ugrt, c, w_img, w_ids, lcam)
        r.display(c["setup"], **GI_FRAME, **kw)
        ctx.synchronize()
        np.testing.assert_array_equal(r.ao_active.cpu().numpy(), c["oactive"], err_msg=what)
        np.testing.assert_array_equal(_words(r.gi_sum), g["sums"], err_msg=what)
        np.testing.assert_array_equal(_words(r.gi_acc), g["acc"], err_msg=what)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        w_gi = g["image_gi"] if last is None else last(g["image_gi"])
        np.testing.assert_array_equal(r.image.cpu().numpy(), w_gi, err_msg=what)
        assert int((w_gi != off).sum()) > 1000
        r.display(c["setup"], **kw)  # the option off, behind a gi frame on the same renderer: the frame as it was
        ctx.synchronize()
        np.testing.assert_array_equal(r.image.cpu().numpy(), off, err_msg=what + ", behind a gi frame")


@pytest.mark.gpu
def test_cornell_frames_equal_the_cpu_frames(ugrt, O, REFS, IR, AO, torch):
    """cornell 128 x 128: the plain frame, and the plain frame under ambient occlusion (which scales the indirect term
    too), with gi=8, gi_sets=16, gi_filter=2."""
    c = cornell(O, IR, AO, ugrt)
    want, N = c["want"], c["N"]
    s = c["scene"]
    v3 = _f32(s["verts"]).reshape(-1, 3)
    radius = float(np.float32(0.05 * float((v3.max(0) - v3.min(0)).max())))
    dirs = ugrt.scenes.ao_directions(8)
    mask = AM.cpu_mask(REFS[1], AO, c["ugrid"], s["verts"], s["faces"], c["orays"], c["oactive"], dirs, radius, 0, N, N)
    _check_frame(ugrt, IR, torch, c, [
        ("plain", dict(shadows=True), want["image"], want["mat_ids"], want["lcam"], None),
        ("plain, ao", dict(shadows=True, ao=8, ao_radius=radius), want["image"], want["mat_ids"], want["lcam"],
         lambda img: AO.shade(img, mask, 8, 0, N))])


@pytest.mark.gpu
def test_crash_frames_equal_the_cpu_frames(ugrt, O, REFS, IR, AO, AR, torch):
    """crash 256 x 144: the plain frame, the reflections of depth 3 with their shadows, the same under ambient occlusion,
    and the plain frame under an area light of 16 samples (its penumbra is shaded before the indirect term is added)."""
    a = AM.cpu_ambient(O, REFS, AO, ugrt, "crash")
    area = TAL.cpu_area(O, REFS, AO, AR, ugrt, "crash")
    W, H = SIZES["crash"]
    base, plain = a["base"], TL.cpu_frame(O, ugrt, "crash", W, H)
    c = dict(scene=a["scene"], setup=TL.setup_for(ugrt, a["scene"]), W=W, H=H, N=a["N"], ugrid=base["ugrid"], orays=a["orays"],
             oactive=a["oactive"])
    _check_frame(ugrt, IR, torch, c, [
        ("plain", dict(shadows=True), plain["image"], plain["mat_ids"], base["lcam"], None),
        ("reflect", dict(shadows=True, reflect=True, bounces=AM.DEPTH, reflect_shadows=True), base["image_occluded"],
         base["mat_ids_occluded"], base["lcam"], None),
        ("reflect, ao", dict(shadows=True, reflect=True, bounces=AM.DEPTH, reflect_shadows=True, ao=AM.S_FRAME,
                             ao_radius=a["radius"]), base["image_occluded"], base["mat_ids_occluded"], base["lcam"],
         lambda img: AO.shade(img, a["mask"], AM.S_FRAME, 0, a["N"])),
        ("plain, area", dict(shadows=True, area=TAL.S_FRAME, area_radius=area["radius"]),
         AR.shade(plain["image_unshadowed"], area["mask"], TAL.S_FRAME, 0, a["N"]), plain["mat_ids"], base["lcam"], None)])


PROF_STAGES = ("worklist", "trace_dda", "shade", "reflect_gen")


@pytest.mark.gpu
def test_the_calls_open_one_bracket_per_stage_and_none_with_profiling_off(ugrt, O, IR, torch):
    y = syn(O, ugrt)
    d = _syn_context(ugrt, y)
    ctx = d.ctx
    table = ctx.upload(_table(ugrt, 8, 4).reshape(-1))
    sums, acc = (torch.zeros(4 * SYN_N, dtype=torch.int32, device=ctx.device) for _ in range(2))
    img = torch.zeros(3 * SYN_N, dtype=torch.uint8, device=ctx.device)
    ids = torch.zeros(SYN_N, dtype=torch.int32, device=ctx.device)
    calls = [
        ("gi_gather", lambda: ctx.gi_gather(*d.grid, d.dv, d.df, d.orays, d.oactive, 8, 2, 2, table, 3.0, d.mat_idx, d.mat_list, 4,
                                            y["shadow_light"], EPS, sums), {"worklist": 1, "trace_dda": 1}),
        ("gi_gather, no shadow phase", lambda: ctx.gi_gather(*d.grid, d.dv, d.df, d.orays, d.oactive, 8, 2, 2, table, 3.0,
                                                             d.mat_idx, d.mat_list, 4, None, EPS, sums), {"worklist": 1, "trace_dda": 1}),
        ("gi_filter", lambda: ctx.gi_filter(sums, d.orays, d.oactive, 2, 0.9, 0.1, acc), {"shade": 1}),
        ("gi_apply", lambda: ctx.gi_apply(img, acc, 8, 1.0, ids, d.mat_list, 4), {"shade": 1})]
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
def test_the_gather_leaves_the_shared_dda_state_alone(ugrt, O, REFS, IR, AO, torch):
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
    S, dirs = 4, _table(ugrt, 4, 4)
    sums = torch.full((4 * N,), -1, dtype=torch.int32, device=ctx.device)
    base = a["base"]
    ctx.gi_gather(g[0], g[1], g[2], r.d_verts, r.d_faces, ctx.upload(a["orays"]), ctx.upload(a["oactive"]), S, 2, 2,
                  ctx.upload(dirs.reshape(-1)), a["radius"], r.d_matidx, r.d_matlist, r.num_materials, base["light"], EPS, sums)
    ctx.synchronize()
    want = IR.gather(base["ugrid"], s["verts"], s["faces"], a["orays"], a["oactive"], S, (2, 2), dirs, W, a["radius"],
                     s["matidx"], s["mat_list"], base["lcam"].cc, RD.setup_for(ugrt, s).shading_light, base["light"], EPS, 0, N, N)
    np.testing.assert_array_equal(_words(sums), want)
    assert int((want.reshape(-1, 4)[:, :3].sum(1) > 0).sum()) > 1000
    assert ctx.stats_dda_split() == before
    ht1, hid1 = level1()
    assert torch.equal(hid0, hid1) and torch.equal(ht0.view(torch.int32), ht1.view(torch.int32))
    np.testing.assert_array_equal(hid1.cpu().numpy(), base["levels"][0]["hit_id"])
    assert ctx.stats_dda_split() == before


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, IR, torch):
    y = syn(O, ugrt)
    fresh = ugrt.Context(SYN_W, SYN_H, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS)
    z = torch.zeros(6 * SYN_N, dtype=torch.int32, device=fresh.device)
    with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
        fresh.gi_gather(z, z, z, z, z, z, z, 4, 1, 1, z, 1.0, z, z, 4, None, EPS, z)
    assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    d = _syn_context(ugrt, y)
    ctx = d.ctx
    dirs = _table(ugrt, 4, 4)
    table = ctx.upload(dirs.reshape(-1))
    sums = torch.full((4 * SYN_N,), -1, dtype=torch.int32, device=ctx.device)
    acc = torch.full((4 * SYN_N,), -1, dtype=torch.int32, device=ctx.device)
    img = torch.full((3 * SYN_N,), 200, dtype=torch.uint8, device=ctx.device)
    ids = torch.zeros(SYN_N, dtype=torch.int32, device=ctx.device)
    args = [d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, d.orays, d.oactive, 4, 2, 2, table, 3.0, d.mat_idx, d.mat_list, 4,
            y["shadow_light"], EPS, sums]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    def swap(a, h, v):
        return a[:h] + [v] + a[h + 1:]

    for bad in (0, 33, -1):
        fails(ctx.gi_gather, swap(args, 7, bad), b"num_dirs")
    for bad in (0, 5):
        fails(ctx.gi_gather, swap(args, 8, bad), b"set_w")
        fails(ctx.gi_gather, swap(args, 9, bad), b"set_h")
    for bad in (0.0, -1.0, float("nan")):
        fails(ctx.gi_gather, swap(args, 11, bad), b"radius")
    fails(ctx.gi_gather, swap(args, 16, float("nan")), b"eps")
    for bad in (0, -3):
        fails(ctx.gi_gather, swap(args, 14, bad), b"num_materials")
    for h in (0, 1, 2, 3, 4, 5, 6, 10, 12, 13, 17):
        fails(ctx.gi_gather, swap(args, h, None), b"null")
    f_args = [sums, d.orays, d.oactive, 2, 0.9, 0.1, acc]
    for bad in (-1, 9):
        fails(ctx.gi_filter, swap(f_args, 3, bad), b"radius")
    for bad in (-1.0, float("nan")):
        fails(ctx.gi_filter, swap(f_args, 5, bad), b"plane_tol")
    for h in (0, 1, 2, 6):
        fails(ctx.gi_filter, swap(f_args, h, None), b"null")
    a_args = [img, acc, 4, 1.0, ids, d.mat_list, 4]
    for bad in (0, 33):
        fails(ctx.gi_apply, swap(a_args, 2, bad), b"num_dirs")
    for bad in (-0.5, float("nan")):
        fails(ctx.gi_apply, swap(a_args, 3, bad), b"gain")
    for h in (0, 1, 4, 5):
        fails(ctx.gi_apply, swap(a_args, h, None), b"null")
    ctx.synchronize()
    assert (_words(sums) == 0xFFFFFFFF).all() and (_words(acc) == 0xFFFFFFFF).all() and (img == 200).all()  # nothing ran
    want = syn_sums(IR, y, 4, (2, 2), dirs, 3.0, True)
    np.testing.assert_array_equal(_gather(torch, d, y, 4, (2, 2), table, 3.0, True), want)
