"""Adaptive anti-aliasing: ugrt_aa_edges, ugrt_aa_gather, ugrt_aa_resolve and display(aa=...).

The checker is tests/aa_ref.c, a plain-C restatement with one loop per sample.  With one sample at the offset (0, 0) it is
compared with the oracle's primary pass and frame -- the hit, its t and the bytes, on every pixel -- which is what lets a
frame mix the two tracers; the kernels are compared with it exactly."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import test_ambient as AM
import test_ambient_sets as TS
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
from test_ambient import AO  # noqa: F401  (fixtures)
from test_reflect_shadows import REFS  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, bits, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.LG, RD.UD
CALLS = ("ugrt_aa_edges", "ugrt_aa_gather", "ugrt_aa_resolve")
EPS = 1e-3
COS = float(np.float32(0.9))
TILE = {1: (1, 1), 4: (2, 2), 16: (4, 4)}
SIZES = {"hall": (256, 256), "crash": (256, 144), "glass": (128, 128), "mirrors": (128, 128)}
_names = TS.TA._names
CAMERA_PASS, HARD = TS.TA.CAMERA_PASS, TS.TA.HARD


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _opt(a):
    return None if a is None else _p(a)


class AaRef:
    def __init__(self, lib):
        self.lib = lib

    def edges(self, pr, cam_pos, mat_idx, shadowed, cos, tol, W, H, p0, n, fill=0):
        edge = np.full(W * H, fill, np.int32)
        self.lib.aa_edges(_p(_f32(pr["normal"])), _p(_f32(pr["t"])), _p(_f32(pr["dir"])), _p(_i32(pr["id"])), _p(_f32(cam_pos)),
                          _p(_i32(mat_idx)), _opt(None if shadowed is None else _i32(shadowed)), C.c_float(cos), C.c_float(tol),
                          C.c_int(W), C.c_int(H), C.c_int(p0), C.c_int(n), _p(edge))
        return edge

    def gather(self, ugrid, verts, faces, cam, strict, W, H, edge, S, tile, offsets, mat_idx, mat_list, cc, light, shadow_light,
               eps, p0, n, fill=0, detail=False):
        """[4N] sums; detail: also (hit_t, hit_id), each [S, N].  cam: the eye's oracle_lib.Cam."""
        N = W * H
        sums = np.full(4 * N, fill, np.uint32)
        mat_list = _f32(mat_list).reshape(-1)
        det = [np.zeros(S * N, t) for t in (np.float32, np.int32)] if detail else [None, None]
        self.lib.aa_gather(_p(_f32(ugrid["ug"])), _p(_i32(ugrid["dims"])), _p(_u32(ugrid["vals"])), _p(_u32(ugrid["span"])),
                           _p(_u32(ugrid["offset"])), _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)), _p(_f32(cam.cc)),
                           _p(_f32(cam.tex)), C.c_int(1 if strict else 0), C.c_int(W), C.c_int(H), _p(_i32(edge)), C.c_int(S),
                           C.c_int(tile[0]), C.c_int(tile[1]), _p(_f32(offsets).reshape(-1)), _p(_i32(mat_idx)), _p(mat_list),
                           C.c_int(len(mat_list) // 6), _p(_f32(cc)), _p(_f32(light)),
                           _opt(None if shadow_light is None else _f32(shadow_light)), C.c_float(eps), C.c_int(p0), C.c_int(n),
                           C.c_longlong(N), _p(sums), *[_opt(d) for d in det])
        return (sums, [d.reshape(S, N) for d in det]) if detail else sums

    def resolve(self, img, sums, S, p0, n):
        img = np.ascontiguousarray(img, np.uint8).copy()
        self.lib.aa_resolve(_p(img), _p(_u32(sums)), C.c_int(S), C.c_int(p0), C.c_int(n))
        return img


@pytest.fixture(scope="session")
def AA(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("aa_ref") / "libaa_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "aa_ref.c"), "-lm"], check=True, capture_output=True)
    return AaRef(C.CDLL(out))


_SCENES, _FRAMES, _CPU = {}, {}, {}


def scene(ugrt, name):
    if name not in _SCENES:
        _SCENES[name] = ugrt.scenes.glass(scale=0.1) if name == "glass" else RD.scene(ugrt, name)
    return _SCENES[name]


def frame(O, ugrt, name, W, H, shadows=True, strict=False):
    """The oracle's plain frame of a scene, its uniform grid and the default plane tolerance.  Computed once per key and
    shared: nobody writes to it."""
    key = (name, W, H, shadows, strict)
    if key not in _FRAMES:
        s = scene(ugrt, name)
        setup = ugrt.FrameSetup.from_scene(s)
        want = O.frame(s, setup, W, H, light_grid=LG, all_chunks=True, shadows=shadows, strict_texture=strict)
        O.set_strict_texture(False)
        v3 = _f32(s["verts"]).reshape(-1, 3)
        lcam = want["lcam"] if shadows else O.cam_from(setup.light_camera, setup.fovy, float(np.float32(W) / np.float32(H)))
        if not shadows:
            # the renderer makes the light camera's block the current one, shadows or not (use_light_camera); the oracle's
            # frame without shadows shades under the eye's, which rounds differently: shaded again as the renderer shades
            pr = want["primary"]
            img, ids = np.zeros(3 * W * H, np.uint8), pr["id"].copy()
            O.shade(lcam.cc, setup.shading_light, img, pr["normal"], pr["t"], pr["dir"], ids, want["cam"].worldori[:3].copy(),
                    s["matidx"], s["mat_list"], 0, W * H)
            want.update(image=img, image_unshadowed=img.copy(), mat_ids=ids)
        want.update(scene=s, setup=setup, W=W, H=H, N=W * H, ugrid=O.grid_uniform(s["faces"], s["verts"], v3.min(0), v3.max(0), UD),
                    plane=RLT._rmod(ugrt).default_filter_plane(v3.min(0), v3.max(0)), cam_pos=want["cam"].worldori[:3].copy(),
                    lcam=lcam, strict=strict)
        _FRAMES[key] = want
    return _FRAMES[key]


def cpu_edges(AA, f, with_shadows, cos=COS, plane=None, p0=0, n=None, fill=0):
    s = f["scene"]
    return AA.edges(f["primary"], f["cam_pos"], s["matidx"], f["is_shadowed"] if with_shadows else None, cos,
                    f["plane"] if plane is None else plane, f["W"], f["H"], p0, f["N"] if n is None else n, fill)


def cpu_sums(AA, f, edge, S, tile, offsets, shadow, p0=0, n=None, fill=0, detail=False):
    """The checker's gather under the frame's own state: the light camera's block is the current one."""
    s = f["scene"]
    return AA.gather(f["ugrid"], s["verts"], s["faces"], f["cam"], f["strict"], f["W"], f["H"], edge, S, tile, offsets, s["matidx"],
                     s["mat_list"], f["lcam"].cc, f["setup"].shading_light, f["lcam"].worldori[:3].copy() if shadow else None, EPS,
                     p0, f["N"] if n is None else n, fill, detail)


def cpu_aa(AA, ugrt, f, S, sets, shadows, aa_shadows=True, edge=None):
    """display(aa=S, aa_sets=sets) on the CPU on top of the oracle's frame: (edge, sums, image).  Shared per key."""
    key = (id(f), S, sets, shadows, aa_shadows, None if edge is None else edge.tobytes())
    if key not in _CPU:
        use = shadows and aa_shadows
        e = cpu_edges(AA, f, use) if edge is None else edge
        sums = cpu_sums(AA, f, e, S, TILE[sets], ugrt.scenes.aa_offset_sets(S, sets), use)
        _CPU[key] = (e, sums, AA.resolve(f["image"], sums, S, 0, f["N"]))
    return _CPU[key]


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_the_header_the_library_and_the_prototypes_name_the_calls(ugrt):
    with open(os.path.join(RD.ROOT, "include", "ugrt.h")) as fh:
        header = fh.read()
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert "int %s(ugrt_ctx *ctx" % name in header and hasattr(lib, name) and name in ugrt.PROTOTYPES
    assert "#define UGRT_MAX_AA_SAMPLES 32" in header and ugrt.MAX_AA_SAMPLES == 32
    for name in ("aa_edges", "aa_gather", "aa_resolve"):
        assert callable(getattr(ugrt.Context, name))
    assert len(ugrt.PROTOTYPES["ugrt_aa_edges"][1]) == 11 and len(ugrt.PROTOTYPES["ugrt_aa_gather"][1]) == 18
    assert len(ugrt.PROTOTYPES["ugrt_aa_resolve"][1]) == 4


def test_offsets_are_stratified_and_the_sets_are_shifted_copies(ugrt):
    sc = ugrt.scenes
    np.testing.assert_array_equal(sc.aa_offsets(1), np.zeros((1, 2), np.float32))
    for S in range(1, 33):
        o = sc.aa_offsets(S)
        assert o.shape == (S, 2) and o.dtype == np.float32 and (o >= -0.5).all() and (o < 0.5).all()
        assert bits(o).tobytes() == bits(sc.aa_offsets(S)).tobytes()  # deterministic
        strata = np.floor((o.astype(np.float64) + 0.5) * S).astype(int)
        assert sorted(strata[:, 0]) == list(range(S)), S
        if S & (S - 1) == 0:
            assert sorted(strata[:, 1]) == list(range(S)), S
        for sets in (1, 4, 16):
            t = sc.aa_offset_sets(S, sets)
            assert t.shape == (sets, S, 2) and t.dtype == np.float32 and (t >= -0.5).all() and (t < 0.5).all()
            assert bits(t[0]).tobytes() == bits(o).tobytes()
            for k in range(1, sets):
                assert bits(t[k]).tobytes() != bits(o).tobytes()
                # a shift of the whole set, wrapped: the same differences modulo the pixel
                d = (t[k].astype(np.float64) - o.astype(np.float64)) % 1.0
                assert np.abs(d - d[0]).max() < 1e-6 or np.abs(np.abs(d - d[0]) - 1.0).min() < 1e-6, (S, sets, k)
    for bad in (0, 2, 3, 8, 17):
        with pytest.raises(ValueError):
            sc.aa_offset_sets(4, bad)


def _fake(ugrt):
    r = TS._fake(ugrt)
    r.__dict__.update(aa_edge="aaedge", aa_sum="aasum", _aa_set_tables={})
    r._ensure_aa_buffers = lambda: None
    return r


def test_aa_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    chk = rmod.check_aa
    assert chk(0) is None
    assert chk(4) == (4, 1, COS, None, True)
    assert chk(np.int64(32), np.int32(16), np.float32(0.5), 2, np.bool_(False)) == (32, 16, 0.5, 2.0, False)
    for bad in (-1, 33, 1.5, True, "4", None, np.float32(2)):
        with pytest.raises(ValueError):
            chk(bad)
    for bad in (0, 2, 3, 17, 16.0, True, "4", None):
        with pytest.raises(ValueError):
            chk(4, bad)
    for bad in (None, "x", True, float("nan")):
        with pytest.raises(ValueError):
            chk(4, 1, bad)
    for bad in ("x", True, float("nan")):
        with pytest.raises(ValueError):
            chk(4, 1, 0.9, bad)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError):
            chk(4, 1, 0.9, None, bad)
    # a value away from its default needs aa > 0
    for kw in (dict(aa_sets=4), dict(aa_cos=0.5), dict(aa_plane=1.0), dict(aa_shadows=False)):
        with pytest.raises(ValueError):
            chk(0, **kw)
    # the frames that stay open; with aa = 0 they are what they were
    for kw in (dict(reflect=True), dict(frame_cnt=2), dict(lights=[("cam", "pos")]), dict(area=4), dict(gi=4),
               dict(reflect_lights=True), dict(two_streams=True)):
        with pytest.raises(ValueError):
            chk(4, **kw)
        assert chk(0, **kw) is None
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    for kw in (dict(aa=33), dict(aa=True), dict(aa_sets=16), dict(aa=4, aa_sets=3), dict(aa=4, aa_cos=None), dict(aa=4, aa_shadows=1),
               dict(aa=4, reflect=True), dict(aa=4, reflect=True, bounces=3, reflect_shadows=True), dict(aa=4, reflect=True, refract=True),
               dict(aa=4, frame_cnt=2), dict(aa=4, area=4, area_radius=0.5), dict(aa=4, gi=4), dict(aa_plane=0.5)):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(setup, **kw)
        assert r.ctx.calls == [], kw
    for lights_setup, kw in ((TL.setup_for(ugrt, s, TL.lights_for(s, 2)), dict()),
                             (TL.setup_for(ugrt, s, TL.lights_for(s, 2)), dict(reflect=True, reflect_lights=True))):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(lights_setup, aa=4, **kw)
        assert r.ctx.calls == []
    r = _fake(ugrt)
    r.aux = object()  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(setup, aa=4)
    assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    for kw in (dict(aa=4), dict(aa_sets=16), dict(aa_shadows=False)):
        with pytest.raises(ValueError):
            br.display(setup, **kw)


def test_an_aa_frame_enqueues_its_calls_in_order_and_the_default_frame_none_of_them(ugrt):
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    new = {"aa_edges", "aa_gather", "aa_resolve"}
    for kw in (dict(), dict(reflect=True), dict(ao=4, ao_radius=1.0), dict(shadows=False), dict(shade=False), dict(gi=4)):
        a, b = TS._fake(ugrt), TS._fake(ugrt)
        if "gi" in kw:
            for r in (a, b):
                r.__dict__.update(gi_sum="gisum", gi_acc="giacc", _gi_set_tables={})
                r._ensure_gi_buffers = lambda gather: None
        a.display(setup, **kw)
        b.display(setup, aa=0, aa_sets=1, aa_cos=0.9, aa_plane=None, aa_shadows=True, **kw)
        assert _names(a) == _names(b) and not set(_names(a)) & new
        assert not [k for k in vars(a) if k.startswith("aa_") or k.startswith("_aa_")]
    plain = ["shade_simple", "shade_add_shadows"]
    rmod = RLT._rmod(ugrt)
    cam = rmod.make_camera(setup.camera, setup.fovy, 1.0)
    lcam = rmod.make_camera(setup.light_camera, setup.fovy, 1.0)
    for kw, aa, want in (
            (dict(), dict(aa=4), CAMERA_PASS + HARD + ["aa_edges", "grid_build_uniform", "aa_gather"] + plain + ["aa_resolve"]),
            (dict(shadows=False), dict(aa=8, aa_sets=16), CAMERA_PASS + ["aa_edges", "grid_build_uniform", "aa_gather", "shade_simple",
                                                                          "aa_resolve"]),
            (dict(), dict(aa=4, aa_shadows=False, aa_cos=0.5, aa_plane=0.25),
             CAMERA_PASS + HARD + ["aa_edges", "grid_build_uniform", "aa_gather"] + plain + ["aa_resolve"]),
            (dict(ao=4, ao_radius=1.0), dict(aa=4, aa_sets=4),
             CAMERA_PASS + HARD + ["aa_edges", "grid_build_uniform", "ao_rays", "trace_dda_any_hemi", "aa_gather"] + plain
             + ["aa_resolve", "shade_ao"]),
            (dict(shade=False), dict(aa=4), CAMERA_PASS + HARD)):
        r = _fake(ugrt)
        r.display(setup, **aa, **kw)
        assert _names(r) == want, (kw, aa, _names(r))
        if not kw.get("shade", True):
            continue
        S, sets = aa["aa"], aa.get("aa_sets", 1)
        shadowed = kw.get("shadows", True) and aa.get("aa_shadows", True)
        call = {c[0]: c for c in r.ctx.calls}
        e = call["aa_edges"]
        plane = aa.get("aa_plane", rmod.default_filter_plane(r.bbmin, r.bbmax))
        assert e[1:7] == ("n", "t", "d", "ids", "cam", "mi") and e[7] == ("sh" if shadowed else None)
        assert e[8:] == (float(np.float32(aa.get("aa_cos", 0.9))), plane, "aaedge")
        g = call["aa_gather"]
        assert g[1:6] == ("value", "span", "offset", "v", "f") and g[7:11] == ("aaedge", S) + TILE[sets]
        np.testing.assert_array_equal(np.float32(g[6]), np.float32(cam.camcoords))
        assert g[11][0] == "aotable" and bits(g[11][1]).tobytes() == bits(ugrt.scenes.aa_offset_sets(S, sets)).tobytes()
        assert g[12:15] == ("mi", "ml", 3) and g[16:] == (1e-3, "aasum")
        if shadowed:
            np.testing.assert_array_equal(np.float32(g[15]), np.float32(lcam.worldori[:3]))
        else:
            assert g[15] is None
        assert call["aa_resolve"][1:] == ("img", "aasum", S)
        assert list(r._aa_set_tables) == [(S, sets)]
        r.display(setup, **aa, **kw)  # the table is kept
        assert list(r._aa_set_tables) == [(S, sets)]


@pytest.mark.parametrize("name", ["hall", "crash", "glass", "mirrors"])
def test_one_sample_without_an_offset_is_the_primary_hit(ugrt, O, AA, name):
    """Seamlessness: S = 1, offset (0, 0), every pixel flagged, no shadow light -- the checker's hit id and t are the
    oracle's primary id and t bit for bit on every pixel, and its bytes the oracle frame's unshadowed image."""
    W, H = SIZES[name]
    f = frame(O, ugrt, name, W, H)
    N = f["N"]
    sums, (t, ids) = cpu_sums(AA, f, np.ones(N, np.int32), 1, (1, 1), ugrt.scenes.aa_offsets(1), False, detail=True)
    pr = f["primary"]
    np.testing.assert_array_equal(ids[0], pr["id"])
    np.testing.assert_array_equal(bits(t[0]), bits(pr["t"]))
    sums = sums.reshape(N, 4)
    assert (sums[:, 3] == 1).all()
    np.testing.assert_array_equal(sums[:, :3].astype(np.uint8).reshape(-1), f["image_unshadowed"])
    np.testing.assert_array_equal(AA.resolve(np.zeros(3 * N, np.uint8), sums.reshape(-1), 1, 0, N), f["image_unshadowed"])
    assert int((pr["id"] >= 0).sum()) > N // 4 and int((f["image_unshadowed"] != 0).sum()) > N // 4


@pytest.mark.parametrize("name,lo,hi", [("hall", 0.0, 0.25), ("glass", 0.0, 0.25), ("mirrors", 0.0, 0.25), ("crash", 0.0, 1.0)])
def test_the_edge_criterion_flags_a_minority_of_the_pixels(ugrt, O, AA, name, lo, hi):
    """Under the defaults, with the oracle's shadow flags.  crash is a soup of tiny triangles and carries no cap."""
    W, H = SIZES[name]
    f = frame(O, ugrt, name, W, H)
    edge = cpu_edges(AA, f, True)
    share = float(edge.sum()) / f["N"]
    print(name, "edge share", share)
    assert set(np.unique(edge)) <= {0, 1} and lo < share < hi
    pr = f["primary"]
    hit = ((pr["t"] > 0) & (pr["id"] >= 0)).reshape(H, W)
    # a miss with only misses around it is no edge; a pixel whose neighbourhood mixes hits and misses is one
    pad = np.pad(hit, 1, mode="edge")
    around = np.stack([pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    assert not edge.reshape(H, W)[~around.any(0)].any()
    assert edge.reshape(H, W)[around.any(0) & ~around.all(0)].all()
    # without the shadow flags no more pixels are flagged, and a band writes its own pixels only
    bare = cpu_edges(AA, f, False)
    assert (bare <= edge).all()
    p0, n = 8 * W, 16 * W
    band = cpu_edges(AA, f, True, p0=p0, n=n, fill=-7)
    assert (band[:p0] == -7).all() and (band[p0 + n:] == -7).all()
    np.testing.assert_array_equal(band[p0:p0 + n], edge[p0:p0 + n])


@pytest.mark.parametrize("shadows", [False, True])
def test_supersampled_edges_lie_closer_to_the_converged_image(ugrt, O, AA, shadows):
    """hall 128 x 128: the mean absolute byte error against the checker's own S = 32 image of ALL pixels is strictly
    smaller at aa = 4 and at aa = 8 than the plain image's."""
    f = frame(O, ugrt, "hall", 128, 128, shadows=shadows)
    N = f["N"]
    _, _, ref = cpu_aa(AA, ugrt, f, 32, 1, shadows, edge=np.ones(N, np.int32))
    err = lambda img: float(np.abs(img.astype(np.int32) - ref.astype(np.int32)).mean())
    plain, e4, e8 = err(f["image"]), err(cpu_aa(AA, ugrt, f, 4, 1, shadows)[2]), err(cpu_aa(AA, ugrt, f, 8, 1, shadows)[2])
    print("shadows", shadows, "plain", plain, "aa=4", e4, "aa=8", e8)
    assert e4 < plain and e8 < plain


# ---------------------------------------------------------------------------------------------------------------- GPU

SMALL = {"hall": (64, 64, (2, 5)), "crash": (64, 40, (1, 3))}  # width, height, the tile rows of the band context


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _context(ugrt, f, rows=None, flags=0):
    """A context in a frame's state behind its shadow stage: the uniform grid built, the light camera's block current."""
    s = f["scene"]
    ctx = ugrt.Context(f["W"], f["H"], light_grid=LG, uniform_dims=UD, rows=rows, flags=flags)
    v3 = _f32(s["verts"]).reshape(-1, 3)
    dv, df = ctx.upload(v3.reshape(-1)), ctx.upload(_i32(s["faces"]).reshape(-1))
    ctx.grid_build_uniform(df, dv, len(_i32(s["faces"]).reshape(-1)) // 3, v3.min(0), v3.max(0))
    ctx.upload_camera(f["lcam"].cc)
    ctx.set_light_position(f["setup"].shading_light)
    pr = f["primary"]
    return types.SimpleNamespace(ctx=ctx, dv=dv, df=df, grid=ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3],
                                 mat_idx=ctx.upload(_i32(s["matidx"])), mat_list=ctx.upload(_f32(s["mat_list"]).reshape(-1)),
                                 nmat=len(_f32(s["mat_list"]).reshape(-1)) // 6, normal=ctx.upload(pr["normal"]),
                                 t=ctx.upload(pr["t"]), dir=ctx.upload(pr["dir"]), ids=ctx.upload(pr["id"]),
                                 cam_pos=ctx.upload(f["cam_pos"]), shadowed=ctx.upload(f["is_shadowed"]))


def _gather(torch, d, f, edge, S, tile, table, shadow, sentinel=-1, dv=None, df=None):
    sums = torch.full((4 * f["N"],), sentinel, dtype=torch.int32, device=d.ctx.device)
    d.ctx.aa_gather(d.grid[0], d.grid[1], d.grid[2], d.dv if dv is None else dv, d.df if df is None else df, f["cam"].cc,
                    d.ctx.upload(edge), S, tile[0], tile[1], table, d.mat_idx, d.mat_list, d.nmat,
                    f["lcam"].worldori[:3].copy() if shadow else None, EPS, sums)
    d.ctx.synchronize()
    return _words(sums)


def _edge_forms(AA, f, p0, n):
    N = f["N"]
    last = np.zeros(N, np.int32)
    last[p0 + n - 1] = 1
    return (("real", cpu_edges(AA, f, True)), ("ones", np.ones(N, np.int32)), ("zeros", np.zeros(N, np.int32)), ("last", last))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3, 8, 32])
@pytest.mark.parametrize("name", ["hall", "crash"])
def test_gather_equals_the_checker(ugrt, O, AA, torch, name, S):
    """Sets of 1, 4 and 16, with and without the shadow light, four forms of the flags, on the whole frame and on a band in
    its middle with sentinel-filled outputs: the checker's words, exactly."""
    W, H, rows = SMALL[name]
    f = frame(O, ugrt, name, W, H)
    N = f["N"]
    whole, band = _context(ugrt, f), _context(ugrt, f, rows)
    p0, n = band.ctx.p0, band.ctx.npix
    assert (p0, n) == (rows[0] * 8 * W, (rows[1] - rows[0]) * 8 * W)
    nonzero = 0
    for sets in (1, 4, 16):
        offsets = ugrt.scenes.aa_offset_sets(S, sets)
        for shadow in (True, False):
            for what, edge in _edge_forms(AA, f, p0, n):
                msg = "%s S %d sets %d shadow %s edge %s" % (name, S, sets, shadow, what)
                want = cpu_sums(AA, f, edge, S, TILE[sets], offsets, shadow)
                got = _gather(torch, whole, f, edge, S, TILE[sets], whole.ctx.upload(offsets.reshape(-1)), shadow)
                np.testing.assert_array_equal(got, want, err_msg=msg)
                got = _gather(torch, band, f, edge, S, TILE[sets], band.ctx.upload(offsets.reshape(-1)), shadow, sentinel=-7)
                assert (got[:4 * p0] == 0xFFFFFFF9).all() and (got[4 * (p0 + n):] == 0xFFFFFFF9).all(), msg
                np.testing.assert_array_equal(got[4 * p0:4 * (p0 + n)], want[4 * p0:4 * (p0 + n)], err_msg=msg + ", band")
                if what == "zeros":
                    assert not want.any()
                if what == "ones":
                    nonzero += int((want.reshape(N, 4)[:, :3].sum(1) > 0).sum())
                    assert (want.reshape(N, 4)[:, 3] == 1).all()
    assert nonzero > N
    # through the gather of vertices (not the arrays the grid was built from: no triangle records)
    offsets = ugrt.scenes.aa_offset_sets(S, 4)
    edge = cpu_edges(AA, f, True)
    got = _gather(torch, whole, f, edge, S, (2, 2), whole.ctx.upload(offsets.reshape(-1)), True, dv=whole.dv.clone(), df=whole.df.clone())
    np.testing.assert_array_equal(got, cpu_sums(AA, f, edge, S, (2, 2), offsets, True), err_msg="no records")


@pytest.mark.gpu
def test_gather_under_the_strict_texture_rule(ugrt, O, AA, torch):
    """UGRT_FLAG_STRICT_TEXTURE: the sub-pixel directions go through the texture unit's 8-bit weights, as the primary
    pass's do; with one sample and no offset the bytes are the strict frame's."""
    W, H, _ = SMALL["hall"]
    f = frame(O, ugrt, "hall", W, H, strict=True)
    loose = frame(O, ugrt, "hall", W, H)
    N = f["N"]
    d = _context(ugrt, f, flags=ugrt.FLAG_STRICT_TEXTURE)
    ones = np.ones(N, np.int32)
    for S, sets, shadow in ((1, 1, False), (8, 4, True)):
        offsets = ugrt.scenes.aa_offset_sets(S, sets)
        want = cpu_sums(AA, f, ones, S, TILE[sets], offsets, shadow)
        got = _gather(torch, d, f, ones, S, TILE[sets], d.ctx.upload(offsets.reshape(-1)), shadow)
        np.testing.assert_array_equal(got, want)
        if S == 1:
            np.testing.assert_array_equal(want.reshape(N, 4)[:, :3].astype(np.uint8).reshape(-1), f["image_unshadowed"])
        else:  # (at the pixels' own corners of a 64-pixel row the weights are multiples of 1/16: 8 bits hold them exactly)
            assert (want != cpu_sums(AA, loose, ones, S, TILE[sets], offsets, shadow)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "crash"])
def test_edges_and_resolve_equal_the_checker(ugrt, O, AA, torch, name):
    W, H, rows = SMALL[name]
    f = frame(O, ugrt, name, W, H)
    N = f["N"]
    rng = np.random.RandomState(11)
    img = rng.randint(0, 256, 3 * N).astype(np.uint8)
    for rows_ in (None, rows):
        d = _context(ugrt, f, rows_)
        p0, n = d.ctx.p0, d.ctx.npix
        flagged = 0
        for with_shadows in (True, False):
            for cos, tol in ((COS, f["plane"]), (0.999, 0.0), (-1.0, 1e30), (0.5, -1.0)):
                edge = torch.full((N,), -7, dtype=torch.int32, device=d.ctx.device)
                d.ctx.aa_edges(d.normal, d.t, d.dir, d.ids, d.cam_pos, d.mat_idx, d.shadowed if with_shadows else None, cos, tol, edge)
                d.ctx.synchronize()
                want = cpu_edges(AA, f, with_shadows, cos, tol, p0, n, fill=-7)
                np.testing.assert_array_equal(edge.cpu().numpy(), want, err_msg="%s cos %g tol %g rows %s" % (name, cos, tol, rows_))
                flagged += int((want == 1).sum())
        assert flagged > 100
        for S in (1, 3, 8, 32):
            sums = cpu_sums(AA, f, cpu_edges(AA, f, True), S, (1, 1), ugrt.scenes.aa_offsets(S), True).copy()
            sums.reshape(N, 4)[::5, 3] = 0  # pixels nobody supersampled keep their bytes, whatever the other words say
            d_img = d.ctx.upload(img)
            d.ctx.aa_resolve(d_img, d.ctx.upload(sums.view(np.int32)), S)
            d.ctx.synchronize()
            want = AA.resolve(img, sums, S, p0, n)
            np.testing.assert_array_equal(d_img.cpu().numpy(), want, err_msg="resolve S %d rows %s" % (S, rows_))
            assert (want[:3 * p0] == img[:3 * p0]).all() and int((want != img).sum()) > 100


@pytest.mark.gpu
def test_launch_shapes_change_no_word(ugrt, O, AA, torch):
    """any_coop at 1, 8 and 2^30, any_rays_per_wave at 32 and 64, and dda_blocks = 1 (every later group from the ticket)."""
    W, H, _ = SMALL["crash"]
    f = frame(O, ugrt, "crash", W, H)
    d = _context(ugrt, f)
    ones = np.ones(f["N"], np.int32)
    for S, sets in ((8, 16), (3, 4)):
        offsets = ugrt.scenes.aa_offset_sets(S, sets)
        table = d.ctx.upload(offsets.reshape(-1))
        want = cpu_sums(AA, f, ones, S, TILE[sets], offsets, True)
        for rpw in (32, 64):
            for coop in (1, 8, 1 << 30):
                d.ctx.set_option("any_rays_per_wave", rpw)
                d.ctx.set_option("any_coop", coop)
                np.testing.assert_array_equal(_gather(torch, d, f, ones, S, TILE[sets], table, True), want,
                                              err_msg="S %d rays per wave %d, coop %d" % (S, rpw, coop))
        d.ctx.set_option("any_rays_per_wave", -1)
        d.ctx.set_option("any_coop", -1)
        for blocks in (1, 7):
            d.ctx.set_option("dda_blocks", blocks)
            np.testing.assert_array_equal(_gather(torch, d, f, ones, S, TILE[sets], table, True), want, err_msg="blocks %d" % blocks)
        d.ctx.set_option("dda_blocks", -1)


def _make(ugrt, s, W, H):
    ctx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
    return ctx, ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])


@pytest.mark.gpu
@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("name", ["hall", "crash"])
def test_frames_equal_the_cpu_frames(ugrt, O, REFS, AO, AA, torch, name, shadows):
    """display(aa=4, aa_sets=16) and display(aa=8): image, aa_edge and aa_sum are the frame composed on the CPU from the
    oracle's frame plus the checker; with ao=8 behind it the image is the checker's scaled by the ambient occlusion's
    reference; and a frame without the keyword on the same renderer is the frame as it was."""
    W, H = SIZES[name]
    f = frame(O, ugrt, name, W, H, shadows=shadows)
    s, N, setup = f["scene"], f["N"], f["setup"]
    ctx, r = _make(ugrt, s, W, H)
    r.display(setup, shadows=shadows)
    ctx.synchronize()
    off = r.image.cpu().numpy().copy()
    np.testing.assert_array_equal(off, f["image"])
    assert r.aa_edge is None and r.aa_sum is None
    for kw in (dict(aa=4, aa_sets=16), dict(aa=8)):
        edge, sums, image = cpu_aa(AA, ugrt, f, kw["aa"], kw.get("aa_sets", 1), shadows)
        r.display(setup, shadows=shadows, **kw)
        ctx.synchronize()
        np.testing.assert_array_equal(r.aa_edge.cpu().numpy(), edge, err_msg=str(kw))
        np.testing.assert_array_equal(_words(r.aa_sum), sums, err_msg=str(kw))
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), f["mat_ids"], err_msg=str(kw))
        np.testing.assert_array_equal(r.image.cpu().numpy(), image, err_msg=str(kw))
        assert int((image != off).sum()) > 1000
    # ambient occlusion scales the finished image
    pr, verts, faces = f["primary"], _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    v3 = verts.reshape(-1, 3)
    radius = float(np.float32(0.05 * float((v3.max(0) - v3.min(0)).max())))
    orays, oactive = AO.rays(f["cam_pos"], pr["t"], pr["dir"], pr["id"], verts, faces, EPS, 0, N, N)
    mask = AM.cpu_mask(REFS[1], AO, f["ugrid"], s["verts"], s["faces"], orays, oactive, ugrt.scenes.ao_directions(8), radius, 0, N, N)
    r.display(setup, shadows=shadows, aa=8, ao=8, ao_radius=radius)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), AO.shade(cpu_aa(AA, ugrt, f, 8, 1, shadows)[2], mask, 8, 0, N))
    # aa_shadows=False: the shadow edges are not flagged and the samples are not shadowed
    if shadows:
        edge, sums, image = cpu_aa(AA, ugrt, f, 4, 1, True, aa_shadows=False)
        r.display(setup, shadows=True, aa=4, aa_shadows=False)
        ctx.synchronize()
        np.testing.assert_array_equal(r.aa_edge.cpu().numpy(), edge)
        np.testing.assert_array_equal(_words(r.aa_sum), sums)
        np.testing.assert_array_equal(r.image.cpu().numpy(), image)
    r.display(setup, shadows=shadows)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), off, err_msg="behind an aa frame")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "glass"])
def test_one_sample_per_edge_pixel_is_the_plain_frame(ugrt, O, torch, name):
    """The seam test on the device: display(aa=1, aa_sets=1, shadows=False) equals display(shadows=False) byte for byte."""
    W, H = SIZES[name]
    s = scene(ugrt, name)
    setup = ugrt.FrameSetup.from_scene(s)
    ctx, r = _make(ugrt, s, W, H)
    r.display(setup, shadows=False)
    ctx.synchronize()
    plain = r.image.cpu().numpy().copy()
    r.display(setup, aa=1, aa_sets=1, shadows=False)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), plain)
    flagged = r.aa_edge.cpu().numpy() == 1
    assert 100 < int(flagged.sum()) < W * H // 4
    sums = _words(r.aa_sum).reshape(-1, 4)
    assert (sums[flagged, 3] == 1).all() and not sums[~flagged].any()
    np.testing.assert_array_equal(sums[flagged, :3].astype(np.uint8), plain.reshape(-1, 3)[flagged])
    assert int((plain != 0).sum()) > W * H // 4


PROF_STAGES = tuple("build_count build_scan build_fill build_sort build_bounds trace_primary map_rays sort_rays trace_shadow shade "
                    "reflect_gen trace_dda worklist shadow_cull shadow_prep".split())


@pytest.mark.gpu
def test_aa_0_is_the_frame_as_it_was_launch_for_launch(ugrt, O, torch):
    """The image and the launches per stage (ugrt_prof_get) of display(aa=0, ...) against a second renderer that is never
    given the keyword; and an aa frame adds exactly its own brackets."""
    W, H = SIZES["hall"]
    f = frame(O, ugrt, "hall", W, H)
    s, setup = f["scene"], f["setup"]

    def counts(ctx):
        return {k: v[1] for k, v in ctx.prof_get().items() if k in PROF_STAGES}

    out = []
    for kw in (dict(), dict(aa=0, aa_sets=1, aa_cos=0.9, aa_plane=None, aa_shadows=True)):
        ctx, r = _make(ugrt, s, W, H)
        r.display(setup, **kw)  # (the first frame builds what later frames keep)
        ctx.prof_enable(True, stages=PROF_STAGES)
        ctx.prof_reset()
        r.display(setup, **kw)
        ctx.synchronize()
        out.append((counts(ctx), r.image.cpu().numpy().copy(), ctx, r))
    assert out[0][0] == out[1][0] and sum(out[0][0].values()) > 5
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][1], f["image"])
    assert out[1][3].aa_edge is None and out[1][3].aa_sum is None
    ctx, r = out[1][2], out[1][3]
    r.display(setup, aa=4)  # (builds the uniform grid)
    ctx.prof_reset()
    r.display(setup, aa=4)
    ctx.synchronize()
    with_aa = counts(ctx)
    base = out[0][0]
    assert with_aa["shade"] == base["shade"] + 2 and with_aa["worklist"] == base["worklist"] + 1
    assert with_aa["trace_dda"] == base["trace_dda"] + 1
    assert {k: v for k, v in with_aa.items() if k not in ("shade", "worklist", "trace_dda") and not k.startswith("build_")} \
        == {k: v for k, v in base.items() if k not in ("shade", "worklist", "trace_dda") and not k.startswith("build_")}


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, AA, torch):
    W, H, _ = SMALL["hall"]
    f = frame(O, ugrt, "hall", W, H)
    N = f["N"]
    fresh = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD)
    z = torch.zeros(6 * N, dtype=torch.int32, device=fresh.device)
    with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
        fresh.aa_gather(z, z, z, z, z, f["cam"].cc, z, 4, 1, 1, z, z, z, 4, None, EPS, z)
    assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    d = _context(ugrt, f)
    ctx = d.ctx
    offsets = ugrt.scenes.aa_offset_sets(4, 4)
    table = ctx.upload(offsets.reshape(-1))
    ones = np.ones(N, np.int32)
    d_edge = ctx.upload(ones)
    sums = torch.full((4 * N + 4,), -1, dtype=torch.int32, device=ctx.device)
    edge = torch.full((N,), -1, dtype=torch.int32, device=ctx.device)
    img = torch.full((3 * N,), 200, dtype=torch.uint8, device=ctx.device)
    light = f["lcam"].worldori[:3].copy()
    args = [d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, f["cam"].cc, d_edge, 4, 2, 2, table, d.mat_idx, d.mat_list, d.nmat, light,
            EPS, sums[:4 * N]]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    def swap(a, h, v):
        return a[:h] + [v] + a[h + 1:]

    for bad in (0, 33, -1):
        fails(ctx.aa_gather, swap(args, 7, bad), b"num_samples")
    for bad in (0, 5):
        fails(ctx.aa_gather, swap(args, 8, bad), b"set_w")
        fails(ctx.aa_gather, swap(args, 9, bad), b"set_h")
    fails(ctx.aa_gather, swap(args, 15, float("nan")), b"eps")
    for bad in (0, -3):
        fails(ctx.aa_gather, swap(args, 13, bad), b"num_materials")
    fails(ctx.aa_gather, swap(args, 16, sums[1:4 * N + 1]), b"d_sum")
    for h in (0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 16):
        fails(ctx.aa_gather, swap(args, h, None), b"null")
    e_args = [d.normal, d.t, d.dir, d.ids, d.cam_pos, d.mat_idx, d.shadowed, COS, f["plane"], edge]
    fails(ctx.aa_edges, swap(e_args, 7, float("nan")), b"normal_cos")
    fails(ctx.aa_edges, swap(e_args, 8, float("nan")), b"plane_tol")
    for h in (0, 1, 2, 3, 4, 5, 9):
        fails(ctx.aa_edges, swap(e_args, h, None), b"null")
    r_args = [img, sums[:4 * N], 4]
    for bad in (0, 33):
        fails(ctx.aa_resolve, swap(r_args, 2, bad), b"num_samples")
    fails(ctx.aa_resolve, swap(r_args, 1, sums[1:4 * N + 1]), b"d_sum")
    for h in (0, 1):
        fails(ctx.aa_resolve, swap(r_args, h, None), b"null")
    ctx.synchronize()
    assert (_words(sums) == 0xFFFFFFFF).all() and (edge == -1).all() and (img == 200).all()  # nothing ran
    want = cpu_sums(AA, f, ones, 4, (2, 2), offsets, True)
    np.testing.assert_array_equal(_gather(torch, d, f, ones, 4, (2, 2), table, True), want)
    # and the context renders a correct frame afterwards
    big = frame(O, ugrt, "hall", *SIZES["hall"])
    ctx2, r = _make(ugrt, big["scene"], *SIZES["hall"])
    with pytest.raises(ugrt.UgrtError):
        ctx2.aa_resolve(r.image, None, 4)
    r.display(big["setup"], aa=4)
    ctx2.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), cpu_aa(AA, ugrt, big, 4, 1, True)[2])
