"""Depth of field: ugrt_dof_pixels, ugrt_dof_gather and display(dof=...).

The checker is tests/dof_ref.c, a plain-C restatement with one loop per sample on top of aa_ref.c's walks.  With an
all-zero table it is compared with the oracle's primary pass and frame, with lens points (0, 0) with aa_ref.c; the kernels
are compared with it exactly.  tests/test_dof_synthetic.py holds ugrt_dof_pixels' synthetic g-buffer."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import test_ambient as AM
import test_antialias as TA
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
from test_ambient import AO  # noqa: F401  (fixtures)
from test_antialias import AA  # noqa: F401
from test_reflect_shadows import REFS  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, bits, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.LG, RD.UD
_u32, _opt, _words, _names = TA._u32, TA._opt, TA._words, TA._names
CALLS = ("ugrt_dof_pixels", "ugrt_dof_gather")
EPS, TILE = TA.EPS, TA.TILE
CAMERA_PASS, HARD = TA.CAMERA_PASS, TA.HARD


class DofRef:
    def __init__(self, lib):
        self.lib = lib

    def pixels(self, pr, axis, focus, coc_scale, coc_min, R, W, H, p0, n, fill=0):
        flag = np.full(W * H, fill, np.int32)
        coc = np.zeros(W * H, np.float32)
        self.lib.dof_pixels(_p(_f32(pr["t"])), _p(_f32(pr["dir"])), _p(_i32(pr["id"])), _p(_f32(axis)), C.c_float(focus),
                            C.c_float(coc_scale), C.c_float(coc_min), C.c_int(R), C.c_int(W), C.c_int(H), C.c_int(p0), C.c_int(n),
                            _p(coc), _p(flag))
        return flag

    def coc(self, pr, axis, focus, coc_scale, W, H):
        coc = np.zeros(W * H, np.float32)
        self.lib.dof_coc(_p(_f32(pr["t"])), _p(_f32(pr["dir"])), _p(_i32(pr["id"])), _p(_f32(axis)), C.c_float(focus),
                         C.c_float(coc_scale), C.c_int(W), C.c_int(H), _p(coc))
        return coc

    def rays(self, cam, strict, W, H, lens, px, py, ent):
        n = len(px)
        o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        self.lib.dof_rays(_p(_f32(cam.cc)), _p(_f32(cam.tex)), C.c_int(1 if strict else 0), C.c_int(W), C.c_int(H), _p(_f32(lens)),
                          C.c_int(n), _p(_i32(px)), _p(_i32(py)), _p(_f32(ent).reshape(-1)), _p(o), _p(d))
        return o, d

    def gather(self, ugrid, verts, faces, cam, strict, W, H, lens, flags, S, tile, table, mat_idx, mat_list, cc, light,
               shadow_light, eps, p0, n, fill=0, detail=False):
        """[4N] sums; detail: also (hit_t, hit_id), each [S, N].  cam: the eye's oracle_lib.Cam."""
        N = W * H
        sums = np.full(4 * N, fill, np.uint32)
        mat_list = _f32(mat_list).reshape(-1)
        det = [np.zeros(S * N, t) for t in (np.float32, np.int32)] if detail else [None, None]
        self.lib.dof_gather(_p(_f32(ugrid["ug"])), _p(_i32(ugrid["dims"])), _p(_u32(ugrid["vals"])), _p(_u32(ugrid["span"])),
                            _p(_u32(ugrid["offset"])), _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)), _p(_f32(cam.cc)),
                            _p(_f32(cam.tex)), C.c_int(1 if strict else 0), C.c_int(W), C.c_int(H), _p(_f32(lens)), _p(_i32(flags)),
                            C.c_int(S), C.c_int(tile[0]), C.c_int(tile[1]), _p(_f32(table).reshape(-1)), _p(_i32(mat_idx)),
                            _p(mat_list), C.c_int(len(mat_list) // 6), _p(_f32(cc)), _p(_f32(light)),
                            _opt(None if shadow_light is None else _f32(shadow_light)), C.c_float(eps), C.c_int(p0), C.c_int(n),
                            C.c_longlong(N), _p(sums), *[_opt(d) for d in det])
        return (sums, [d.reshape(S, N) for d in det]) if detail else sums


@pytest.fixture(scope="session")
def DOF(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dof_ref") / "libdof_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "dof_ref.c"), "-lm"], check=True, capture_output=True)
    return DofRef(C.CDLL(out))


_CPU = {}


def frame(O, ugrt, name, W, H, shadows=True, strict=False):
    if name == "depth" and "depth" not in TA._SCENES:
        TA._SCENES["depth"] = ugrt.scenes.depth()
    return TA.frame(O, ugrt, name, W, H, shadows=shadows, strict=strict)


def lens_of(ugrt, f, aperture, focus=None, camera=None):
    """(lens[10], coc_scale) of a frame's camera, as the renderer forms them."""
    setup = f["setup"]
    cam = RLT._rmod(ugrt).make_camera(setup.camera if camera is None else camera, setup.fovy,
                                      float(np.float32(f["W"]) / np.float32(f["H"])))
    return cam.lens(aperture, focus, f["H"])


def with_lens(table2, lu=0.0, lv=0.0):
    """[.., 2] offsets -> [.., 4] entries with one lens point."""
    t = np.zeros(table2.shape[:-1] + (4,), np.float32)
    t[..., :2] = table2
    t[..., 2], t[..., 3] = lu, lv
    return t


def cpu_sums(DOF, f, lens, flags, S, tile, table, shadow, p0=0, n=None, fill=0, detail=False, cam=None):
    """The checker's gather under the frame's own state: the light camera's block is the current one."""
    s = f["scene"]
    return DOF.gather(f["ugrid"], s["verts"], s["faces"], f["cam"] if cam is None else cam, f["strict"], f["W"], f["H"], lens, flags,
                      S, tile, table, s["matidx"], s["mat_list"], f["lcam"].cc, f["setup"].shading_light,
                      f["lcam"].worldori[:3].copy() if shadow else None, EPS, p0, f["N"] if n is None else n, fill, detail)


def cpu_dof(DOF, AA, ugrt, f, S, aperture, sets=1, shadows=True, dof_shadows=True, focus=None, cmin=0.5, window=4, camera=None,
            O=None):
    """display(dof=S, dof_aperture=aperture, ...) on the CPU on top of the oracle's frame: (flags, sums, image).  Shared per
    key.  camera: other parameters than the frame's own (the frame's arrays must be that camera's)."""
    key = (id(f), S, aperture, sets, shadows, dof_shadows, focus, cmin, window)
    if key not in _CPU:
        lens, coc_scale = lens_of(ugrt, f, aperture, focus, camera)
        flags = DOF.pixels(f["primary"], lens[6:9], float(lens[9]), coc_scale, cmin, window, f["W"], f["H"], 0, f["N"])
        sums = cpu_sums(DOF, f, lens, flags, S, TILE[sets], ugrt.scenes.lens_sample_sets(S, sets), shadows and dof_shadows)
        _CPU[key] = (flags, sums, AA.resolve(f["image"], sums, S, 0, f["N"]))
    return _CPU[key]


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_the_header_the_library_and_the_prototypes_name_the_calls(ugrt):
    with open(os.path.join(RD.ROOT, "include", "ugrt.h")) as fh:
        header = fh.read()
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert "int %s(ugrt_ctx *ctx" % name in header and hasattr(lib, name) and name in ugrt.PROTOTYPES
    assert "#define UGRT_MAX_DOF_WINDOW 8" in header and ugrt.MAX_DOF_WINDOW == 8
    for name in ("dof_pixels", "dof_gather"):
        assert callable(getattr(ugrt.Context, name))
    assert len(ugrt.PROTOTYPES["ugrt_dof_pixels"][1]) == 10 and len(ugrt.PROTOTYPES["ugrt_dof_gather"][1]) == 19
    rmod = RLT._rmod(ugrt)
    assert callable(rmod.check_dof) and callable(rmod.dof_pixels) and callable(rmod.dof_pass)
    import inspect

    for cls in (ugrt.Renderer, ugrt.BandedRenderer):
        sig = inspect.signature(cls.display).parameters
        assert [sig[k].default for k in ("dof", "dof_aperture", "dof_focus", "dof_sets", "dof_min", "dof_window", "dof_shadows")] \
            == [0, 0.0, None, 1, 0.5, 4, True]


def test_lens_sample_sets(ugrt):
    sc = ugrt.scenes
    for S in (1, 2, 3, 8, 16, 32):
        for sets in (1, 4, 16):
            t = sc.lens_sample_sets(S, sets)
            assert t.shape == (sets, S, 4) and t.dtype == np.float32 and t.flags["C_CONTIGUOUS"]
            assert (t[..., :2] >= -0.5).all() and (t[..., :2] < 0.5).all()
            assert ((t[..., 2].astype(np.float64) ** 2 + t[..., 3].astype(np.float64) ** 2) < 1.0).all()
            assert bits(t).tobytes() == bits(sc.lens_sample_sets(S, sets)).tobytes()  # deterministic
            assert bits(t[..., :2]).tobytes() == bits(sc.aa_offset_sets(S, sets)).tobytes()
            for k in range(1, sets):
                assert bits(t[k, :, :2]).tobytes() != bits(t[0, :, :2]).tobytes()
                assert bits(t[k, :, 2:]).tobytes() != bits(t[0, :, 2:]).tobytes()
            if S > 1:  # the points spread over the disk: not all in one half
                assert (t[0, :, 2] > 0).any() and (t[0, :, 2] < 0).any()
    for bad in (0, 2, 3, 8, 17):
        with pytest.raises(ValueError):
            sc.lens_sample_sets(4, bad)


def test_the_depth_scene(ugrt):
    s = ugrt.scenes.depth()
    posts = s["posts"]
    assert len(posts) == 5 and [d for _, _, d in posts] == sorted(d for _, _, d in posts)
    v, f = s["verts"].reshape(-1, 3), s["faces"].reshape(-1, 3)
    sizes = []
    for a, b, dist in posts:
        pv = v[np.unique(f[a:b])]
        sizes.append(tuple(np.round(pv.max(0) - pv.min(0), 5)))
        assert abs(float(pv[:, 0].mean()) - (1.0 + dist)) < 1e-4
    assert len(set(sizes)) == 1  # identical posts
    cam = s["cameras"]["ref"]
    assert np.allclose(np.subtract(cam["look"], cam["eye"]), (posts[2][2], 0, 0))  # the look-at lies on the middle post


def test_the_lens_of_a_camera(ugrt):
    rmod = RLT._rmod(ugrt)
    s = ugrt.scenes.depth()
    cam = rmod.make_camera(s["cameras"]["ref"], 45.0, 1.0)
    lens, coc_scale = cam.lens(0.25, None, 128)
    assert lens.dtype == np.float32 and lens.shape == (10,)
    np.testing.assert_allclose(lens[6:9], (1, 0, 0), atol=1e-7)
    assert lens[9] == 12.0
    U, V, A = lens[0:3].astype(np.float64), lens[3:6].astype(np.float64), lens[6:9].astype(np.float64)
    assert abs(np.linalg.norm(U) - 0.25) < 1e-6 and abs(np.linalg.norm(V) - 0.25) < 1e-6
    assert abs(U @ V) < 1e-7 and abs(U @ A) < 1e-7 and abs(V @ A) < 1e-7
    np.testing.assert_allclose(V / 0.25, (0, 0, 1), atol=1e-6)  # the second axis is the camera's up
    f_px = 64.0 / np.tan(np.radians(45.0) / 2)
    assert abs(coc_scale - 0.25 * f_px / 12.0) < 1e-5
    assert cam.lens(0.25, 6.0, 128)[0][9] == 6.0 and abs(cam.lens(0.25, 6.0, 128)[1] - 0.25 * f_px / 6.0) < 1e-5
    assert not cam.lens(0.0, None, 128)[0][:6].any() and cam.lens(0.0, None, 128)[1] == 0.0


def _fake(ugrt):
    r = TA._fake(ugrt)
    r.__dict__.update(dof_flag="dofflag", dof_sum="dofsum", _dof_set_tables={})
    r._ensure_dof_buffers = lambda: None
    r.ctx.height = 128
    return r


def test_dof_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    chk = rmod.check_dof
    assert chk(0) is None
    assert chk(4, 0.1) == (4, 1, float(np.float32(0.1)), None, 0.5, 4, True)
    assert chk(np.int64(32), np.float32(0.5), 3, np.int32(16), 1, np.int64(8), np.bool_(False)) == (32, 16, 0.5, 3.0, 1.0, 8, False)
    assert chk(4) == (4, 1, 0.0, None, 0.5, 4, True)  # a lens of radius 0: legal, flags nothing
    for bad in (-1, 33, 1.5, True, "4", None, np.float32(2)):
        with pytest.raises(ValueError):
            chk(bad, 0.1)
    for bad in (-0.1, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError):
            chk(4, bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError):
            chk(4, 0.1, bad)
    for bad in (0, 2, 3, 17, 16.0, True, "4", None):
        with pytest.raises(ValueError):
            chk(4, 0.1, None, bad)
    for bad in (0, -0.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError):
            chk(4, 0.1, None, 1, bad)
    for bad in (-1, 9, 4.0, True, "4", None):
        with pytest.raises(ValueError):
            chk(4, 0.1, None, 1, 0.5, bad)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError):
            chk(4, 0.1, None, 1, 0.5, 4, bad)
    # a value away from its default needs dof > 0
    for kw in (dict(dof_aperture=0.1), dict(dof_focus=2.0), dict(dof_sets=4), dict(dof_min=1.0), dict(dof_window=2),
               dict(dof_shadows=False)):
        with pytest.raises(ValueError):
            chk(0, **kw)
    # the frames that stay open; with dof = 0 they are what they were
    for kw in (dict(aa=4), dict(reflect=True), dict(refract=True), dict(fresnel=True), dict(glossy=4), dict(gi=4), dict(area=4),
               dict(smooth=True), dict(temporal=4), dict(frame_cnt=2), dict(lights=[("cam", "pos")]), dict(reflect_lights=True),
               dict(two_streams=True)):
        with pytest.raises(ValueError):
            chk(4, 0.1, **kw)
        assert chk(0, **kw) is None
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    on = dict(dof=4, dof_aperture=0.1)
    for kw in (dict(dof=33), dict(dof=True), dict(dof_sets=16), dict(dof_aperture=0.1), dict(dof=4, dof_sets=3), dict(dof=4, dof_min=0),
               dict(dof=4, dof_window=9), dict(dof=4, dof_shadows=1), dict(dof=4, dof_focus=0.0), dict(dof=4, dof_aperture=-1.0),
               dict(on, aa=4), dict(on, reflect=True), dict(on, reflect=True, bounces=3, reflect_shadows=True),
               dict(on, reflect=True, refract=True), dict(on, reflect=True, refract=True, fresnel=True), dict(on, glossy=4),
               dict(on, gi=4), dict(on, area=4, area_radius=0.5), dict(on, smooth=True), dict(on, ao=4, ao_radius=1.0, temporal=4),
               dict(on, frame_cnt=2)):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(setup, **kw)
        assert r.ctx.calls == [], kw
    for lights_setup, kw in ((TL.setup_for(ugrt, s, TL.lights_for(s, 2)), dict()),
                             (TL.setup_for(ugrt, s, TL.lights_for(s, 2)), dict(reflect=True, reflect_lights=True))):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(lights_setup, **on, **kw)
        assert r.ctx.calls == []
    r = _fake(ugrt)
    r.aux = object()  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(setup, **on)
    assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    for kw in (on, dict(dof=4, reflect=False), dict(dof_sets=16), dict(dof_shadows=False), dict(dof_aperture=0.5)):
        with pytest.raises(ValueError):
            br.display(setup, **kw)


def test_a_dof_frame_enqueues_its_calls_in_order_and_the_default_frame_none_of_them(ugrt):
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    new = {"dof_pixels", "dof_gather"}
    for kw in (dict(), dict(reflect=True), dict(ao=4, ao_radius=1.0), dict(shadows=False), dict(shade=False), dict(aa=4)):
        a, b = TA._fake(ugrt), TA._fake(ugrt)
        a.display(setup, **kw)
        b.display(setup, dof=0, dof_aperture=0.0, dof_focus=None, dof_sets=1, dof_min=0.5, dof_window=4, dof_shadows=True, **kw)
        assert _names(a) == _names(b) and not set(_names(a)) & new
        assert not [k for k in vars(b) if k.startswith("dof_") or k.startswith("_dof_")]
    plain = ["shade_simple", "shade_add_shadows"]
    rmod = RLT._rmod(ugrt)
    cam = rmod.make_camera(setup.camera, setup.fovy, 1.0)
    lcam = rmod.make_camera(setup.light_camera, setup.fovy, 1.0)
    for kw, dof, want in (
            (dict(), dict(dof=4, dof_aperture=0.1),
             CAMERA_PASS + HARD + ["dof_pixels", "grid_build_uniform", "dof_gather"] + plain + ["aa_resolve"]),
            (dict(shadows=False), dict(dof=8, dof_aperture=0.2, dof_sets=16, dof_focus=7.5, dof_min=1.0, dof_window=8),
             CAMERA_PASS + ["dof_pixels", "grid_build_uniform", "dof_gather", "shade_simple", "aa_resolve"]),
            (dict(), dict(dof=4, dof_aperture=0.1, dof_shadows=False),
             CAMERA_PASS + HARD + ["dof_pixels", "grid_build_uniform", "dof_gather"] + plain + ["aa_resolve"]),
            (dict(ao=4, ao_radius=1.0), dict(dof=4, dof_aperture=0.1, dof_sets=4),
             CAMERA_PASS + HARD + ["dof_pixels", "grid_build_uniform", "ao_rays", "trace_dda_any_hemi", "dof_gather"] + plain
             + ["aa_resolve", "shade_ao"]),
            (dict(shade=False), dict(dof=4, dof_aperture=0.1), CAMERA_PASS + HARD)):
        r = _fake(ugrt)
        r.display(setup, **dof, **kw)
        assert _names(r) == want, (kw, dof, _names(r))
        if not kw.get("shade", True):
            continue
        S, sets = dof["dof"], dof.get("dof_sets", 1)
        shadowed = kw.get("shadows", True) and dof.get("dof_shadows", True)
        lens, coc_scale = cam.lens(float(np.float32(dof["dof_aperture"])), dof.get("dof_focus"), 128)
        call = {c[0]: c for c in r.ctx.calls}
        e = call["dof_pixels"]
        assert e[1:4] == ("t", "d", "ids") and e[9] == "dofflag"
        np.testing.assert_array_equal(np.float32(e[4]), lens[6:9])
        assert e[5:9] == (float(lens[9]), coc_scale, dof.get("dof_min", 0.5), dof.get("dof_window", 4))
        g = call["dof_gather"]
        assert g[1:6] == ("value", "span", "offset", "v", "f") and g[8:12] == ("dofflag", S) + TILE[sets]
        np.testing.assert_array_equal(np.float32(g[6]), np.float32(cam.camcoords))
        assert bits(np.float32(g[7])).tobytes() == bits(lens).tobytes()
        assert g[12][0] == "aotable" and bits(g[12][1]).tobytes() == bits(ugrt.scenes.lens_sample_sets(S, sets)).tobytes()
        assert g[13:16] == ("mi", "ml", 3) and g[17:] == (1e-3, "dofsum")
        if shadowed:
            np.testing.assert_array_equal(np.float32(g[16]), np.float32(lcam.worldori[:3]))
        else:
            assert g[16] is None
        assert call["aa_resolve"][1:] == ("img", "dofsum", S)
        assert list(r._dof_set_tables) == [(S, sets)]
        r.display(setup, **dof, **kw)  # the table is kept
        assert list(r._dof_set_tables) == [(S, sets)]


def test_one_sample_from_the_lens_centre_is_the_primary_hit(ugrt, O, DOF):
    """Seamlessness: S = 1, an all-zero table, every pixel flagged, no shadow light, a lens of radius 0.3 -- the checker's
    hit id and t are the oracle's primary id and t bit for bit on every pixel of the hall at 128 x 128, and its bytes the
    oracle frame's unshadowed image."""
    f = frame(O, ugrt, "hall", 128, 128)
    N = f["N"]
    lens, _ = lens_of(ugrt, f, 0.3)
    sums, (t, ids) = cpu_sums(DOF, f, lens, np.ones(N, np.int32), 1, (1, 1), np.zeros((1, 1, 4), np.float32), False, detail=True)
    pr = f["primary"]
    np.testing.assert_array_equal(ids[0], pr["id"])
    np.testing.assert_array_equal(bits(t[0]), bits(pr["t"]))
    sums = sums.reshape(N, 4)
    assert (sums[:, 3] == 1).all()
    np.testing.assert_array_equal(sums[:, :3].astype(np.uint8).reshape(-1), f["image_unshadowed"])
    assert int((pr["id"] >= 0).sum()) > N // 4 and int((f["image_unshadowed"] != 0).sum()) > N // 4


@pytest.mark.parametrize("S,sets,shadow", [(4, 4, True), (3, 1, False), (8, 16, True)])
def test_lens_points_at_the_centre_give_the_anti_aliasing_sums(ugrt, O, AA, DOF, S, sets, shadow):
    """(sx, sy, 0, 0), and (sx, sy, lu, lv) under a lens of radius 0: aa_ref.c's sums on the same offsets and flags."""
    f = frame(O, ugrt, "hall", 128, 128)
    flags = TA.cpu_edges(AA, f, True)
    offsets = ugrt.scenes.aa_offset_sets(S, sets)
    want = TA.cpu_sums(AA, f, flags, S, TILE[sets], offsets, shadow)
    lens, _ = lens_of(ugrt, f, 0.3)
    np.testing.assert_array_equal(cpu_sums(DOF, f, lens, flags, S, TILE[sets], with_lens(offsets), shadow), want)
    lens0, _ = lens_of(ugrt, f, 0.0)
    table = ugrt.scenes.lens_sample_sets(S, sets)
    np.testing.assert_array_equal(cpu_sums(DOF, f, lens0, flags, S, TILE[sets], table, shadow), want)
    assert (cpu_sums(DOF, f, lens, flags, S, TILE[sets], table, shadow) != want).any()  # and the lens does move the rays
    assert int(flags.sum()) > 100


QUAD_F = 7.0


def _quad_frame(O, ugrt):
    """One large quad (two triangles) perpendicular to the view axis +x at distance QUAD_F from an eye at (1, 2, 3).  The
    view lies inside one of the triangles, away from the diagonal: two rays to one point of a shared edge may fall on
    different sides of it, or through the crack, which is the tracer's business and not the lens's."""
    eye = np.array([1.0, 2.0, 3.0])
    x = eye[0] + QUAD_F
    verts = np.float32([[x, -20, -140], [x, 140, -140], [x, 140, 20], [x, -20, 20]])
    faces = np.int32([[0, 1, 2], [0, 2, 3]])
    camera = dict(eye=tuple(eye), look=(eye[0] + 3.0, eye[1], eye[2]), up=(0, 0, 1), near=0.1, far=100.0)
    cam = O.cam_from(camera, 45.0, 1.0)
    lo, hi = np.float32([x - 1, -20, -140]), np.float32([x + 1, 140, 20])
    ugrid = O.grid_uniform(faces, verts, lo, hi, (4, 8, 8))
    return types.SimpleNamespace(eye=eye, verts=verts, faces=faces, camera=camera, cam=cam, ugrid=ugrid)


def test_lens_rays_of_a_pixel_meet_on_the_focus_plane(ugrt, O, DOF):
    """A quad at exactly z = F: every lens sample of a pixel with sx = sy = 0 hits within a rounding bound of the pinhole
    hit point.

    The bound.  With u = 2^-24 and exact U, V perpendicular to A, P = o + t d = eye + L + t d0 - t L / s_f = eye + s_f d0
    when t = s_f.  In fp32 each of s_f, L_k (3 roundings), L_k / s_f, d_k, o_k and the two roundings of P_k = o_k + t d_k
    is off by at most u relative to its own magnitude, and the magnitudes are bounded by M = |eye|_inf + a + F / c_min
    (a the lens radius, c_min the smallest cosine between a pixel's direction and A, so that F / c_min bounds |t d|):
    9 u M.  The Moeller-Trumbore t of the checker -- 2 cross products, 3 dot products and a product with the reciprocal,
    26 roundings -- is off by at most 26 u / c_min relative, on both the lens ray and the pinhole ray: 2 * 26 u M / c_min.
    U, V and A are rounded to fp32, so A . L is not 0 but at most 3 u a, which moves t by 3 u a / c_min relative: 3 u M.
    Sum with c_min = cos(atan(sqrt(2) tan(22.5 deg))) > 0.86: (9 + 61 + 3) u M < 80 u M, i.e. 40 ulps of M.  Not a
    measurement; the test prints the largest distance it saw."""
    q = _quad_frame(O, ugrt)
    W = H = 32
    N = W * H
    a = 0.4
    rmod = RLT._rmod(ugrt)
    lens, _ = rmod.make_camera(q.camera, 45.0, 1.0).lens(a, QUAD_F, H)
    assert lens[9] == np.float32(QUAD_F)
    S = 32
    table = np.zeros((1, S, 4), np.float32)
    table[0, :, 2:] = ugrt.scenes.lens_sample_sets(S, 1)[0, :, 2:]
    table[0, 0, 2:] = 0.0  # sample 0: the pinhole ray
    table[0, 1, 2:] = (1.0, 1.0)  # a corner of the lens's square
    table[0, 2, 2:] = (-1.0, 1.0)
    flags = np.ones(N, np.int32)
    mat_idx, mat_list = np.zeros(2, np.int32), np.float32([[0.2, 0.2, 0.2, 0.7, 0.7, 0.7]])
    _, (t, ids) = DOF.gather(q.ugrid, q.verts, q.faces, q.cam, False, W, H, lens, flags, S, (1, 1), table, mat_idx, mat_list,
                             q.cam.cc, np.float32([1, 2, 9]), None, EPS, 0, N, detail=True)
    assert (ids >= 0).all()
    py, px = np.divmod(np.arange(N, dtype=np.int32), W)
    P = []
    for s in range(S):
        o, d = DOF.rays(q.cam, False, W, H, lens, px, py, np.tile(table[0, s], (N, 1)))
        P.append(o + t[s][:, None] * d)  # fp32, as the gather forms the point
    P = np.stack(P).astype(np.float64)
    u = 2.0 ** -24
    c_min = 0.86
    M = float(np.abs(q.eye).max()) + a + QUAD_F / c_min
    dist = np.abs(P[1:] - P[0]).max()
    print("largest distance %.3g, bound %.3g (M = %.3g)" % (dist, 80 * u * M, M))
    assert dist <= 80 * u * M
    assert np.abs(P[0][:, 0] - (q.eye[0] + QUAD_F)).max() <= 80 * u * M  # and that point lies on the quad's plane
    o1, _ = DOF.rays(q.cam, False, W, H, lens, px[:1], py[:1], table[0, 1:2])
    assert np.abs(o1[0] - q.eye).max() > 0.3  # the origins did move


APERTURES = (0.1, 0.2, 0.3)  # the farthest post's circle of confusion: 0.7, 1.4 and 2.1 pixels at 128 x 128


def edge_steps(f, image):
    """Per post of scenes.depth(): the mean absolute byte step, summed over the channels, between the two pixels on either
    side of the post's left and right edges, over the rows of the post above the horizon (where the background is a
    miss).  The edges are where the pinhole frame's ids enter or leave the post."""
    W, H = f["W"], f["H"]
    ids = f["primary"]["id"].reshape(H, W)
    img = image.reshape(H, W, 3).astype(np.int32)
    out = []
    for a, b, _ in f["scene"]["posts"]:
        post = (ids >= a) & (ids < b)
        edge = post[:, 1:] != post[:, :-1]
        miss_side = np.where(post[:, 1:], ids[:, :-1], ids[:, 1:]) < 0  # the pixel outside the post is a miss
        pick = edge & miss_side
        assert int(pick.sum()) >= 16
        out.append(float(np.abs(img[:, 1:] - img[:, :-1]).sum(2)[pick].mean()))
    return out


def test_the_focused_post_stays_sharp_and_the_others_blur_with_the_aperture(ugrt, O, AA, DOF):
    """scenes.depth() at 128 x 128 with dof=16, focused on the middle post: its edges keep a larger byte step than the
    nearest and the farthest post's at every aperture, and the step of those two falls as the aperture grows (it does
    not rise from one aperture to the next and is smaller at the widest than without a lens)."""
    f = frame(O, ugrt, "depth", 128, 128)
    plain = edge_steps(f, f["image"])
    steps = [edge_steps(f, cpu_dof(DOF, AA, ugrt, f, 16, a)[2]) for a in APERTURES]
    print("edge steps without a lens", plain)
    for a, st in zip(APERTURES, steps):
        print("aperture", a, "edge steps", st, "flagged", int(cpu_dof(DOF, AA, ugrt, f, 16, a)[0].sum()))
    for st in steps:
        assert st[2] > st[0] and st[2] > st[4]
    for k in (0, 4):
        ladder = [plain[k]] + [st[k] for st in steps]
        assert all(x >= y for x, y in zip(ladder[:-1], ladder[1:])) and ladder[0] > ladder[-1], (k, ladder)
    # a lens of radius 0 flags nothing and leaves the frame
    flags, sums, image = cpu_dof(DOF, AA, ugrt, f, 16, 0.0)
    assert not flags.any() and not sums.any()
    np.testing.assert_array_equal(image, f["image"])


def test_a_miss_beside_a_blurred_post_is_traced_and_a_miss_among_misses_is_not(ugrt, O, DOF):
    f = frame(O, ugrt, "depth", 128, 128)
    W, H = f["W"], f["H"]
    lens, coc_scale = lens_of(ugrt, f, 0.2)
    pr = f["primary"]
    flags = DOF.pixels(pr, lens[6:9], float(lens[9]), coc_scale, 0.5, 4, W, H, 0, W * H).reshape(H, W)
    coc = DOF.coc(pr, lens[6:9], float(lens[9]), coc_scale, W, H).reshape(H, W)
    hit = ((pr["t"] > 0) & (pr["id"] >= 0)).reshape(H, W)
    assert set(np.unique(flags)) == {0, 1} and (coc[~hit] == 0).all()
    a, b, _ = f["scene"]["posts"][0]
    near = ((pr["id"] >= a) & (pr["id"] < b)).reshape(H, W)
    assert coc[near].min() >= 2.0 and flags[near].all()
    beside = np.zeros_like(near)
    beside[:, 1:] |= near[:, :-1]
    beside[:, :-1] |= near[:, 1:]
    assert int((beside & ~hit).sum()) > 10 and flags[beside & ~hit].all()
    pad = np.pad(hit, 4, mode="constant")
    lonely = ~np.stack([pad[4 + dy:4 + dy + H, 4 + dx:4 + dx + W] for dy in range(-4, 5) for dx in range(-4, 5)]).any(0)
    assert int(lonely.sum()) > 100 and not flags[lonely].any()
    # a band writes its own pixels only
    p0, n = 8 * W, 16 * W
    band = DOF.pixels(pr, lens[6:9], float(lens[9]), coc_scale, 0.5, 4, W, H, p0, n, fill=-7)
    assert (band[:p0] == -7).all() and (band[p0 + n:] == -7).all()
    np.testing.assert_array_equal(band[p0:p0 + n], flags.reshape(-1)[p0:p0 + n])


# ---------------------------------------------------------------------------------------------------------------- GPU

SIZES = {"hall": (128, 128, (3, 11)), "crash": (256, 144, (2, 9))}  # width, height, the tile rows of the band context
TILE_OF = {1: (1, 1), 3: (2, 2), 8: (4, 4), 32: (4, 1)}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _gather(torch, d, f, lens, flags, S, tile, table, shadow, sentinel=-1, dv=None, df=None, cam=None):
    sums = torch.full((4 * f["N"],), sentinel, dtype=torch.int32, device=d.ctx.device)
    d.ctx.dof_gather(d.grid[0], d.grid[1], d.grid[2], d.dv if dv is None else dv, d.df if df is None else df,
                     (f["cam"] if cam is None else cam).cc, lens, d.ctx.upload(_i32(flags)), S, tile[0], tile[1],
                     d.ctx.upload(_f32(table).reshape(-1)), d.mat_idx, d.mat_list, d.nmat,
                     f["lcam"].worldori[:3].copy() if shadow else None, EPS, sums)
    d.ctx.synchronize()
    return _words(sums)


def _table(ugrt, S, tile, seed=5):
    """lens_sample_sets' entries for a tile of any shape: the sets of the 4 x 4 table, dealt row-major."""
    n = tile[0] * tile[1]
    return np.ascontiguousarray(ugrt.scenes.lens_sample_sets(S, 16)[:n])


def _sparse(N, every, phase=0):
    flags = np.zeros(N, np.int32)
    flags[phase::every] = 1
    return flags


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3, 8, 32])
@pytest.mark.parametrize("name", ["hall", "crash"])
def test_gather_equals_the_checker(ugrt, O, DOF, torch, name, S):
    """Tiles of 1 x 1, 2 x 2, 4 x 4 and 4 x 1 (one per S, and all four at S = 3), with and without the shadow light, flags
    all ones, sparse and zero, with and without triangle records, on the whole frame and on a band with row_begin > 0 and
    sentinel-filled outputs: the checker's words, exactly."""
    W, H, rows = SIZES[name]
    f = frame(O, ugrt, name, W, H)
    N = f["N"]
    whole, band = TA._context(ugrt, f), TA._context(ugrt, f, rows)
    p0, n = band.ctx.p0, band.ctx.npix
    assert (p0, n) == (rows[0] * 8 * W, (rows[1] - rows[0]) * 8 * W) and p0 > 0
    v3 = _f32(f["scene"]["verts"]).reshape(-1, 3)
    extent = float((v3.max(0) - v3.min(0)).max())
    lens, _ = lens_of(ugrt, f, 0.01 * extent)
    ones, dense = np.ones(N, np.int32), _sparse(N, 3 if S <= 3 else 11)
    nonzero = 0
    cases = [(TILE_OF[S], True, "sparse", dense), (TILE_OF[S], False, "ones" if S <= 3 else "sparse2", ones if S <= 3 else _sparse(N, 13, 5)),
             (TILE_OF[S], True, "zeros", np.zeros(N, np.int32))]
    if S == 3:
        cases += [(t, k % 2 == 0, "sparse", dense) for k, t in enumerate(((1, 1), (4, 4), (4, 1)))]
    for tile, shadow, what, flags in cases:
        msg = "%s S %d tile %s shadow %s flags %s" % (name, S, tile, shadow, what)
        table = _table(ugrt, S, tile)
        want = cpu_sums(DOF, f, lens, flags, S, tile, table, shadow)
        got = _gather(torch, whole, f, lens, flags, S, tile, table, shadow)
        np.testing.assert_array_equal(got, want, err_msg=msg)
        got = _gather(torch, band, f, lens, flags, S, tile, table, shadow, sentinel=-7)
        assert (got[:4 * p0] == 0xFFFFFFF9).all() and (got[4 * (p0 + n):] == 0xFFFFFFF9).all(), msg
        np.testing.assert_array_equal(got[4 * p0:4 * (p0 + n)], want[4 * p0:4 * (p0 + n)], err_msg=msg + ", band")
        w4 = want.reshape(N, 4)
        assert not w4[flags == 0].any() and (w4[flags != 0, 3] == 1).all(), msg  # unflagged pixels: four zeros
        nonzero += int((w4[:, :3].sum(1) > 0).sum())
        if what == "sparse":  # through the gather of vertices (not the arrays the grid was built from: no triangle records)
            got = _gather(torch, whole, f, lens, flags, S, tile, table, shadow, dv=whole.dv.clone(), df=whole.df.clone())
            np.testing.assert_array_equal(got, want, err_msg=msg + ", no records")
    assert nonzero > N // 16


@pytest.mark.gpu
def test_launch_shapes_change_no_word(ugrt, O, DOF, torch):
    """any_rays_per_wave unset, 8 and 3, any_coop at 1 and 2^30, and dda_blocks = 1 (every later group from the ticket)."""
    W, H, _ = SIZES["hall"]
    f = frame(O, ugrt, "hall", W, H)
    d = TA._context(ugrt, f)
    flags = _sparse(f["N"], 5)
    lens, _ = lens_of(ugrt, f, 0.3)
    for S, tile in ((8, (4, 4)), (3, (2, 2))):
        table = _table(ugrt, S, tile)
        want = cpu_sums(DOF, f, lens, flags, S, tile, table, True)
        for rpw in (-1, 8, 3):
            for coop in (-1, 1, 1 << 30):
                d.ctx.set_option("any_rays_per_wave", rpw)
                d.ctx.set_option("any_coop", coop)
                np.testing.assert_array_equal(_gather(torch, d, f, lens, flags, S, tile, table, True), want,
                                              err_msg="S %d rays per wave %d, coop %d" % (S, rpw, coop))
        d.ctx.set_option("any_rays_per_wave", -1)
        d.ctx.set_option("any_coop", -1)
        d.ctx.set_option("dda_blocks", 1)
        np.testing.assert_array_equal(_gather(torch, d, f, lens, flags, S, tile, table, True), want, err_msg="one block")
        d.ctx.set_option("dda_blocks", -1)


@pytest.mark.gpu
def test_gather_under_the_strict_texture_rule(ugrt, O, DOF, torch):
    W, H = 64, 64
    f = frame(O, ugrt, "hall", W, H, strict=True)
    loose = frame(O, ugrt, "hall", W, H)
    d = TA._context(ugrt, f, flags=ugrt.FLAG_STRICT_TEXTURE)
    ones = np.ones(f["N"], np.int32)
    lens, _ = lens_of(ugrt, f, 0.3)
    table = _table(ugrt, 8, (2, 2))
    want = cpu_sums(DOF, f, lens, ones, 8, (2, 2), table, True)
    np.testing.assert_array_equal(_gather(torch, d, f, lens, ones, 8, (2, 2), table, True), want)
    assert (want != cpu_sums(DOF, loose, lens, ones, 8, (2, 2), table, True)).any()


@pytest.mark.gpu
def test_lens_points_outside_the_disk_and_lenses_at_the_edges_of_the_contract(ugrt, O, AA, DOF, torch):
    """A table with lu, lv at +-1, beyond +-1 and NaN; a view axis that points away from the view (the c <= 0 branch: the
    anti-aliasing's rays); a tiny and a huge F; a lens of radius 0 (ugrt_aa_gather's words on the same offsets)."""
    W, H = 64, 64
    f = frame(O, ugrt, "hall", W, H)
    N = f["N"]
    d = TA._context(ugrt, f)
    flags = _sparse(N, 2)
    v3 = _f32(f["scene"]["verts"]).reshape(-1, 3)
    extent = float((v3.max(0) - v3.min(0)).max())
    lens, _ = lens_of(ugrt, f, 0.3)
    S, tile = 8, (2, 2)
    offsets = ugrt.scenes.aa_offset_sets(S, 4)
    odd = with_lens(offsets)
    nan = float("nan")
    points = [(1, 1), (-1, -1), (1, -1), (-1, 1), (1.5, 0.25), (-7, 3), (nan, 0.5), (0.5, nan), (nan, nan), (np.inf, -np.inf), (0, 0),
              (1e-30, -1e-30)]
    for i in range(4 * S):
        odd.reshape(-1, 4)[i, 2:] = points[i % len(points)]
    want = cpu_sums(DOF, f, lens, flags, S, tile, odd, True)
    np.testing.assert_array_equal(_gather(torch, d, f, lens, flags, S, tile, odd, True), want)
    clamped = odd.copy()
    clamped[..., 2:] = np.clip(np.nan_to_num(odd[..., 2:], nan=0.0, posinf=1.0, neginf=-1.0), -1, 1)
    np.testing.assert_array_equal(cpu_sums(DOF, f, lens, flags, S, tile, clamped, True), want)  # the clamp is the contract's
    beyond = odd.copy()
    beyond[..., :2] = (0.75, nan)  # sx, sy as ugrt_aa_gather clamps them
    want = cpu_sums(DOF, f, lens, flags, S, tile, beyond, False)
    np.testing.assert_array_equal(_gather(torch, d, f, lens, flags, S, tile, beyond, False), want)
    table = ugrt.scenes.lens_sample_sets(S, 4)
    aa = TA.cpu_sums(AA, f, flags, S, tile, offsets, True)
    # A points away: the pinhole ray whatever the lens
    away = lens.copy()
    away[6:9] = -away[6:9]
    want = cpu_sums(DOF, f, away, flags, S, tile, table, True)
    np.testing.assert_array_equal(want, aa)
    np.testing.assert_array_equal(_gather(torch, d, f, away, flags, S, tile, table, True), want)
    for F in (1e-3 * extent, 1e6 * extent):
        far = lens.copy()
        far[9] = F
        want = cpu_sums(DOF, f, far, flags, S, tile, table, True)
        np.testing.assert_array_equal(_gather(torch, d, f, far, flags, S, tile, table, True), want, err_msg="F %g" % F)
        assert (want != aa).any()
    # the lens radius 0: the anti-aliasing's gather on the same offsets and flags, word for word
    lens0 = lens.copy()
    lens0[:6] = 0.0
    got = _gather(torch, d, f, lens0, flags, S, tile, table, True)
    np.testing.assert_array_equal(got, aa)
    np.testing.assert_array_equal(got, TA._gather(torch, d, f, flags, S, tile, d.ctx.upload(offsets.reshape(-1)), True))


def _make(ugrt, s, W, H):
    ctx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
    return ctx, ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])


APERTURE = {"hall": 0.15, "depth": 0.2}


@pytest.mark.gpu
@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("name", ["hall", "depth"])
def test_frames_equal_the_cpu_frames(ugrt, O, REFS, AO, AA, DOF, torch, name, shadows):
    """display(dof=4, ...) plain, with dof_sets=16 and with dof_shadows=False: image, dof_flag and dof_sum are the frame
    composed on the CPU from the oracle's frame plus the checker; with ao=4 behind it the image is the checker's scaled by
    the ambient occlusion's reference; dof_aperture=0 and a frame without the keyword are the frame as it was."""
    W = H = 128
    f = frame(O, ugrt, name, W, H, shadows=shadows)
    s, N, setup = f["scene"], f["N"], f["setup"]
    a = APERTURE[name]
    ctx, r = _make(ugrt, s, W, H)
    r.display(setup, shadows=shadows)
    ctx.synchronize()
    off = r.image.cpu().numpy().copy()
    np.testing.assert_array_equal(off, f["image"])
    assert r.dof_flag is None and r.dof_sum is None
    forms = [dict(dof=4), dict(dof=8, dof_sets=16)] + ([dict(dof=4, dof_shadows=False)] if shadows else [])
    for kw in forms:
        flags, sums, image = cpu_dof(DOF, AA, ugrt, f, kw["dof"], a, kw.get("dof_sets", 1), shadows, kw.get("dof_shadows", True))
        r.display(setup, shadows=shadows, dof_aperture=a, **kw)
        ctx.synchronize()
        np.testing.assert_array_equal(r.dof_flag.cpu().numpy(), flags, err_msg=str(kw))
        np.testing.assert_array_equal(_words(r.dof_sum), sums, err_msg=str(kw))
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), f["mat_ids"], err_msg=str(kw))
        np.testing.assert_array_equal(r.image.cpu().numpy(), image, err_msg=str(kw))
        assert int((image != off).sum()) > 1000 and 100 < int(flags.sum()) < N
    # ambient occlusion scales the finished image
    pr, verts, faces = f["primary"], _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    v3 = verts.reshape(-1, 3)
    radius = float(np.float32(0.05 * float((v3.max(0) - v3.min(0)).max())))
    orays, oactive = AO.rays(f["cam_pos"], pr["t"], pr["dir"], pr["id"], verts, faces, EPS, 0, N, N)
    mask = AM.cpu_mask(REFS[1], AO, f["ugrid"], s["verts"], s["faces"], orays, oactive, ugrt.scenes.ao_directions(4), radius, 0, N, N)
    r.display(setup, shadows=shadows, dof=4, dof_aperture=a, ao=4, ao_radius=radius)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), AO.shade(cpu_dof(DOF, AA, ugrt, f, 4, a, 1, shadows)[2], mask, 4, 0, N))
    # a lens of radius 0 flags nothing: the plain frame's bytes
    r.display(setup, shadows=shadows, dof=4, dof_aperture=0.0)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), off, err_msg="aperture 0")
    assert not r.dof_flag.cpu().numpy().any() and not _words(r.dof_sum).any()
    r.display(setup, shadows=shadows)
    ctx.synchronize()
    np.testing.assert_array_equal(r.image.cpu().numpy(), off, err_msg="behind a dof frame")


@pytest.mark.gpu
def test_a_second_call_after_a_camera_change_flags_again(ugrt, O, AA, DOF, torch):
    """The same renderer, a camera moved sideways and focused by dof_focus: flags, sums and image are the moved camera's."""
    W = H = 128
    s = frame(O, ugrt, "depth", W, H)["scene"]
    ctx, r = _make(ugrt, s, W, H)
    first = frame(O, ugrt, "depth", W, H)
    r.display(first["setup"], dof=4, dof_aperture=0.2)
    ctx.synchronize()
    np.testing.assert_array_equal(r.dof_flag.cpu().numpy(), cpu_dof(DOF, AA, ugrt, first, 4, 0.2)[0])
    moved = dict(s["cameras"]["ref"], eye=(1.0, 11.0, 3.0), look=(13.0, 14.0, 2.0))
    setup = ugrt.FrameSetup(moved, s["light_camera"], s["shading_light"])
    want = O.frame(s, setup, W, H, light_grid=LG, all_chunks=True)
    f2 = dict(first)
    f2.update(want)
    f2.update(setup=setup, cam_pos=want["cam"].worldori[:3].copy())
    flags, sums, image = cpu_dof(DOF, AA, ugrt, f2, 4, 0.2, focus=6.0, camera=moved)
    r.display(setup, dof=4, dof_aperture=0.2, dof_focus=6.0)
    ctx.synchronize()
    np.testing.assert_array_equal(r.dof_flag.cpu().numpy(), flags)
    np.testing.assert_array_equal(_words(r.dof_sum), sums)
    np.testing.assert_array_equal(r.image.cpu().numpy(), image)
    assert (flags != cpu_dof(DOF, AA, ugrt, first, 4, 0.2)[0]).any()


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, DOF, torch):
    W, H = 64, 64
    f = frame(O, ugrt, "hall", W, H)
    N = f["N"]
    fresh = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD)
    z = torch.zeros(6 * N, dtype=torch.int32, device=fresh.device)
    lens, coc_scale = lens_of(ugrt, f, 0.3)
    with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
        fresh.dof_gather(z, z, z, z, z, f["cam"].cc, lens, z, 4, 1, 1, z, z, z, 4, None, EPS, z)
    assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    d = TA._context(ugrt, f)
    ctx = d.ctx
    table = ugrt.scenes.lens_sample_sets(4, 4)
    d_table = ctx.upload(table.reshape(-1))
    ones = np.ones(N, np.int32)
    d_flags = ctx.upload(ones)
    sums = torch.full((4 * N + 4,), -1, dtype=torch.int32, device=ctx.device)
    flag = torch.full((N,), -1, dtype=torch.int32, device=ctx.device)
    light = f["lcam"].worldori[:3].copy()
    args = [d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, f["cam"].cc, lens, d_flags, 4, 2, 2, d_table, d.mat_idx, d.mat_list, d.nmat,
            light, EPS, sums[:4 * N]]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    def swap(a, h, v):
        return a[:h] + [v] + a[h + 1:]

    def lens_with(k, v):
        out = lens.copy()
        out[k] = v
        return out

    for bad in (0, 33, -1):
        fails(ctx.dof_gather, swap(args, 8, bad), b"num_samples")
    for bad in (0, 5):
        fails(ctx.dof_gather, swap(args, 9, bad), b"set_w")
        fails(ctx.dof_gather, swap(args, 10, bad), b"set_h")
    fails(ctx.dof_gather, swap(args, 16, float("nan")), b"eps")
    for bad in (0, -3):
        fails(ctx.dof_gather, swap(args, 14, bad), b"num_materials")
    fails(ctx.dof_gather, swap(args, 17, sums[1:4 * N + 1]), b"d_sum")
    for h in (0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 17):
        fails(ctx.dof_gather, swap(args, h, None), b"null")
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k, word in ((0, b"U[0]"), (2, b"U[2]"), (4, b"V[1]"), (6, b"A[0]"), (8, b"A[2]")):
            fails(ctx.dof_gather, swap(args, 6, lens_with(k, bad)), word)
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        fails(ctx.dof_gather, swap(args, 6, lens_with(9, bad)), b"lens F")
    p_args = [d.t, d.dir, d.ids, lens[6:9], float(lens[9]), coc_scale, 0.5, 4, flag]
    nan = float("nan")
    fails(ctx.dof_pixels, swap(p_args, 3, np.float32([1, nan, 0])), b"axis[1]")
    fails(ctx.dof_pixels, swap(p_args, 4, nan), b"focus")
    fails(ctx.dof_pixels, swap(p_args, 5, nan), b"coc_scale")
    fails(ctx.dof_pixels, swap(p_args, 6, nan), b"coc_min")
    for bad in (-1, 9):
        fails(ctx.dof_pixels, swap(p_args, 7, bad), b"radius")
    for h in (0, 1, 2, 3, 8):
        fails(ctx.dof_pixels, swap(p_args, h, None), b"null")
    ctx.synchronize()
    assert (_words(sums) == 0xFFFFFFFF).all() and (flag == -1).all()  # nothing ran
    want = cpu_sums(DOF, f, lens, ones, 4, (2, 2), table, True)
    np.testing.assert_array_equal(_gather(torch, d, f, lens, ones, 4, (2, 2), table, True), want)
    ctx.dof_pixels(*p_args)
    ctx.synchronize()
    np.testing.assert_array_equal(flag.cpu().numpy(), DOF.pixels(f["primary"], lens[6:9], float(lens[9]), coc_scale, 0.5, 4, W, H, 0, N))
