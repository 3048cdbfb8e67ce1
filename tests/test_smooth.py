"""Smooth shading: ugrt_smooth_adjacency, ugrt_smooth_corner_normals, ugrt_smooth_normals and
display(smooth=True), against tests/smooth_ref.c (one loop per corner, one per pixel) and numpy, to the bit.

  CPU  the checker on icospheres and on the welded box, scenes.weld, the legality of display(smooth=True) on the three
       renderer kinds and the calls a smooth frame enqueues.
  GPU  the adjacency against a stable argsort; the corner normals on a seeded soup with a hub and on a mesh of special
       faces; the shading normals on a synthetic 64 x 128 g-buffer; frames at 128 x 128 on scenes.smooth() and
       scenes.glass() against CPU frames composed by tests/frame_ref.py with the checker's normals in the place of the
       primary pass'; the caching; the errors.

The corner count 3F is a multiple of 3 and a power of two is not, so the sizes "around the sort's tile" are the nearest
multiples of 3 on both sides of it: 4095 and 4098 around 4096, 8190 and 8193 around 8192, each with tiles of 4096 and of
8192 pairs (option "sort_items")."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_ref as FR
import test_area_light as TA
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
import test_refract as RFR
import test_temporal as TT
from test_ambient import AO  # noqa: F401  (fixtures)
from test_ambient_sets import ASR  # noqa: F401
from test_antialias import AA  # noqa: F401
from test_area_light import AR  # noqa: F401
from test_filter_visibility import SR  # noqa: F401
from test_frame_matrix import K  # noqa: F401
from test_glossy import GL  # noqa: F401
from test_indirect import IR  # noqa: F401
from test_lights import LT  # noqa: F401
from test_reflect_lights import RL  # noqa: F401
from test_reflect_shadows import REFS  # noqa: F401
from test_refract import RF  # noqa: F401
from test_temporal import TR  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, bits, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.LG, RD.UD
CALLS = ("ugrt_smooth_adjacency", "ugrt_smooth_get_adjacency", "ugrt_smooth_corner_normals", "ugrt_smooth_normals")
W = H = 128
N = W * H


class SmoothRef:
    def __init__(self, lib):
        self.lib = lib

    def adjacency(self, faces, V, key=None):
        faces = _i32(faces).reshape(-1)
        corners, start = np.zeros(len(faces), np.uint32), np.zeros(V + 1, np.uint32)
        self.lib.smooth_adjacency(_p(faces), C.c_int(len(faces) // 3), C.c_int(V), None if key is None else _p(_i32(key)),
                                  _p(corners), _p(start))
        return corners, start

    def corner_normals(self, faces, verts, cos, key=None):
        faces, verts = _i32(faces).reshape(-1), _f32(verts).reshape(-1)
        corners, start = self.adjacency(faces, len(verts) // 3, key)
        out = np.zeros(3 * len(faces), np.float32)
        self.lib.smooth_corner_normals(_p(faces), _p(verts), C.c_int(len(faces) // 3), None if key is None else _p(_i32(key)),
                                       _p(corners), _p(start), C.c_float(cos), _p(out))
        return out

    def normals(self, t, dirs, ids, cam_pos, verts, faces, cn, normal_in, fold, p0, n, out=None):
        """The words behind ugrt_smooth_normals over pixels p0 .. p0 + n - 1; out: what the buffer held before (a copy is
        written; None: normal_in itself, the call in place)."""
        out = _f32(normal_in).copy() if out is None else _f32(out).copy()
        self.lib.smooth_normals(_p(_f32(t)), _p(_f32(dirs)), _p(_i32(ids)), _p(_f32(cam_pos)), _p(_f32(verts).reshape(-1)),
                                _p(_i32(faces).reshape(-1)), _p(_f32(cn)), _p(_f32(normal_in)), C.c_int(fold), _p(out),
                                C.c_int(p0), C.c_int(n))
        return out


@pytest.fixture(scope="session")
def SM(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("smooth_ref") / "libsmooth_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "smooth_ref.c"), "-lm"], check=True, capture_output=True)
    return SmoothRef(C.CDLL(out))


def box(ugrt):
    m = ugrt.scenes.Mesh()
    ugrt.scenes.add_box(m, (0.5, -1.0, 2.0), (1.5, 0.25, 3.0), 2, 0)
    v, f, _ = m.arrays()
    return v.astype(np.float32), f


def assert_same(got, want, what=""):
    """Floats to the bit; where the checker holds a NaN the device holds a NaN (a NaN's sign and payload are no value: the
    invalid operations of the checker's x86 give 0xFFC00000, the GPU's 0x7FC00000)."""
    got, want = _f32(got).reshape(-1), _f32(want).reshape(-1)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    wrong = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    assert not wrong.any(), "%s: %d of %d words differ, first at %d: %r, checker %r" % (
        what, int(wrong.sum()), wrong.size, int(np.flatnonzero(wrong)[0]), got[wrong][0], want[wrong][0])


def face_normals(verts, faces):
    """float64, for the properties (never compared to the bit)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)[np.asarray(faces).reshape(-1, 3)]
    with np.errstate(all="ignore"):  # (a zero-area face, a NaN vertex: their rows are NaN)
        a = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        return a / np.sqrt((a * a).sum(1))[:, None]


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    header = open(os.path.join(RD.ROOT, "include", "ugrt.h")).read()
    for name in CALLS:
        assert hasattr(lib, name) and name in ugrt.PROTOTYPES and name + "(" in header
        assert callable(getattr(ugrt.Context, name[5:]))
    assert lib.ugrt_version() == 105


@pytest.mark.parametrize("level", [1, 2, 3])
def test_on_an_icosphere_every_corner_normal_is_closer_to_the_radius_than_its_face_normal(ugrt, SM, level):
    v, f = ugrt.scenes.icosphere(level)
    v, f = ugrt.scenes._wind_outwards(v * 1.5, f)
    cn = SM.corner_normals(f, v.astype(np.float32), -1.0).astype(np.float64).reshape(-1, 3)
    radial = v[f.reshape(-1)] / np.sqrt((v[f.reshape(-1)] ** 2).sum(1))[:, None]
    nf = np.repeat(face_normals(v.astype(np.float32), f), 3, 0)
    assert np.isfinite(cn).all()
    assert ((cn * radial).sum(1) > (nf * radial).sum(1)).all()
    # all the corners of a vertex hold one normal, bit for bit: the same list, the same order
    for vert in (0, 5, len(v) - 1):
        rows = bits(cn.astype(np.float32))[f.reshape(-1) == vert]
        assert len(rows) >= 5 and (rows == rows[0]).all()


def test_the_welded_box_keeps_its_edges_at_half(ugrt, SM):
    v, f = box(ugrt)
    key = ugrt.scenes.weld(v)
    cn = SM.corner_normals(f, v, 0.5, key).reshape(-1, 3)
    nf = np.repeat(face_normals(v, f), 3, 0).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(nf), np.float32(2.0 ** -24)).astype(np.float32))
    assert (np.abs(cn - nf) <= 2 * ulp).all()
    # and every face of a welded vertex counts at -1: the corners of the box's corners leave their faces' normals
    away = SM.corner_normals(f, v, -1.0, key).reshape(-1, 3)
    assert (np.abs(away - nf).max(1) > 0.1).sum() >= 8 * 3
    # without the weld every vertex stands alone on its side of the box
    alone = SM.corner_normals(f, v, -1.0).reshape(-1, 3)
    assert (np.abs(alone - nf) <= 2 * ulp).all()


def test_weld(ugrt):
    weld = ugrt.scenes.weld
    v, f = box(ugrt)
    key = weld(v)
    assert key.dtype == np.int32 and key.shape == (54,) and len(set(key)) == 26
    assert (key <= np.arange(54)).all() and (key[key] == key).all()
    assert all(np.array_equal(v[i], v[k]) for i, k in enumerate(key))
    m = ugrt.scenes.Mesh()
    ugrt.scenes.add_cylinder(m, 0.0, 0.0, 0.0, 1.0, 0.45, 32, 4, 3, flutes=8)
    cv = m.arrays()[0].astype(np.float32)
    assert len(cv) == 165 and len(set(weld(cv))) == 165          # sin(2 pi) is not 0: the seam columns differ in their last bits
    k5 = weld(cv, 1e-5)
    assert len(set(k5)) == 160 and (k5[-5:] == np.arange(5)).all() and (k5[:-5] == np.arange(160)).all()
    z = np.float32([[0.0, 0.0, 1.0], [-0.0, 0.0, 1.0], [0.0, -0.0, 1.0], [0.0, 0.0, -1.0], [-0.0, -0.0, 1.0]])
    assert list(weld(z)) == [0, 0, 0, 3, 0] and list(weld(z, 1e-3)) == [0, 0, 0, 3, 0]
    assert list(weld(np.float32([[1, 2, 3], [1, 2, 3 + 1e-6], [1, 2, 3]]))) == [0, 1, 0]
    assert list(weld(np.float32([[1, 2, 3], [1, 2, 3 + 1e-6], [1, 2, 3]]), 1e-3)) == [0, 0, 0]
    assert weld(np.zeros((0, 3), np.float32)).shape == (0,)
    with pytest.raises(ValueError):
        weld(v, -1.0)
    s = ugrt.scenes.smooth(scale=0.1)
    assert np.array_equal(s["vertex_key"], weld(s["verts"], 1e-5)) and set(s["objects"]) == {"sphere", "cylinder", "box"}
    a, b = s["objects"]["sphere"]
    assert b - a == 320 and s["objects"]["box"][1] == s["num_faces"]


def _fake(ugrt):
    r = TT._fake(ugrt)
    r.__dict__.update(snormal="snormal", corner_normals="cn")
    r._smooth_stage = lambda cos: r.ctx.calls.append(("smooth_stage", cos))
    return r


def test_smooth_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    chk = rmod.check_smooth
    assert chk(False) is None and chk(np.bool_(False), 0.5, False) is None
    assert chk(True) == (0.5, False) and chk(True, -1, np.bool_(True)) == (-1.0, True) and chk(True, np.float32(2)) == (2.0, False)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError):
            chk(bad)
        with pytest.raises(ValueError):
            chk(True, 0.5, bad)
    for bad in (float("nan"), "0.5", None, True):
        with pytest.raises(ValueError):
            chk(True, bad)
    for kw in (dict(smooth_cos=0.7), dict(smooth_signed=True)):  # a value away from its default needs smooth
        with pytest.raises(ValueError):
            chk(False, **kw)
    for kw in (dict(reflect=True), dict(reflect=True, refract=True), dict(glossy=4), dict(aa=4), dict(reflect_lights=True),
               dict(two_streams=True)):
        with pytest.raises(ValueError):
            chk(True, **kw)
        assert chk(False, **kw) is None
    s = RD.scene(ugrt, "hall")
    single, multi = TL.setup_for(ugrt, s), TL.setup_for(ugrt, s, TL.lights_for(s, 2))
    illegal = (dict(reflect=True), dict(reflect=True, refract=True), dict(reflect=True, bounces=3, reflect_shadows=True),
               dict(glossy=4), dict(aa=4), dict(aa=4, ao=4, ao_radius=1.0), dict(smooth_cos=float("nan")), dict(smooth_signed=1))
    for kw in illegal:
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(single, smooth=True, **kw)
        assert r.ctx.calls == [] and r.cleared == [], kw
    for kw in (dict(smooth_cos=0.7), dict(smooth_signed=True), dict(smooth=1)):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(single, **kw)
        assert r.ctx.calls == []
    r = _fake(ugrt)
    with pytest.raises(ValueError):
        r.display(multi, smooth=True, reflect=True, reflect_lights=True)
    assert r.ctx.calls == []
    for kw in (dict(), dict(frame_cnt=2), dict(shadows=False), dict(ao=4, ao_radius=1.0)):  # the two-stream renderer
        r = _fake(ugrt)
        r.aux = object()
        with pytest.raises(ValueError):
            r.display(single, smooth=True, **kw)
        assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    for kw in (dict(smooth=True), dict(smooth=True, reflect=False), dict(smooth_cos=0.7), dict(smooth_signed=True)):
        with pytest.raises(ValueError):
            br.display(single, **kw)


def test_the_design_table_is_what_check_smooth_says(ugrt):
    chk = RLT._rmod(ugrt).check_smooth
    rows = (("plain", dict()), ("plain, frame_cnt 2", dict()), ("shadows=False", dict()), ("reflect", dict(reflect=True)),
            ("reflect + refract", dict(reflect=True, refract=True)), ("setup.lights", dict()),
            ("reflect_lights", dict(reflect=True, reflect_lights=True)), ("two-stream", dict(two_streams=True)),
            ("banded", dict(two_streams=True)), ("glossy", dict(glossy=8)), ("area", dict()), ("gi", dict()), ("aa", dict(aa=4)),
            ("ao", dict()), ("temporal", dict()))
    text = open(os.path.join(RD.ROOT, "DESIGN.md")).read()
    want = ["| with | smooth |", "|---|---|"]
    for name, kw in rows:
        try:
            chk(True, **kw)
            want.append("| %s | yes |" % name)
        except ValueError:
            want.append("| %s | - |" % name)
    assert "\n".join(want) + "\n" in text
    doc = " ".join(ugrt.Renderer.display.__doc__.split())
    assert "smooth (one-stream renderer; the plain frame, frame_cnt=2, shadows=False and setup.lights; ao, area, gi and " \
           "temporal compose; no reflect, refract, glossy, aa or reflect_lights" in doc


def test_a_smooth_frame_enqueues_one_pass_before_its_shading_call_and_the_default_frame_nothing(ugrt):
    s = RD.scene(ugrt, "hall")
    single, multi = TL.setup_for(ugrt, s), TL.setup_for(ugrt, s, TL.lights_for(s, 2))
    names = TA._names
    frames = ((single, dict(), "shade_simple"), (single, dict(frame_cnt=2), "shade_spotlight"),
              (single, dict(shadows=False), "shade_simple"), (multi, dict(), "shade_lights"),
              (single, dict(ao=4, ao_radius=1.0), "shade_simple"), (single, dict(area=5, area_radius=0.5), "shade_simple"),
              (single, dict(gi=8, gi_filter=2), "shade_simple"), (single, dict(ao=4, ao_radius=1.0, temporal=4), "shade_simple"),
              (multi, dict(ao=4, ao_radius=1.0), "shade_lights"))
    for setup, kw, shade in frames:
        a, b, c = TT._fake(ugrt), TT._fake(ugrt), _fake(ugrt)
        a.display(setup, **kw)
        b.display(setup, smooth=False, smooth_cos=0.5, smooth_signed=False, **kw)
        assert names(a) == names(b) and not [k for k in vars(b) if "smooth" in k or k in ("snormal", "corner_normals")]
        c.display(setup, smooth=True, smooth_cos=0.25, **kw)
        at = names(c).index(shade)
        assert names(c)[:at - 2] + names(c)[at:] == names(a), kw
        assert c.ctx.calls[at - 2] == ("smooth_stage", 0.25)
        assert c.ctx.calls[at - 1] == ("smooth_normals", "t", "d", "ids", "cam", "v", "f", "cn", "n", True, "snormal"), kw
        flat = a.ctx.calls[at - 2]
        assert flat[0] == shade and flat[2] == "n" and c.ctx.calls[at][2] == "snormal"
        plain = lambda call: [x for x in call[:2] + call[3:] if isinstance(x, (str, int, float))]  # (the lights' rows are objects)
        assert plain(c.ctx.calls[at]) == plain(flat) and len(c.ctx.calls[at]) == len(flat)
        # nothing else reads the new buffer
        assert sum("snormal" in [x for x in call if isinstance(x, str)] for call in c.ctx.calls) == 2
        c = _fake(ugrt)
        c.display(setup, smooth=True, smooth_signed=True, shade=False, **kw)
        assert names(c) == names(b)[:len(names(c))] and "smooth_normals" not in names(c)
    c = _fake(ugrt)
    c.display(single, smooth=True, smooth_signed=True)
    assert [x for x in c.ctx.calls if x[0] == "smooth_normals"][0][9] is False


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _small_context(ugrt, rows=None, flags=0):
    return ugrt.Context(64, 128, light_grid=(16, 16), uniform_dims=(8, 8, 8), rows=rows, flags=flags)


def _gpu_adjacency(ctx, faces, V, key):
    faces = _i32(faces).reshape(-1)
    ctx.smooth_adjacency(ctx.upload(faces) if len(faces) else None, len(faces) // 3, V, None if key is None else ctx.upload(_i32(key)))
    ctx.synchronize()
    corners, start = ctx.smooth_get_adjacency()
    return _words(corners), _words(start)


def _np_adjacency(faces, V, key):
    faces = _i32(faces).reshape(-1)
    keys = faces if key is None else _i32(key)[faces]
    corners = np.argsort(keys, kind="stable").astype(np.uint32)
    return corners, np.searchsorted(keys[corners], np.arange(V + 1)).astype(np.uint32)


def _hub(n):
    """n faces around vertex 0: (0, i + 1, i + 2)."""
    i = np.arange(n, dtype=np.int32)
    return np.stack([np.zeros(n, np.int32), i + 1, i + 2], 1)


@pytest.mark.gpu
def test_adjacency_equals_a_stable_argsort(ugrt, SM, torch):
    rng = np.random.RandomState(615)
    cases = [("V = 1", np.zeros((5, 3), np.int32), 1), ("F = 0", np.zeros((0, 3), np.int32), 7), ("F = 0, V = 0", np.zeros((0, 3), np.int32), 0),
             ("F = 1", np.int32([[2, 0, 1]]), 3), ("unused vertices", 2 * rng.randint(0, 50, (300, 3)), 100),
             ("a face (a, a, b)", np.int32([[3, 3, 1], [1, 3, 3], [0, 1, 2], [3, 1, 3]]), 5), ("a hub of 4096", _hub(4096), 4098)]
    for F in (1365, 1366, 2730, 2731):  # 3F = 4095, 4098, 8190, 8193
        cases.append(("3F = %d" % (3 * F), rng.randint(0, 700, (F, 3)), 700))
    for V in (255, 256, 257, 65537):  # 8, 8, 9 and 17 key bits: one, one, two and three passes
        f = rng.randint(0, V, (2000, 3))
        f[0, 0], f[1, 1] = V - 1, 0
        cases.append(("V = %d" % V, f, V))
    ctx = _small_context(ugrt)
    builds = 0
    for items in (8, 16):
        ctx.set_option("sort_items", items)
        for what, faces, V in cases:
            tables = [None]
            if V:
                tables += [rng.randint(0, V, V), np.zeros(V, np.int32), ugrt.scenes.weld(rng.randint(0, 3, (V, 3)).astype(np.float32))]
            for key in tables:
                want = _np_adjacency(faces, V, key)
                got = _gpu_adjacency(ctx, faces, V, key)
                builds += 1
                where = "%s, tiles of %d, %s" % (what, 512 * items, "no table" if key is None else "a table")
                np.testing.assert_array_equal(got[0], want[0], err_msg=where)
                np.testing.assert_array_equal(got[1], want[1], err_msg=where)
                ref = SM.adjacency(faces, V, key)
                assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[1], want[1]), where
    assert ctx.get_state("smooth_adjacency_builds") == builds and ctx.get_state("smooth_normal_builds") == 0


def _gpu_corner_normals(torch, ctx, faces, verts, cos, key, adjacency=True):
    faces, verts = _i32(faces).reshape(-1), _f32(verts).reshape(-1)
    df, dv = ctx.upload(faces), ctx.upload(verts)
    if adjacency:
        ctx.smooth_adjacency(df, len(faces) // 3, len(verts) // 3, None if key is None else ctx.upload(_i32(key)))
    out = torch.full((3 * len(faces),), float("nan"), dtype=torch.float32, device=ctx.device)
    ctx.smooth_corner_normals(df, dv, len(faces) // 3, cos, out)
    ctx.synchronize()
    return out.cpu().numpy()


def soup(seed=616, F=20000 - 4096, V=6000):
    """A seeded soup with a hub of valence 4096 behind it, and a key table that welds a tenth of the vertices."""
    rng = np.random.RandomState(seed)
    verts = rng.uniform(-1, 1, (V + 4098, 3)).astype(np.float32)
    faces = np.concatenate([rng.randint(0, V, (F, 3)), _hub(4096) + V]).astype(np.int32)
    key = np.arange(V + 4098, dtype=np.int32)
    pick = rng.choice(V, V // 10, replace=False)
    key[pick] = np.minimum(pick, rng.randint(0, V, V // 10))
    key = key[key]  # (a key is its own key)
    return verts, faces, np.minimum(key, key[key])


@pytest.mark.gpu
@pytest.mark.parametrize("cos", [-1.0, 0.5, 1.0, 2.0])
def test_corner_normals_on_a_soup_with_a_hub(ugrt, SM, torch, cos):
    verts, faces, key = soup()
    ctx = _small_context(ugrt)
    for table in (None, key):
        want = SM.corner_normals(faces, verts, cos, table)
        got = _gpu_corner_normals(torch, ctx, faces, verts, cos, table)
        assert_same(got, want, "cos %g" % cos)
    nf = np.repeat(face_normals(verts, faces), 3, 0)
    mixed = (np.abs(want.reshape(-1, 3) - nf).max(1) > 1e-3).mean()
    assert (mixed > 0.5) if cos <= 0.5 else (mixed < 0.02), mixed  # (a random neighbour lies within 60 degrees one time in four)
    assert ctx.get_state("smooth_normal_builds") == 2


def _f32_dot_of_unit_normals(verts, fa, fb):
    """N_a . N_b of two faces in the specification's fp32 operations (numpy float32 scalars: one rounding per operation)."""
    def unit(f):
        v0, v1, v2 = (verts[i].astype(np.float32) for i in f)
        a, b = v1 - v0, v2 - v0
        A = np.float32([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        return A * (np.float32(1.0) / np.sqrt(A[0] * A[0] + A[1] * A[1] + A[2] * A[2]))
    a, b = unit(fa), unit(fb)
    return np.float32((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def specials():
    """Faces at the edges of the arithmetic.  Returns (verts, faces, the fold: two faces over a shared edge)."""
    inf, nan = np.inf, np.nan
    v = [(0, 0, 0), (1, 0, 0), (0.3, 1, 0), (0.4, -0.8, 0.7),                       # 0-3: the fold (0,1,2) / (1,0,3)
         (5, 5, 5), (6, 5, 5), (7, 5, 5), (5, 6, 5.5),                               # 4-7: collinear (4,5,6), (a,a,b), a good face
         (nan, 0, 0), (inf, 1, 0), (-inf, 1, 2), (2, 2, 2), (2, 3, 2), (3, 2, 2),    # 8-13: NaN and infinite vertices
         (9, 9, 9), (9 + 1e-20, 9, 9), (0, 0, 0), (1e-20, 0, 0), (0, 1e-20, 0), (0, 0, 1e-20),  # 14-19: edges of 1e-20
         (1e19, 0, 0), (0, 1e19, 0), (0, 0, 1e19), (-1e19, -1e19, 0),                # 20-23: edges of 1e19
         (10, 0, 0), (11, 0, 0), (10, 1, 0), (10, 0, 1)]                             # 24-27: opposite faces
    f = [(0, 1, 2), (1, 0, 3),
         (4, 5, 6), (4, 4, 7), (4, 5, 7), (7, 7, 7),
         (8, 11, 12), (9, 11, 13), (10, 12, 13), (11, 12, 13), (9, 10, 8),
         (16, 17, 18), (16, 18, 19), (17, 18, 19), (14, 15, 16),
         (20, 21, 22), (20, 22, 23), (21, 20, 23), (16, 20, 21),
         (24, 25, 26), (24, 26, 25), (24, 25, 27), (25, 24, 27)]
    return np.float32(v), np.int32(f), ((0, 1, 2), (1, 0, 3))


@pytest.mark.gpu
def test_corner_normals_at_the_edges_of_the_arithmetic(ugrt, SM, torch):
    verts, faces, fold = specials()
    d = _f32_dot_of_unit_normals(verts, *fold)
    assert 0.0 < d < 1.0
    up, down = np.nextafter(d, np.float32(2)), np.nextafter(d, np.float32(-2))
    ctx = _small_context(ugrt)
    results = {}
    for cos in (-1.0, 0.5, 1.0, 2.0, float(d), float(up), float(down), -0.0, np.float32(-1.0000001), np.float32(1.0000001), float("inf"),
                float("-inf")):
        want = SM.corner_normals(faces, verts, cos)
        got = _gpu_corner_normals(torch, ctx, faces, verts, cos, None)
        assert_same(got, want, "cos %r" % cos)
        results[float(cos)] = want.reshape(-1, 3)
    nf = face_normals(verts, faces)
    # the threshold itself and the float below it take the neighbour in, the float above leaves the face alone
    for cos, joined in ((float(d), True), (float(down), True), (float(up), False)):
        c = results[cos][0]  # corner (face 0, vertex 0): the fold's faces meet there
        assert (np.abs(c - nf[0]).max() > 1e-2) == joined, cos
    # opposite faces: the sum has no direction and the corner keeps its face's normal; alone (2) it is the face's anyway
    lo = results[-1.0].reshape(-1, 3, 3)
    assert np.array_equal(bits(lo[19, 1]), bits(results[2.0].reshape(-1, 3, 3)[19, 1]))
    assert np.isnan(lo[19, 2]).sum() == 0 and np.abs(lo[19, 1] - nf[19]).max() < 1e-6
    # a zero-area face has a NaN normal and keeps it; edges of 1e19: the squares overflow, 1 / inf = 0 and the normal is
    # zero, which is finite and stays; edges of 1e-20: the cross product is a denormal, its square 0 and 1 / 0 = inf, so the
    # normal is (0 * inf, 0 * inf, denormal * inf) = (NaN, NaN, inf), the face's own as it is
    own = results[2.0].reshape(-1, 3, 3)
    assert np.isnan(own[2]).all() and (own[15] == 0).all() and np.isfinite(own[9]).all()
    assert np.isnan(own[11][:, :2]).all() and (own[11][:, 2] == np.inf).all()


def gbuffer(seed=617):
    """A synthetic g-buffer of 64 x 128 pixels over a seeded soup: directions through a point of the pixel's triangle (a
    tenth of them through a point well outside it: u, v are not clamped), every eighth pixel edge-on (the direction is the
    triangle's second edge: the determinant is exactly 0), ids below 0, every kind of t, and corner normals that are NaN,
    zero or opposed to the triangle's own.  Computed once and shared: nobody writes to it."""
    if _G:
        return _G
    rng = np.random.RandomState(seed)
    Wg, Hg, F, V = 64, 128, 500, 300
    n = Wg * Hg
    verts = rng.uniform(-2, 2, (V, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    cam = np.float32([0.3, -5.0, 0.7])
    ids = rng.randint(0, F, n).astype(np.int32)
    tri = verts[faces[ids]].astype(np.float64)
    bary = rng.dirichlet([1, 1, 1], n)
    out = rng.uniform(size=n) < 0.1
    bary[out] = rng.uniform(-2, 3, (int(out.sum()), 3))
    point = (bary[:, :, None] * tri).sum(1) / np.maximum(np.abs(bary.sum(1)), 0.1)[:, None]
    dirs = point - cam
    dirs /= np.sqrt((dirs * dirs).sum(1))[:, None]
    dirs = dirs.astype(np.float32)
    edge_on = np.arange(n) % 8 == 3
    dirs[edge_on] = (verts[faces[ids, 2]] - verts[faces[ids, 0]])[edge_on]
    ids[rng.choice(n, n // 10, replace=False)] = rng.choice([-1, -2, -2 ** 31], n // 10)
    t = rng.uniform(0.5, 9.0, n).astype(np.float32)
    odd = np.float32([np.nan, 0.0, -0.0, 1e-42, np.inf, -3.0, -np.inf, -1e-42])
    pick = rng.choice(n, n // 5, replace=False)
    t[pick] = odd[rng.randint(0, len(odd), len(pick))]
    a = verts[faces]
    flat = np.cross(a[:, 1] - a[:, 0], a[:, 2] - a[:, 0]).astype(np.float64)
    flat /= np.sqrt((flat * flat).sum(1))[:, None]
    cn = flat[:, None, :] + np.clip(rng.normal(0, 0.3, (F, 3, 3)), -0.5, 0.5)  # (on the side of the triangle's own)
    cn /= np.sqrt((cn * cn).sum(2))[:, :, None]
    cn = cn.astype(np.float32)
    cn[0:30] *= -1                      # opposed to the triangle's own normal
    cn[30:50, 1] = np.nan               # one corner NaN
    cn[50:70] = 0.0                     # all zero: the mix has no direction
    cn[70:80, 0, 2] = np.inf
    cn[80:90] = np.float32(1e30)        # the squares overflow
    cn[90:100] = -flat[90:100, None, :] * np.float32(1e-30)  # the squares underflow
    normal_in = rng.uniform(-1, 1, 3 * n).astype(np.float32)
    _G.update(outside=out, W=Wg, H=Hg, N=n, verts=verts.reshape(-1), faces=faces.reshape(-1), cam=cam, ids=ids, t=t, dirs=dirs.reshape(-1),
              cn=cn.reshape(-1), normal_in=normal_in, edge_on=edge_on)
    return _G


_G = {}


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [0, 1])
def test_shading_normals_on_a_synthetic_gbuffer(ugrt, SM, torch, fold):
    g = gbuffer()
    n = g["N"]
    hit = (g["ids"] >= 0) & (g["t"] > 0)
    want = SM.normals(g["t"], g["dirs"], g["ids"], g["cam"], g["verts"], g["faces"], g["cn"], g["normal_in"], fold, 0, n,
                      out=np.full(3 * n, 7.0, np.float32))
    # the checker's words are what the section says
    w3, in3 = want.reshape(-1, 3), g["normal_in"].reshape(-1, 3)
    assert np.array_equal(bits(w3[~hit]), bits(in3[~hit])) and 1000 < int((~hit).sum()) < n - 1000
    ng = np.repeat(face_normals(g["verts"], g["faces"]), 1, 0)[np.maximum(g["ids"], 0)]
    own = np.abs(np.abs(w3.astype(np.float64)) - np.abs(ng)).max(1) < 1e-5
    assert own[hit & g["edge_on"]].all() and 100 < int((hit & ~own).sum())
    for f in (range(0, 30), range(30, 50), range(50, 70), range(80, 100)):  # (outside the triangle a weight is negative)
        assert own[hit & ~g["outside"] & np.isin(g["ids"], list(f))].all()
    assert np.isfinite(w3[hit]).all() and (fold == 0 or (w3[hit] >= 0).all()) and (fold == 1 or (w3[hit] < 0).any())
    ctx = _small_context(ugrt)
    d = {k: ctx.upload(g[k]) for k in ("t", "dirs", "ids", "cam", "verts", "faces", "cn", "normal_in")}
    out = torch.full((3 * n,), 7.0, dtype=torch.float32, device=ctx.device)
    ctx.smooth_normals(d["t"], d["dirs"], d["ids"], d["cam"], d["verts"], d["faces"], d["cn"], d["normal_in"], fold, out)
    ctx.synchronize()
    assert_same(out.cpu().numpy(), want, "fold %d" % fold)
    np.testing.assert_array_equal(bits(d["normal_in"].cpu().numpy()), bits(g["normal_in"]))
    # in place
    buf = d["normal_in"].clone()
    ctx.smooth_normals(d["t"], d["dirs"], d["ids"], d["cam"], d["verts"], d["faces"], d["cn"], buf, fold, buf)
    ctx.synchronize()
    assert_same(buf.cpu().numpy(), want, "in place")
    # a band: the rows outside keep the fill
    band = _small_context(ugrt, rows=(3, 11))
    p0, m = 3 * 8 * g["W"], 8 * 8 * g["W"]
    assert (band.p0, band.npix) == (p0, m)
    db = {k: band.upload(g[k]) for k in ("t", "dirs", "ids", "cam", "verts", "faces", "cn", "normal_in")}
    out = torch.full((3 * n,), 7.0, dtype=torch.float32, device=band.device)
    band.smooth_normals(db["t"], db["dirs"], db["ids"], db["cam"], db["verts"], db["faces"], db["cn"], db["normal_in"], fold, out)
    band.synchronize()
    banded = SM.normals(g["t"], g["dirs"], g["ids"], g["cam"], g["verts"], g["faces"], g["cn"], g["normal_in"], fold, p0, m,
                        out=np.full(3 * n, 7.0, np.float32))
    assert_same(out.cpu().numpy(), banded, "a band")
    assert (banded[:3 * p0] == 7.0).all() and (banded[3 * (p0 + m):] == 7.0).all()
    np.testing.assert_array_equal(bits(banded[3 * p0:3 * (p0 + m)]), bits(want[3 * p0:3 * (p0 + m)]))


# ------------------------------------------------------------------------------------------------------------- frames

_SCENES = {}


def scene(ugrt, name):
    if name not in _SCENES:
        if name == "smooth":
            s = ugrt.scenes.smooth(scale=0.1)
        else:
            s = dict(RFR.scene(ugrt, "glass"))
            s["vertex_key"] = ugrt.scenes.weld(s["verts"], 1e-5)
        _SCENES[name] = s
    return _SCENES[name]


_FRAMES = {}


def frames(K, name):
    if name not in _FRAMES:
        _FRAMES[name] = FR.Frames(K, scene(K.ugrt, name), W, H)
    return _FRAMES[name]


def smooth_frames(SM, F, setup, cos, signed=False):
    """F with the checker's shading normals in the place of the primary pass' normals, for frame_ref's shading call: a copy
    whose cache holds F's words (they do not depend on the normal the shading call reads) and nothing shaded."""
    P = FR.primary(F, setup)
    pr, s = P["pr"], F.scene
    cn = F.once(("corner normals", cos), lambda: SM.corner_normals(s["faces"], s["verts"], cos, s["vertex_key"]))
    sn = SM.normals(pr["t"], pr["dir"], pr["id"], P["cam_pos"], F.verts, F.faces, cn, pr["normal"], 0 if signed else 1, 0, F.N)
    F2 = copy.copy(F)
    F2.cache = {k: v for k, v in F.cache.items() if k[0] != "shaded"}
    F2.cache[("primary", FR._setup_key(setup))] = dict(P, pr=dict(pr, normal=sn))
    return F2, sn, cn


def make(F, flags=0, key=True):
    u, s = F.K.ugrt, F.scene
    ctx = u.Context(F.W, F.H, light_grid=LG, flags=u.FLAG_SHADOW_ALL_CHUNKS | flags, uniform_dims=UD)
    return ctx, u.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], s["transmit"], s["ior"],
                           vertex_key=s["vertex_key"] if key else None)


def radii(F):
    return dict(ao_radius=float(np.float32(0.10 * F.extent)), area_radius=float(np.float32(0.25 * F.extent)))


BASES = (("plain", dict(), False), ("frame_cnt 2", dict(frame_cnt=2), False), ("shadows=False", dict(shadows=False), False),
         ("setup.lights", dict(), True))
EFFECTS = (("none", dict()), ("ao", dict(ao=8)), ("area", dict(area=5)), ("gi", dict(gi=8)), ("temporal + ao", dict(ao=8, temporal=4)))


def legal_frames(F):
    out = []
    for base_name, base, lights in BASES:
        for effect_name, effect in EFFECTS:
            kw = dict(base, **effect)
            if FR.legal(dict({n: v for n, v in kw.items() if n in FR.DEFAULTS}, lights=lights)):
                r = radii(F)
                kw.update({n: r[n] for n in r if kw.get(n[:-7])})
                out.append((base_name + ", " + effect_name, kw, lights))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["smooth", "glass"])
def test_smooth_frames_equal_the_cpu_frames(ugrt, SM, K, torch, name):
    """display(smooth=True) on every legal base, alone and with ao, area, gi and temporal + ao: everything the frame leaves
    behind is frame_ref's with the checker's normals in the shading call, and everything but the image is the smooth=False
    frame's."""
    F = frames(K, name)
    s = F.scene
    single = F.setup
    multi = ugrt.FrameSetup.from_scene(s, lights=TL.lights_for(s, 2))
    todo = legal_frames(F)
    assert len(todo) == 5 + 5 + 4 + 2  # (no area without shadows; under setup.lights ao alone)
    ctx, r = make(F)
    changed = 0
    for what, kw, lights in todo:
        setup = multi if lights else single
        chain = lambda: dict(chain=FR.Chain()) if kw.get("temporal") else {}
        flat_want = FR.cpu_display(F, setup, **chain(), **kw)
        r.display(setup, **kw)
        ctx.synchronize()
        flat = FR.device_frame(r, setup, **kw)
        assert FR.differences(flat_want, flat) == [], what
        F2, sn, cn = smooth_frames(SM, F, setup, 0.5)
        want = FR.cpu_display(F2, setup, **chain(), **kw)
        if kw.get("temporal"):
            r.display(setup, shade=False)  # (a frame that is no temporal one: the sequence starts again, as the Chain does)
        r.display(setup, smooth=True, **kw)
        ctx.synchronize()
        got = FR.device_frame(r, setup, **kw)
        assert FR.differences(want, got) == [], what
        assert_same(r.snormal.cpu().numpy(), sn, what)
        assert_same(r.corner_normals.cpu().numpy(), cn, what)
        np.testing.assert_array_equal(bits(r.normal.cpu().numpy()), bits(FR.primary(F, setup)["pr"]["normal"]), err_msg=what)
        assert FR.differences({k: v for k, v in flat.items() if k != "image"}, got) == [], what
        changed += int((want["image"] != flat_want["image"]).any())
    assert changed == len(todo)
    assert ctx.get_state("smooth_adjacency_builds") == 1 and ctx.get_state("smooth_normal_builds") == len(todo)


def _object_pixels(F, setup, which):
    ids = FR.primary(F, setup)["pr"]["id"]
    a, b = F.scene["objects"][which]
    return (ids >= a) & (ids < b), ids


@pytest.mark.gpu
def test_creases_stay_and_the_sphere_loses_its_facets(ugrt, SM, K, torch, capsys):
    """scenes.smooth() at 128 x 128, the plain frame.
    With smooth_cos = 2 every corner keeps its face's normal, and at 0.5 so do the welded box's: the bytes are within 1 of
    the plain frame's (the shading normal is NORMALIZE(e1 x e2), the primary pass' normalises the edges first, and the mix
    rounds).  Measured: smooth_cos = 2 changes 0.00 % of the 16 384 hit pixels, smooth_cos = 0.5 changes 0.00 % of the box's
    2 243 pixels.
    On the sphere's pixels off its silhouette (the pixel and its eight neighbours lie on the sphere), shadows=False so
    that no shadow edge crosses them, the mean absolute difference of horizontally neighbouring bytes across a change of
    triangle is 16.12 flat and 1.52 smooth (422 pairs)."""
    F = frames(K, "smooth")
    setup = F.setup
    ctx, r = make(F)
    img = {}
    for what, kw in (("flat", dict()), ("cos 2", dict(smooth=True, smooth_cos=2)), ("cos 0.5", dict(smooth=True)),
                     ("flat, no shadows", dict(shadows=False)), ("smooth, no shadows", dict(smooth=True, shadows=False))):
        r.display(setup, **kw)
        ctx.synchronize()
        img[what] = r.image.cpu().numpy().reshape(-1, 3).astype(np.int32)
    hit = FR.primary(F, setup)["pr"]["id"] >= 0
    diff = np.abs(img["cos 2"] - img["flat"]).max(1)
    box_px, ids = _object_pixels(F, setup, "box")
    box_diff = np.abs(img["cos 0.5"] - img["flat"]).max(1)[box_px]
    with capsys.disabled():
        print("\nsmooth_cos=2: %.2f %% of %d hit pixels differ; smooth_cos=0.5: %.2f %% of the box's %d pixels differ"
              % (100.0 * (diff[hit] > 0).mean(), int(hit.sum()), 100.0 * (box_diff > 0).mean(), int(box_px.sum())))
    assert diff.max() <= 1 and box_diff.max() <= 1 and int(box_px.sum()) > 100
    on, _ = _object_pixels(F, setup, "sphere")
    on2 = on.reshape(H, W)
    inner = on2.copy()
    inner[0, :] = inner[-1, :] = inner[:, 0] = inner[:, -1] = False
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner[1:-1, 1:-1] &= on2[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
    id2 = ids.reshape(H, W)
    pairs = inner[:, :-1] & inner[:, 1:] & (id2[:, :-1] != id2[:, 1:])
    assert int(pairs.sum()) > 200
    step = {}
    for what in ("flat, no shadows", "smooth, no shadows"):
        a = img[what].reshape(H, W, 3)
        step[what] = float(np.abs(a[:, :-1] - a[:, 1:])[pairs].mean())
    with capsys.disabled():
        print("sphere, %d pairs across a change of triangle: mean |step| %.2f flat, %.2f smooth"
              % (int(pairs.sum()), step["flat, no shadows"], step["smooth, no shadows"]))
    assert step["smooth, no shadows"] < step["flat, no shadows"]


@pytest.mark.gpu
def test_the_adjacency_and_the_corner_normals_are_kept_while_they_stand(ugrt, SM, K, torch):
    F = frames(K, "smooth")
    s, setup = F.scene, F.setup
    counts = lambda c: (c.get_state("smooth_adjacency_builds"), c.get_state("smooth_normal_builds"))

    def fresh_image(verts, **kw):
        c2 = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
        r2 = ugrt.Renderer(c2, verts, s["faces"], s["matidx"], s["mat_list"], s["reflect"], vertex_key=s["vertex_key"])
        r2.display(setup, smooth=True, **kw)
        c2.synchronize()
        return r2.image.cpu().numpy()

    ctx, r = make(F, ugrt.FLAG_STATIC_GEOMETRY)
    a, b = s["objects"]["sphere"]
    used = np.unique(np.asarray(s["faces"])[a:b])
    r.init_orig_list(int(used.max() - used.min() + 1), int(used.min()))
    first = fresh_image(s["verts"])
    for _ in range(8):
        r.display(setup, smooth=True)
        ctx.synchronize()
        np.testing.assert_array_equal(r.image.cpu().numpy(), first)
    assert counts(ctx) == (1, 1)
    r.display(setup, smooth=True, smooth_cos=0.25)  # another crease angle: the corner normals again
    r.display(setup, smooth=True, smooth_cos=0.25)
    ctx.synchronize()
    assert counts(ctx) == (1, 2)
    np.testing.assert_array_equal(r.image.cpu().numpy(), fresh_image(s["verts"], smooth_cos=0.25))
    r.display(setup, smooth=True)
    assert counts(ctx) == (1, 3)
    r.rotate_bunny(0.3)
    for _ in range(2):
        r.display(setup, smooth=True)
    ctx.synchronize()
    assert counts(ctx) == (1, 4)
    moved = r.d_verts.cpu().numpy()
    assert not np.array_equal(bits(moved), bits(_f32(s["verts"]).reshape(-1)))
    np.testing.assert_array_equal(r.image.cpu().numpy(), fresh_image(moved))
    assert not np.array_equal(r.image.cpu().numpy(), first)
    r.d_verts.copy_(ctx.upload(_f32(s["verts"]).reshape(-1)))
    r.geometry_changed()
    for _ in range(2):
        r.display(setup, smooth=True)
    ctx.synchronize()
    assert counts(ctx) == (2, 5)
    np.testing.assert_array_equal(r.image.cpu().numpy(), first)
    # without the flag the vertices may have moved behind the context's back: the corner normals every frame
    ctx, r = make(F)
    for _ in range(3):
        r.display(setup, smooth=True)
    ctx.synchronize()
    assert counts(ctx) == (1, 3)
    np.testing.assert_array_equal(r.image.cpu().numpy(), first)
    # smooth=False: nothing is built or allocated
    ctx, r = make(F, ugrt.FLAG_STATIC_GEOMETRY)
    for kw in (dict(), dict(ao=8, **{k: v for k, v in radii(F).items() if k == "ao_radius"})):
        r.display(setup, **kw)
    ctx.synchronize()
    assert counts(ctx) == (0, 0) and not hasattr(r, "snormal") and not hasattr(r, "_smooth")


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, SM, torch):
    verts, faces, _ = specials()
    faces = faces[:2]
    F, V = len(faces), len(verts)
    ctx = _small_context(ugrt)
    df, dv = ctx.upload(faces.reshape(-1)), ctx.upload(verts.reshape(-1))
    out = torch.full((9 * F,), 7.0, dtype=torch.float32, device=ctx.device)

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    # before any adjacency
    fails(ctx.smooth_corner_normals, (df, dv, F, 0.5, out), b"build the adjacency first")
    fails(ctx.smooth_get_adjacency, (), b"has not been built")
    fails(ctx.smooth_adjacency, (None, F, V), b"null d_facelist")
    fails(ctx.smooth_adjacency, (df, -1, V), b"negative")
    fails(ctx.smooth_adjacency, (df, F, -1), b"negative")
    fails(ctx.smooth_adjacency, (df, F, 0), b"no vertex")
    fails(ctx.smooth_corner_normals, (df, dv, F, 0.5, out), b"build the adjacency first")
    assert (ctx.get_state("smooth_adjacency_builds"), ctx.get_state("smooth_normal_builds")) == (0, 0)
    ctx.smooth_adjacency(df, F, V)
    fails(ctx.smooth_corner_normals, (df, dv, F, float("nan"), out), b"crease_cos")
    fails(ctx.smooth_corner_normals, (df, dv, F + 1, 0.5, out), b"the adjacency was built for")
    fails(ctx.smooth_corner_normals, (df, dv, -1, 0.5, out), b"negative")
    for h in (0, 1, 4):
        a = [df, dv, F, 0.5, out]
        a[h] = None
        fails(ctx.smooth_corner_normals, a, b"null")
    g = gbuffer()
    n = g["N"]
    d = [ctx.upload(g[k]) for k in ("t", "dirs", "ids", "cam", "verts", "faces", "cn", "normal_in")]
    nout = torch.full((3 * n,), 7.0, dtype=torch.float32, device=ctx.device)
    for h in range(9):
        a = d + [1, nout]
        a[h if h < 8 else 9] = None
        fails(ctx.smooth_normals, a, b"null")
    ctx.synchronize()
    assert (out == 7.0).all() and (nout == 7.0).all()  # nothing ran
    assert (ctx.get_state("smooth_adjacency_builds"), ctx.get_state("smooth_normal_builds")) == (1, 0)
    ctx.smooth_corner_normals(df, dv, F, 0.5, out)
    ctx.synchronize()
    assert_same(out.cpu().numpy(), SM.corner_normals(faces, verts, 0.5))
    # an empty face list is an adjacency too
    ctx.smooth_adjacency(None, 0, V)
    ctx.smooth_corner_normals(None, None, 0, 0.5, None)
    ctx.synchronize()
    corners, start = ctx.smooth_get_adjacency()
    assert corners.numel() == 0 and (start.cpu().numpy() == 0).all() and start.numel() == V + 1
    # the Python layer checks the host arrays at construction
    s = ugrt.scenes.smooth(scale=0.1)
    c2 = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD)
    for bad in (s["vertex_key"][:-1], s["vertex_key"].astype(np.float32), np.full(s["num_vertices"], s["num_vertices"], np.int32),
                np.full(s["num_vertices"], -1, np.int32)):
        with pytest.raises(ValueError):
            ugrt.Renderer(c2, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], vertex_key=bad)
