"""Fresnel glass: ugrt_fresnel_gather, ugrt_fresnel_shade and display(fresnel=...).

The checker is tests/fresnel_ref.c, a plain recursion over the section's rule with the same fixed leaf sum.  On the CPU it
is held against what exists: at scale 0 its image is the refract frame's (the chain's restatements) byte for byte and at
every scale its path 0 carries the chain's rays and hits.  The kernel is compared with it exactly: the words of d_acc and
the bytes of the image, a NaN matched by a NaN.

The synthetic tree: a glass slab of 12 triangles (transmit 0.8, reflect 0.1, ior 1.5) in front of a wall of two colours
with an opaque blocker before it, a mirror quad behind the eye, a degenerate triangle, 16 x 8 primary rays from a fan.
A ray reflected by the slab's front meets the mirror and comes back, a ray inside the slab meets its sides past the
critical angle: the trees are deep and of every shape.  `nested`: a second slab inside the first (ior 1.33).  The primary
hits come from the oracle's walk and the level-1 rays from tests/refract_ref.c; the edge cases overwrite single pixels'
primary hits, which the gather takes as given.

The bound of test_the_followed_weights_never_exceed_the_roots: a split forms wk = fl(w*k), fl(1 - F), fl(wk * fl(1 - F)) and
fl(wk * F): with u = 2^-24 the two children together weigh at most w*k*((1 - F)(1 + u)^2 + F(1 + u))(1 + u) <=
w*k*(1 + u)^3, a single child at most w*k*(1 + u).  With k <= 1 the leaves of a tree of depth D sum to at most
(1 + u)^(3 D) times the root's weight."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import frame_ref as FR
import test_frame_matrix as TFM
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
import test_refract as RFR
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
_p, _f32, _i32, bits = RD._p, RD._f32, RD._i32, RD.bits
_u32 = RFR._u32
CALLS = ("ugrt_fresnel_gather", "ugrt_fresnel_shade")
EPS = 1e-3
MAX_DEPTH = 6
U = 2.0 ** -24


class FresnelRef:
    def __init__(self, lib):
        self.lib = lib
        lib.fr_share.restype = C.c_int

    def share(self, c, ior, front, scale):
        """(split?, F, k2) of a glass hit."""
        F, k2 = C.c_float(0.0), C.c_float(0.0)
        two = self.lib.fr_share(C.c_float(c), C.c_float(ior), C.c_int(int(front)), C.c_float(scale), C.byref(F), C.byref(k2))
        return bool(two), np.float32(F.value), np.float32(k2.value)

    def split(self, w, k, F):
        w0, w1 = C.c_float(0.0), C.c_float(0.0)
        self.lib.fr_split(C.c_float(w), C.c_float(k), C.c_float(F), C.byref(w0), C.byref(w1))
        return np.float32(w0.value), np.float32(w1.value)

    def gather(self, ugrid, verts, faces, rays, active, normal, t, dirs, ids, cam_pos, mat_idx, mat_list, reflect, transmit, ior,
               depth, scale, min_weight, cc, light, shadow_light, eps, p0, n, N, fill=0.0, detail=False):
        """[4N] float32 sums; detail: also dict(nodes, share [N], rays [depth, 6N], active, t, id [depth, N]) of path 0."""
        acc = np.full(4 * N, fill, np.float32)
        mat_list, reflect = _f32(mat_list).reshape(-1), _f32(reflect)
        nodes = C.c_longlong(0)
        det = dict(share=np.zeros(N, np.float32), rays=np.zeros(depth * 6 * N, np.float32), active=np.zeros(depth * N, np.int32),
                   t=np.zeros(depth * N, np.float32), id=np.zeros(depth * N, np.int32))
        self.lib.fresnel_gather(_p(_f32(ugrid["ug"])), _p(_i32(ugrid["dims"])), _p(_u32(ugrid["vals"])), _p(_u32(ugrid["span"])),
                                _p(_u32(ugrid["offset"])), _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)),
                                _p(_f32(rays)), _p(_i32(active)), _p(_f32(normal)), _p(_f32(t)), _p(_f32(dirs)), _p(_i32(ids)),
                                _p(_f32(cam_pos)), _p(_i32(mat_idx)), _p(mat_list), _p(reflect), _p(_f32(transmit)), _p(_f32(ior)),
                                C.c_int(len(reflect)), C.c_int(depth), C.c_float(scale), C.c_float(min_weight), _p(_f32(cc)),
                                _p(_f32(light)), None if shadow_light is None else _p(_f32(shadow_light)), C.c_float(eps),
                                C.c_int(p0), C.c_int(n), C.c_longlong(N), _p(acc), C.byref(nodes), _p(det["share"]),
                                _p(det["rays"]), _p(det["active"]), _p(det["t"]), _p(det["id"]))
        if not detail:
            return acc
        det = {k: (v if k == "share" else v.reshape(depth, -1)) for k, v in det.items()}
        det["nodes"] = int(nodes.value)
        return acc, det

    def shade(self, cc, light, normal, t, dirs, ids, cam_pos, mat_idx, mat_list, acc, p0, n, N, fill=0):
        img, ids = np.full(3 * N, fill, np.uint8), _i32(ids).copy()
        mat_list = _f32(mat_list).reshape(-1)
        self.lib.fresnel_shade(_p(_f32(cc)), _p(_f32(light)), _p(img), _p(_f32(normal)), _p(_f32(t)), _p(_f32(dirs)), _p(ids),
                               _p(_f32(cam_pos)), _p(_i32(mat_idx)), _p(mat_list), C.c_int(len(mat_list) // 6), _p(_f32(acc)),
                               C.c_int(p0), C.c_int(n))
        return img, ids


@pytest.fixture(scope="session")
def FRS(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fresnel_ref") / "libfresnel_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "fresnel_ref.c"), "-lm"], check=True, capture_output=True)
    return FresnelRef(C.CDLL(out))


def same_words(got, want):
    """Float words equal bit for bit, a NaN matched by a NaN (sign and payload free)."""
    got, want = _f32(got).reshape(-1), _f32(want).reshape(-1)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def assert_words(got, want, what=""):
    got, want = _f32(got).reshape(-1), _f32(want).reshape(-1)
    bad = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), "%s: %d of %d words differ, first at %d: %r, not %r" % (
        what, int(bad.sum()), bad.size, int(np.flatnonzero(bad)[0]), got[bad][0], want[bad][0])


# --------------------------------------------------------------------------------------------------- the synthetic tree

SYN_W, SYN_H = 16, 8
SYN_N = SYN_W * SYN_H
SYN_DIMS = (8, 8, 8)
SYN_CAM = np.float32([0.3, 0.2, 5.0])
SYN_LIGHT = np.float32([1.0, 3.0, 6.0])          # ugrt_set_light_position's
SYN_SHADOW_LIGHT = np.float32([0.5, 0.5, 2.5])   # in front of the slab: the blocker shadows the wall, the slab does not
#              slab  wall l  wall r  mirror  inner slab
SYN_REFLECT = np.float32([0.1, 0.0, 0.0, 0.7, 0.0])
SYN_TRANSMIT = np.float32([0.8, 0.0, 0.0, 0.0, 0.9])
SYN_IOR = np.float32([1.5, 1.0, 1.0, 1.0, 1.33])


def _box(lo, hi):
    """The 8 corners and 12 triangles of a box, wound outwards."""
    lo, hi = np.float64(lo), np.float64(hi)
    v = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)])
    f = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2],
                  [1, 3, 7], [1, 7, 5]])
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * (v[f].mean(1) - (lo + hi) / 2)).sum(1) > 0).all()
    return v, f


def _quad(a, e1, e2):
    a, e1, e2 = np.float64(a), np.float64(e1), np.float64(e2)
    return np.array([a, a + e1, a + e1 + e2, a + e2]), np.array([[0, 1, 2], [0, 2, 3]])


_TREE = {}


def tree(O, RF, nested=False):
    """The synthetic tree's scene, primary hits and level-1 rays.  Computed once and shared: nobody writes to it."""
    if nested in _TREE:
        return _TREE[nested]
    parts = [(_box((-2, -1, 0), (2, 1, 1)), 0),
             (_quad((-6, -4, -3), (6, 0, 0), (0, 8, 0)), 1), (_quad((0, -4, -3), (6, 0, 0), (0, 8, 0)), 2),
             (_quad((-1, -0.5, -1.5), (1.5, 0, 0), (0, 1, 0)), 2),
             (_quad((-6, -4, 8), (0, 8, 0), (12, 0, 0)), 3),
             ((np.array([[3.0, 3.0, 3.0], [3.5, 3.5, 3.5], [4.0, 4.0, 4.0]]), np.array([[0, 1, 2]])), 0)]
    if nested:
        parts.append((_box((-1, -0.5, 0.25), (1, 0.5, 0.75)), 4))
    verts, faces, mat_idx, base = [], [], [], 0
    for (v, f), m in parts:
        verts.append(v)
        faces.append(f + base)
        mat_idx += [m] * len(f)
        base += len(v)
    verts, faces = np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32)
    mat_idx = np.int32(mat_idx)
    degenerate = 12 + 2 + 2 + 2 + 2
    assert mat_idx[degenerate] == 0 and len(faces) == (33 if nested else 21)
    grid = O.grid_uniform(faces, verts, verts.min(0), verts.max(0), SYN_DIMS)
    rng = np.random.RandomState(66)
    mat_list = rng.uniform(0.1, 0.9, (5, 6)).astype(np.float32)
    y, x = np.mgrid[0:SYN_H, 0:SYN_W]
    d = np.stack([(x - 7.5) / 7.5 * 0.6, (y - 3.5) / 3.5 * 0.3, -np.ones_like(x, float)], 2).reshape(-1, 3)
    dirs = (d / np.sqrt((d * d).sum(1))[:, None]).astype(np.float32).reshape(-1)
    eye = np.concatenate([np.tile(SYN_CAM, (SYN_N, 1)), dirs.reshape(-1, 3)], 1).astype(np.float32).reshape(-1)
    fv, ff = verts.reshape(-1), faces.reshape(-1)
    t, ids, _ = O.trace_dda(grid, fv, ff, eye, np.ones(SYN_N, np.int32), 0, SYN_N, SYN_N)
    tri = verts[faces[np.maximum(ids, 0)]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
    nrm = np.where((ids >= 0)[:, None], nrm / np.maximum(np.sqrt((nrm * nrm).sum(1)), 1e-30)[:, None], 0.0).astype(np.float32)
    cam = O.Cam(tuple(SYN_CAM), (0.3, 0.2, 0.0), (0, 1, 0), 1.0, 50.0)
    z = dict(verts=verts, faces=faces, mat_idx=mat_idx, mat_list=mat_list, grid=grid, dirs=dirs, t=_f32(t), ids=_i32(ids),
             normal=nrm.reshape(-1), cc=cam.cc.copy(), degenerate=degenerate, sums={}, RF=RF)
    z["rays"], z["active"] = level1(z, z["t"], z["dirs"], z["ids"])
    _TREE[nested] = z
    return z


def level1(z, t, dirs, ids, mat_idx=None, tables=None):
    reflect, transmit, ior = tables or (SYN_REFLECT, SYN_TRANSMIT, SYN_IOR)
    rays, active, _ = z["RF"].refract_rays(SYN_CAM, t, dirs, ids, z["mat_idx"] if mat_idx is None else mat_idx, reflect, transmit,
                                           ior, z["verts"], z["faces"], EPS, 0, SYN_N, SYN_N)
    return rays, active


def tree_sums(FRS, z, depth, scale, cut, shadow, active=None, p0=0, n=SYN_N, fill=0.0, detail=False, **over):
    """The checker on the tree; over: arrays in the place of the fixture's (rays, t, dirs, ids, normal, mat_idx, reflect,
    transmit, ior).  Plain calls are computed once per key and shared."""
    key = (depth, float(scale), float(cut), shadow, None if active is None else active.tobytes(), p0, n, fill)
    if not over and not detail and key in z["sums"]:
        return z["sums"][key]
    g = lambda name, default: over.get(name, default)
    out = FRS.gather(z["grid"], z["verts"], z["faces"], g("rays", z["rays"]), z["active"] if active is None else active,
                     g("normal", z["normal"]), g("t", z["t"]), g("dirs", z["dirs"]), g("ids", z["ids"]), SYN_CAM,
                     g("mat_idx", z["mat_idx"]), z["mat_list"], g("reflect", SYN_REFLECT), g("transmit", SYN_TRANSMIT),
                     g("ior", SYN_IOR), depth, scale, cut, z["cc"], SYN_LIGHT, SYN_SHADOW_LIGHT if shadow else None, EPS, p0, n,
                     SYN_N, fill, detail)
    if not over and not detail:
        z["sums"][key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    header = open(os.path.join(RD.ROOT, "include", "ugrt.h")).read()
    for name in CALLS:
        assert hasattr(lib, name) and name in ugrt.PROTOTYPES and "int %s(ugrt_ctx *ctx" % name in header
    assert len(ugrt.PROTOTYPES["ugrt_fresnel_gather"][1]) == 25 and len(ugrt.PROTOTYPES["ugrt_fresnel_shade"][1]) == 11
    for name in ("fresnel_gather", "shade_fresnel"):
        assert callable(getattr(ugrt.Context, name))
    assert "#define UGRT_MAX_FRESNEL_DEPTH 6" in header and ugrt.MAX_FRESNEL_DEPTH == 6
    assert lib.ugrt_version() == 105
    rmod = RLT._rmod(ugrt)
    assert callable(rmod.check_fresnel) and callable(rmod.fresnel_pass)
    import inspect

    for cls in (ugrt.Renderer, ugrt.BandedRenderer):
        names = list(inspect.signature(cls.display).parameters)
        assert names[-2:] == ["fresnel", "fresnel_cut"]
    sig = inspect.signature(ugrt.Renderer.display).parameters
    assert sig["fresnel"].default is False and sig["fresnel_cut"].default == 0.0


def test_the_schlick_share(FRS):
    """1 000 seeded (c, ior) pairs at scale 1, from the front: F lies in [r0, 1], falls as c grows (x = 1 - c falls), is r0
    exactly at c = 1 and 0 exactly for ior = 1, c = 1; a NaN or non-positive ior counts as 1; scale multiplies."""
    rng = np.random.RandomState(1)
    cs = rng.uniform(0, 1, 1000).astype(np.float32)
    iors = rng.uniform(1.0, 3.0, 1000).astype(np.float32)
    for c, ior in zip(cs, iors):
        two, F, k2 = FRS.share(c, ior, True, 1.0)
        q = (np.float32(1) - ior) / (np.float32(1) + ior)
        r0 = q * q
        assert two and k2 >= 0 and r0 <= F <= 1.0, (c, ior, F, r0)
        _, at_one, _ = FRS.share(1.0, ior, True, 1.0)
        assert bits(np.float32([at_one]))[0] == bits(np.float32([r0]))[0]
        _, half, _ = FRS.share(c, ior, True, 0.5)
        assert half == np.float32(0.5) * F
    for ior in (1.2, 1.5, 2.5):
        ladder = [FRS.share(c, ior, True, 1.0)[1] for c in np.linspace(1, 0, 201, dtype=np.float32)]
        assert (np.diff(np.float32(ladder)) >= 0).all() and ladder[0] < ladder[-1] == 1.0
    assert FRS.share(1.0, 1.0, True, 1.0)[1] == 0.0
    for odd in (float("nan"), 0.0, -2.0, -0.0):
        for c in (1.0, 0.5, 0.1):
            assert bits(np.float32([FRS.share(c, odd, True, 1.0)[1]]))[0] == bits(np.float32([FRS.share(c, 1.0, True, 1.0)[1]]))[0]
    # from inside: past the critical angle there is no split, and at it cs = sqrt(k2) = 0 gives F = scale
    assert FRS.share(0.5, 1.5, False, 1.0)[0] is False and FRS.share(0.9, 1.5, False, 1.0)[0] is True
    two, F, k2 = FRS.share(np.sqrt(np.float32(0.75)), 2.0, False, 0.25)
    assert two == (k2 >= 0) and (not two or abs(float(F) - 0.25) < 1e-3)


def test_the_followed_weights_never_exceed_the_roots(FRS):
    """Seeded trees of depth 1..6 with k in (0, 1] and F in [0, 1]: the leaves' weights, added in float64, stay below
    (1 + 2^-24)^(3 D) times the root's (the module's docstring derives the bound); a cut only takes weight away."""
    rng = np.random.RandomState(2)
    for depth in range(1, MAX_DEPTH + 1):
        for trial in range(200):
            cut = np.float32(rng.choice([0.0, 0.05]))
            single = rng.uniform() < 0.3

            def leaves(w, j):
                if j == depth:
                    return float(w)
                k = np.float32(rng.uniform(0.01, 1.0))
                if single and rng.uniform() < 0.5:
                    w0 = np.float32(w * k)
                    return leaves(w0, j + 1) if w0 > cut else 0.0
                F = np.float32(rng.choice([0.0, 1.0, rng.uniform()]))
                w0, w1 = FRS.split(w, k, F)
                return (leaves(w0, j + 1) if w0 > cut else 0.0) + (leaves(w1, j + 1) if w1 > cut else 0.0)

            total = leaves(np.float32(1.0), 0)
            assert total <= (1.0 + U) ** (3 * depth), (depth, trial, total)


def _fake(ugrt):
    r = TFM._fake(ugrt)
    r.__dict__.update(f_acc="facc")
    r._ensure_fresnel_buffers = lambda: None
    return r


GLASS3 = dict(reflect=True, refract=True, bounces=3)


def test_fresnel_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    chk = rmod.check_fresnel
    ok = dict(reflect=True, refract=True, bounces=3)
    assert chk(False) is None and chk(np.bool_(False), 0.0, **ok) is None
    assert chk(True, **ok) == (1.0, 0.0) and chk(np.bool_(True), **ok) == (1.0, 0.0)
    assert chk(0.5, 1 / 256, **ok) == (0.5, 1 / 256) and chk(1, 0, **ok) == (1.0, 0.0)
    assert chk(np.float32(0.25), np.float32(0.5), reflect=True, refract=True, bounces=6) == (0.25, 0.5)
    for bad in (0, 0.0, -0.5, 1.5, float("nan"), "1", None, (1,)):
        with pytest.raises(ValueError):
            chk(bad, **ok)
    for bad in (-1e-9, float("nan"), "0", None, True):
        with pytest.raises(ValueError):
            chk(True, bad, **ok)
    with pytest.raises(ValueError):
        chk(False, 0.1, **ok)  # the cut needs the effect
    for kw in (dict(), dict(reflect=True), dict(refract=True), dict(reflect=True, refract=True, bounces=7),
               dict(ok, lights=[("cam", "pos")]), dict(ok, reflect_lights=True), dict(ok, two_streams=True)):
        with pytest.raises(ValueError):
            chk(True, **kw)
        assert chk(False, **kw) is None
    s = RFR.scene(ugrt, "glass")
    setup = ugrt.FrameSetup.from_scene(s)
    lights = TL.setup_for(ugrt, s, TL.lights_for(s, 2))
    # the one-stream renderer: every illegal combination raises with nothing enqueued
    for st, kw in ((setup, dict(fresnel=True)), (setup, dict(fresnel=True, reflect=True)),
                   (setup, dict(GLASS3, fresnel=2.0)), (setup, dict(GLASS3, fresnel=0.0)), (setup, dict(GLASS3, fresnel_cut=0.1)),
                   (setup, dict(GLASS3, fresnel=True, fresnel_cut=-1.0)), (setup, dict(GLASS3, fresnel=True, bounces=7)),
                   (setup, dict(GLASS3, fresnel=True, bounces=8)), (lights, dict(GLASS3, fresnel=True)),
                   (lights, dict(GLASS3, fresnel=True, reflect_lights=True)), (setup, dict(GLASS3, fresnel=True, aa=4)),
                   (setup, dict(GLASS3, fresnel=True, glossy=4)), (setup, dict(GLASS3, fresnel=True, smooth=True))):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(st, **kw)
        assert r.ctx.calls == [], kw
    r = _fake(ugrt)
    r.aux = object()  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(setup, fresnel=True, **GLASS3)
    assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    for kw in (dict(fresnel=True), dict(fresnel=0.5, refract=True), dict(fresnel_cut=0.1)):
        with pytest.raises(ValueError):
            br.display(setup, **kw)
    # every legal one runs: with and without the shadow phase, every depth, the effects of the refract frame
    for kw in (dict(), dict(reflect_shadows=True), dict(bounces=1), dict(bounces=6), dict(shadows=False), dict(frame_cnt=2),
               dict(ao=4, ao_radius=1.0), dict(area=5, area_radius=0.5), dict(gi=4), dict(ao=4, ao_radius=1.0, temporal=4)):
        r = _fake(ugrt)
        r.display(setup, **dict(GLASS3, fresnel=True, **kw))
        assert [c[0] for c in r.ctx.calls].count("fresnel_gather") == 1, kw


def test_a_fresnel_frame_enqueues_its_calls_in_order_and_the_default_frame_none_of_them(ugrt):
    s = RFR.scene(ugrt, "glass")
    setup = ugrt.FrameSetup.from_scene(s)
    CAMERA_PASS, HARD = TFM.TA.CAMERA_PASS, TFM.TA.HARD
    names = lambda r: [c[0] for c in r.ctx.calls]
    new = {"fresnel_gather", "shade_fresnel"}
    # the defaults, written out or not: the frame as it was, on a renderer that has none of the new attributes
    for kw in (dict(), dict(GLASS3), dict(GLASS3, reflect_shadows=True), dict(reflect=True), dict(ao=4, ao_radius=1.0),
               dict(shade=False)):
        a, b = TFM._fake(ugrt), TFM._fake(ugrt)
        a.display(setup, **kw)
        b.display(setup, fresnel=False, fresnel_cut=0.0, **kw)
        plain = lambda r: [c[:1] + tuple(x for x in c[1:] if isinstance(x, (str, int, float))) for c in r.ctx.calls]
        assert plain(a) == plain(b) and not set(names(a)) & new
        assert not [k for k in vars(b) if "fresnel" in k or k == "f_acc"]
    head = CAMERA_PASS + HARD + ["refract_rays", "grid_build_uniform", "fresnel_gather"]
    for kw, want in ((dict(), head + ["shade_fresnel", "shade_add_shadows"]),
                     (dict(reflect_shadows=True), head + ["shade_fresnel", "shade_add_shadows"]),
                     (dict(shadows=False), CAMERA_PASS + head[len(CAMERA_PASS + HARD):] + ["shade_fresnel"]),
                     (dict(ao=4, ao_radius=1.0), head + ["ao_rays", "trace_dda_any_hemi", "shade_fresnel", "shade_add_shadows",
                                                         "shade_ao"]),
                     (dict(area=5, area_radius=0.5), CAMERA_PASS + head[len(CAMERA_PASS + HARD):]
                      + ["ao_rays", "trace_dda_any_area_thru", "shade_fresnel", "shade_area"]),
                     (dict(gi=8), head + ["ao_rays", "gi_gather", "shade_fresnel", "shade_add_shadows", "gi_apply"]),
                     (dict(shade=False), CAMERA_PASS + HARD)):
        r = _fake(ugrt)
        r.display(setup, fresnel=0.5, fresnel_cut=1 / 256, **dict(GLASS3, **kw))
        assert names(r) == want, (kw, names(r))
        if not kw.get("shade", True):
            continue
        g = [c for c in r.ctx.calls if c[0] == "fresnel_gather"][0]
        assert g[1:18] == ("value", "span", "offset", "v", "f", "rays1", "active1", "n", "t", "d", "ids", "cam", "mi", "ml", "refl",
                           "tr", "ior")
        assert g[18:22] == (3, 3, 0.5, 1 / 256) and g[23:] == (1e-3, "facc")
        if kw.get("reflect_shadows"):
            lcam = RLT._rmod(ugrt).make_camera(setup.light_camera, setup.fovy, 1.0)
            np.testing.assert_array_equal(np.float32(g[22]), np.float32(lcam.worldori[:3]))
        else:
            assert g[22] is None
        sh = [c for c in r.ctx.calls if c[0] == "shade_fresnel"][0]
        assert sh[1:] == ("img", "n", "t", "d", "ids", "cam", "mi", "ml", 3, "facc")
        assert not set(names(r)) & {"trace_dda", "refract_rays_next", "occlusion_rays", "trace_dda_any_thru",
                                    "shade_reflect_depth", "shade_reflect_depth_occluded", "shade_reflect"}
    r = _fake(ugrt)
    r.display(setup, fresnel=True, bounces=6, reflect=True, refract=True)
    g = [c for c in r.ctx.calls if c[0] == "fresnel_gather"][0]
    assert g[19:22] == (6, 1.0, 0.0)


def test_the_synthetic_tree_is_feasible(O, RF, FRS):
    """On the checker alone: the fixture has pixels without a tree, single children past the critical angle, both children
    followed, dropped children under a cut, hits of the mirror, misses and shadowed hits; min_weight = 1 follows nothing."""
    z = tree(O, RF)
    act = z["active"] != 0
    figures = dict(active=int(act.sum()), misses=int((z["ids"] < 0).sum()))
    assert 65 <= figures["active"] < SYN_N and (z["mat_idx"][z["ids"][act]] == 0).all()
    nodes = {}
    for depth in (1, 3, 6):
        for scale in (0.0, 0.5, 1.0):
            acc, det = tree_sums(FRS, z, depth, scale, 0.0, True, detail=True)
            nodes[(depth, scale)] = det["nodes"]
            acc = acc.reshape(-1, 4)
            assert not acc[~act].any() and (acc[act, 3] == 1).all() and np.isfinite(acc).all()
    figures["nodes"] = nodes
    # (a primary hit on the slab's rim can take a side face from behind: past the critical angle, one child)
    assert nodes[(1, 0.0)] == figures["active"] and 2 * figures["active"] - 4 <= nodes[(1, 1.0)] <= 2 * figures["active"]
    assert nodes[(6, 1.0)] > 2 * nodes[(6, 0.0)] and nodes[(3, 0.5)] > nodes[(3, 0.0)]
    cutn = tree_sums(FRS, z, 6, 1.0, 0.05, True, detail=True)[1]["nodes"]
    assert 0 < cutn < nodes[(6, 1.0)]
    figures["nodes_cut"] = cutn
    acc1, det1 = tree_sums(FRS, z, 6, 1.0, 1.0, True, detail=True)
    assert det1["nodes"] == 0
    prim = tree_sums(FRS, z, 1, 0.0, 1.0, False).reshape(-1, 4)
    np.testing.assert_array_equal(bits(acc1), bits(prim.reshape(-1)))  # every active pixel is its primary colour
    lit, shadowed = tree_sums(FRS, z, 4, 0.5, 0.0, False), tree_sums(FRS, z, 4, 0.5, 0.0, True)
    assert (lit >= shadowed).all() and int((lit != shadowed).sum()) >= 20
    figures["shadow_changes"] = int((lit != shadowed).sum())
    # path 0 past the critical angle: a ray inside the slab that meets a side
    _, det = tree_sums(FRS, z, 3, 1.0, 0.0, False, detail=True)
    inside = det["active"][0] != 0
    side = inside & np.isin(det["id"][0], np.arange(4, 12))
    figures["side_hits"] = int(side.sum())
    assert figures["side_hits"] >= 1
    print(figures)


_GLASS = {}


def glass(K):
    """frame_ref's Frames of scenes.glass() at 128 x 128 with the oracle's primary pass.  Made once and shared."""
    if not _GLASS:
        F = FR.Frames(K, K.ugrt.scenes.glass(), 128, 128)
        _GLASS.update(F=F, P=FR.primary(F, F.setup), sums={})
    return _GLASS


def glass_sums(K, FRS, depth, scale, cut, shadow, detail=False):
    G = glass(K)
    key = (depth, scale, cut, shadow)
    if key not in G["sums"]:
        F, P = G["F"], G["P"]
        s, pr = F.scene, P["pr"]
        lv1 = FR.levels(F, F.setup, True, 1, False)[0]
        G["sums"][key] = FRS.gather(F.ugrid, F.verts, F.faces, lv1["rays"], lv1["active"], pr["normal"], pr["t"], pr["dir"], pr["id"],
                                    P["cam_pos"], s["matidx"], s["mat_list"], s["reflect"], s["transmit"], s["ior"], depth, scale,
                                    cut, P["lcam"].cc, F.setup.shading_light, P["light"] if shadow else None, EPS, 0, F.N, F.N,
                                    detail=True)
    return G["sums"][key] if detail else G["sums"][key][0]


def glass_image(K, FRS, acc):
    G = glass(K)
    F, P = G["F"], G["P"]
    pr = P["pr"]
    return FRS.shade(P["lcam"].cc, F.setup.shading_light, pr["normal"], pr["t"], pr["dir"], pr["id"], P["cam_pos"],
                     F.scene["matidx"], F.scene["mat_list"], acc, 0, F.N, F.N)


@pytest.mark.parametrize("depth", [1, 3, 6])
def test_at_scale_0_the_checker_is_the_refract_frame_and_path_0_is_the_chain(K, FRS, depth):
    """scenes.glass() at 128 x 128 on the CPU: the checker's image at scale 0 is the image of the chain's restatements
    (shade_reflect_depth / _occluded over rf_refract_rays + orc_trace_dda) byte for byte, and at scale 0.5 the level rays
    and hits of its path 0 are the chain's."""
    G = glass(K)
    F = G["F"]
    for shadow in (False, True):
        k = dict(FR.DEFAULTS, **FR.MORE)
        k.update(reflect=True, refract=True, bounces=depth, reflect_shadows=shadow)
        if depth == 1 and not shadow:
            k["bounces"] = 1  # (shade_reflect: the same bytes, as tests/test_reflect_depth.py pins)
        want, want_ids = FR.shading_call(F, F.setup, k)
        got, got_ids = glass_image(K, FRS, glass_sums(K, FRS, depth, 0.0, 0.0, shadow))
        np.testing.assert_array_equal(got, want, err_msg="depth %d shadow %s" % (depth, shadow))
        np.testing.assert_array_equal(got_ids, want_ids)
    chain = FR.levels(F, F.setup, True, depth, False)
    _, det = glass_sums(K, FRS, depth, 0.5, 0.0, False, detail=True)
    for j, lv in enumerate(chain):
        np.testing.assert_array_equal(det["active"][j], lv["active"], err_msg="level %d" % (j + 1))
        assert_words(det["rays"][j], lv["rays"], "level %d rays" % (j + 1))
        on = lv["active"] != 0
        np.testing.assert_array_equal(det["id"][j][on], lv["hit_id"][on])
        assert_words(det["t"][j][on], lv["hit_t"][on], "level %d t" % (j + 1))


def test_what_it_looks_like(K, FRS):
    """Reports only: the fresnel frame differs from the refract frame, and the reflected share k*F over the ball's pixels
    within 2 pixels of its silhouette against those within 2 pixels of its centre."""
    G = glass(K)
    F, P = G["F"], G["P"]
    plain, _ = glass_image(K, FRS, glass_sums(K, FRS, 3, 0.0, 0.0, True))
    acc, det = glass_sums(K, FRS, 3, 1.0, 0.0, True, detail=True)
    full, _ = glass_image(K, FRS, acc)
    assert (plain != full).any()
    ids = P["pr"]["id"]
    ball = (np.where(ids >= 0, np.asarray(F.scene["matidx"])[np.maximum(ids, 0)], -1) == 4).reshape(F.H, F.W)
    near = np.zeros_like(ball)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            near |= ~np.roll(np.roll(ball, dy, 0), dx, 1)
    rim = ball & near
    yy, xx = np.nonzero(ball)
    cy, cx = yy.mean(), xx.mean()
    y, x = np.mgrid[0:F.H, 0:F.W]
    centre = ball & (np.maximum(abs(y - cy), abs(x - cx)) <= 2)
    share = det["share"].reshape(F.H, F.W)
    print(dict(ball=int(ball.sum()), rim=int(rim.sum()), centre=int(centre.sum()), share_rim=float(share[rim].mean()),
               share_centre=float(share[centre].mean()), changed=int((plain != full).reshape(-1, 3).any(1).sum())))


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _tree_context(ugrt, z, rows=None, height=SYN_H):
    ctx = ugrt.Context(SYN_W, height, light_grid=(16, 16), uniform_dims=SYN_DIMS, rows=rows)
    dv, df = ctx.upload(z["verts"].reshape(-1)), ctx.upload(z["faces"].reshape(-1))
    ctx.grid_build_uniform(df, dv, len(z["faces"]), z["verts"].min(0), z["verts"].max(0))
    ctx.upload_camera(z["cc"])
    ctx.set_light_position(SYN_LIGHT)
    up = lambda a: ctx.upload(np.ascontiguousarray(a))
    return types.SimpleNamespace(ctx=ctx, dv=dv, df=df, grid=ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3], cam=up(SYN_CAM),
                                 mat_list=up(z["mat_list"].reshape(-1)), up=up,
                                 base={k: up(z[k]) for k in ("rays", "active", "normal", "t", "dirs", "ids", "mat_idx")},
                                 tables=dict(reflect=up(SYN_REFLECT), transmit=up(SYN_TRANSMIT), ior=up(SYN_IOR)))


def _gather(torch, d, depth, scale, cut, shadow, n_words=4 * SYN_N, sentinel=-7.0, dv=None, df=None, **over):
    acc = torch.full((n_words,), sentinel, dtype=torch.float32, device=d.ctx.device)
    g = lambda name: d.up(over[name]) if name in over else (d.base.get(name) if name in d.base else d.tables[name])
    d.ctx.fresnel_gather(d.grid[0], d.grid[1], d.grid[2], d.dv if dv is None else dv, d.df if df is None else df, g("rays"),
                         g("active"), g("normal"), g("t"), g("dirs"), g("ids"), d.cam, g("mat_idx"), d.mat_list, g("reflect"),
                         g("transmit"), g("ior"), 5, depth, scale, cut, SYN_SHADOW_LIGHT if shadow else None, EPS, acc)
    d.ctx.synchronize()
    return acc.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
def test_synthetic_tree(ugrt, O, RF, FRS, torch, depth):
    """scale {0, 0.5, 1} x min_weight {0, 0.05, 1} x the shadow phase, through the triangle records and through the gather
    of vertices, and the nested slab: the words of the checker, exactly, and the nodes it walked."""
    z = tree(O, RF)
    d = _tree_context(ugrt, z)
    dv2, df2 = d.dv.clone(), d.df.clone()  # not the arrays the grid was built from: no triangle records
    gathers = d.ctx.get_state("fresnel_gathers")
    for scale in (0.0, 0.5, 1.0):
        for cut in (0.0, 0.05, 1.0):
            for shadow in (False, True):
                what = "depth %d scale %g cut %g shadow %s" % (depth, scale, cut, shadow)
                want = tree_sums(FRS, z, depth, scale, cut, shadow)
                assert_words(_gather(torch, d, depth, scale, cut, shadow), want, what)
                nodes = d.ctx.get_state("fresnel_nodes")
                assert_words(_gather(torch, d, depth, scale, cut, shadow, dv=dv2, df=df2), want, what + ", no records")
        _, det = tree_sums(FRS, z, depth, scale, 1.0, True, detail=True)
        assert nodes == det["nodes"] == 0
    _, det = tree_sums(FRS, z, depth, 0.5, 0.0, False, detail=True)
    _gather(torch, d, depth, 0.5, 0.0, False)
    assert d.ctx.get_state("fresnel_nodes") == det["nodes"] > 0
    assert d.ctx.get_state("fresnel_gathers") == gathers + 37
    zn = tree(O, RF, nested=True)
    dn = _tree_context(ugrt, zn)
    for scale, cut, shadow in ((1.0, 0.0, True), (0.5, 0.05, False)):
        assert_words(_gather(torch, dn, depth, scale, cut, shadow), tree_sums(FRS, zn, depth, scale, cut, shadow),
                     "nested, depth %d scale %g" % (depth, scale))
    assert int((tree_sums(FRS, zn, depth, 1.0, 0.0, True) != tree_sums(FRS, z, depth, 1.0, 0.0, True)).sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
def test_active_counts_launch_shapes_and_a_band_change_no_other_word(ugrt, O, RF, FRS, torch, depth):
    """1, 63, 64 and 65 active pixels (65 and 63 fill no last wave at any depth); any_rays_per_wave x any_coop and
    dda_blocks = 1 (every later group comes from the ticket); a band of rows of a taller frame: inactive pixels of the band
    get four zeros, pixels outside it keep their words."""
    z = tree(O, RF)
    d = _tree_context(ugrt, z)
    on = np.flatnonzero(z["active"])
    for count in (1, 63, 64, 65):
        act = np.zeros(SYN_N, np.int32)
        act[on[:count]] = 1
        want = tree_sums(FRS, z, depth, 1.0, 0.0, True, active=act)
        assert int((want.reshape(-1, 4)[:, 3] == 1).sum()) == count
        assert_words(_gather(torch, d, depth, 1.0, 0.0, True, active=act), want, "depth %d, %d active" % (depth, count))
    want = tree_sums(FRS, z, depth, 1.0, 0.0, True)
    for rpw in (7, 64):
        for coop in (1, 1000):
            d.ctx.set_option("any_rays_per_wave", rpw)
            d.ctx.set_option("any_coop", coop)
            assert_words(_gather(torch, d, depth, 1.0, 0.0, True), want, "rays per wave %d, coop %d" % (rpw, coop))
    d.ctx.set_option("any_rays_per_wave", -1)
    d.ctx.set_option("any_coop", -1)
    d.ctx.set_option("dda_blocks", 1)
    assert_words(_gather(torch, d, depth, 1.0, 0.0, True), want, "one workgroup")
    d.ctx.set_option("dda_blocks", -1)
    # the band: tile row 1 of 3, the frame's arrays three times over
    b = _tree_context(ugrt, z, rows=(1, 2), height=3 * SYN_H)
    assert (b.ctx.p0, b.ctx.npix) == (SYN_N, SYN_N)
    over = {k: np.tile(z[k], 3) for k in ("rays", "active", "normal", "t", "dirs", "ids")}
    got = _gather(torch, b, depth, 1.0, 0.0, True, n_words=12 * SYN_N, **over)
    assert (got[:4 * SYN_N] == -7.0).all() and (got[8 * SYN_N:] == -7.0).all()
    assert_words(got[4 * SYN_N:8 * SYN_N], want, "the band")


def _critical_scan():
    """Directions (dx, 0, dz) of squared length exactly 1 in float arithmetic whose dz run through consecutive floats around
    sqrt(1 - 1/2.25), the critical cosine of ior 1.5: c = dz exactly for a hit on a triangle whose normal is (0, 0, 1)."""
    crit = np.float32(np.sqrt(1.0 - 1.0 / 2.25))
    dz = crit
    for _ in range(8):
        dz = np.nextafter(dz, np.float32(0))
    out = []
    for _ in range(17):
        guess = np.float32(np.sqrt(1.0 - float(dz) ** 2))
        for step in range(-8, 9):
            dx = guess
            for _ in range(abs(step)):
                dx = np.nextafter(dx, np.float32(2 if step > 0 else 0))
            if np.float32(np.float32(dx * dx) + np.float32(dz * dz)) == np.float32(1.0):
                out.append((dx, dz))
                break
        dz = np.nextafter(dz, np.float32(1))
    return out


def edge_pixels(z, FRS):
    """The tree's arrays with single pixels' primary hits overwritten (the gather takes them as given), and what each is
    for.  Pixel p of the first rows: the critical scan (a hit of the slab's front face from inside, triangle 2: normal
    (0, 0, 1)), then edge-on hits with d.n = +0 and -0, then the degenerate triangle."""
    t, dirs, ids, normal = z["t"].copy(), z["dirs"].copy().reshape(-1, 3), z["ids"].copy(), z["normal"].copy().reshape(-1, 3)
    tri = z["verts"][z["faces"][2]]
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    assert tuple(n / np.abs(n).max()) == (0.0, 0.0, 1.0) and z["mat_idx"][2] == 0
    scan = _critical_scan()
    k2 = []
    for p, (dx, dz) in enumerate(scan):
        dirs[p], t[p], ids[p], normal[p] = (dx, 0.0, dz), 1.0, 2, (0, 0, 1)
        k2.append(FRS.share(dz, 1.5, False, 1.0)[2])
    p = len(scan)
    for d in ((1.0, 1.0, 0.0), (-1.0, -1.0, -0.0)):
        dirs[p], t[p], ids[p], normal[p] = d, 2.0, 2, (0, 0, 1)
        p += 1
    dirs[p], t[p], ids[p], normal[p] = (0.0, 0.6, -0.8), 3.0, z["degenerate"], (0, 0, 1)
    roles = dict(scan=(0, len(scan)), k2=np.float32(k2), edge_on=(len(scan), len(scan) + 2), degenerate=p)
    dirs, normal = np.ascontiguousarray(dirs.reshape(-1)), np.ascontiguousarray(normal.reshape(-1))
    rays, active = level1(z, t, dirs, ids)
    return dict(t=t, dirs=dirs, ids=ids, normal=normal, rays=rays, active=active), roles


@pytest.mark.gpu
def test_the_edges_of_the_rule(ugrt, O, RF, FRS, torch):
    """Incidence at the critical angle and its float neighbours (k2 changes sign between two consecutive cosines), edge-on
    hits (d.n of +0 and -0: front, the normal not turned), the degenerate triangle (NaN rays stay active, NaN words match
    NaN words), a denormal, an infinite, a NaN and a negative ior, a material with both transmit and reflect (the slab's
    own), materials out of range at level 2 (half of the wall), a child of weight exactly min_weight (not followed) and
    the next float above it (followed): the checker's words, exactly, at depths 1, 3 and 6."""
    z = tree(O, RF)
    d = _tree_context(ugrt, z)
    over, roles = edge_pixels(z, FRS)
    k2 = roles["k2"]
    assert len(k2) >= 12 and (k2 < 0).any() and (k2 >= 0).any()
    flip = int(np.flatnonzero(k2 >= 0)[0])
    assert flip > 0 and (k2[:flip] < 0).all() and (k2[flip:] >= 0).all()  # one sign change, between float neighbours
    lo, hi = over["dirs"].reshape(-1, 3)[flip - 1, 2], over["dirs"].reshape(-1, 3)[flip, 2]
    assert np.nextafter(lo, np.float32(1)) == hi
    for p in range(*roles["scan"]):
        assert over["active"][p] == 1
    for p in range(*roles["edge_on"]):
        assert over["active"][p] == 1 and np.isfinite(over["rays"][6 * p:6 * p + 6]).all()
    assert over["active"][roles["degenerate"]] == 1 and np.isnan(over["rays"][6 * roles["degenerate"] + 3])
    for depth in (1, 3, 6):
        for scale in (0.5, 1.0):
            want, det = tree_sums(FRS, z, depth, scale, 0.0, True, detail=True, **over)
            assert_words(_gather(torch, d, depth, scale, 0.0, True, **over), want, "edge pixels, depth %d" % depth)
            if depth == 1:  # past the critical angle one child, at and below it two
                for p in range(*roles["scan"]):
                    assert (det["share"][p] > 0) == (k2[p] >= 0)
    # the indices of refraction: denormal and infinite are themselves, NaN and negative count as 1
    tables = {}
    for name, ior0 in (("denormal", 1e-42), ("inf", float("inf")), ("nan", float("nan")), ("negative", -1.5), ("one", 1.0)):
        ior = SYN_IOR.copy()
        ior[0] = ior0
        rays, active = level1(z, z["t"], z["dirs"], z["ids"], tables=(SYN_REFLECT, SYN_TRANSMIT, ior))
        want = tree_sums(FRS, z, 3, 1.0, 0.0, True, ior=ior, rays=rays, active=active)
        assert_words(_gather(torch, d, 3, 1.0, 0.0, True, ior=ior, rays=rays, active=active), want, "ior " + name)
        tables[name] = want
    assert same_words(tables["nan"], tables["one"]) and same_words(tables["negative"], tables["one"])
    assert not same_words(tables["denormal"], tables["one"]) and not same_words(tables["inf"], tables["one"])
    # materials out of range at level 2: the right half of the wall and the blocker
    mat_idx = z["mat_idx"].copy()
    mat_idx[z["mat_idx"] == 2] = 9
    mat_idx[14] = -1
    want = tree_sums(FRS, z, 3, 1.0, 0.0, True, mat_idx=mat_idx)
    assert_words(_gather(torch, d, 3, 1.0, 0.0, True, mat_idx=mat_idx), want, "materials out of range")
    assert not same_words(want, tree_sums(FRS, z, 3, 1.0, 0.0, True))
    # a cut exactly at a child's weight: the root's child 1 of the first active pixel weighs k*F
    _, det = tree_sums(FRS, z, 2, 1.0, 0.0, False, detail=True)
    p = int(np.flatnonzero(det["share"] > 0)[0])
    w1 = np.float32(det["share"][p])
    below = np.nextafter(w1, np.float32(0))
    one = np.zeros(SYN_N, np.int32)
    one[p] = 1
    nodes = {}
    for name, cut in (("at", w1), ("below", below)):
        want, dd = tree_sums(FRS, z, 2, 1.0, float(cut), False, active=one, detail=True)
        assert_words(_gather(torch, d, 2, 1.0, float(cut), False, active=one), want, "cut %s the weight" % name)
        nodes[name] = dd["nodes"]
        assert d.ctx.get_state("fresnel_nodes") == dd["nodes"]
    assert nodes["below"] > nodes["at"]


def _device_fresnel(ugrt, torch, G, r, ctx, depth, scale, cut, shadow):
    """refract_rays, fresnel_gather and shade_fresnel on a renderer's primary hits (display(shade=False) left them)."""
    F, P = G["F"], G["P"]
    N = F.N
    rays = torch.empty(6 * N, dtype=torch.float32, device=ctx.device)
    active = torch.empty(N, dtype=torch.int32, device=ctx.device)
    acc = torch.full((4 * N,), -7.0, dtype=torch.float32, device=ctx.device)
    img = torch.full((3 * N,), 9, dtype=torch.uint8, device=ctx.device)
    ids = r.intersect_id.clone()
    ctx.refract_rays(r.cam_pos, r.t, r.dir, ids, r.d_matidx, r.d_reflect, r.d_transmit, r.d_ior, r.num_materials, r.d_verts,
                     r.d_faces, EPS, rays, active)
    u = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    ctx.fresnel_gather(u[0], u[1], u[2], r.d_verts, r.d_faces, rays, active, r.normal, r.t, r.dir, ids, r.cam_pos, r.d_matidx,
                       r.d_matlist, r.d_reflect, r.d_transmit, r.d_ior, r.num_materials, depth, scale, cut,
                       P["light"] if shadow else None, EPS, acc)
    ctx.shade_fresnel(img, r.normal, r.t, r.dir, ids, r.cam_pos, r.d_matidx, r.d_matlist, r.num_materials, acc)
    ctx.synchronize()
    return acc.cpu().numpy(), img.cpu().numpy(), ids.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3, 6])
def test_the_seam_to_the_refract_frame(ugrt, K, FRS, torch, depth):
    """scenes.glass() at 128 x 128, reflect_shadows on and off: fresnel_gather(scale = 0) + shade_fresnel give the image of
    display(reflect=True, refract=True, bounces=depth, reflect_shadows=...) byte for byte; the levels that display traced
    are the checker's path 0 at scale 0.5; and at scale 0.5 the words and bytes are the checker's."""
    G = glass(K)
    F = G["F"]
    ctx, r = F.make()
    for shadow in (False, True):
        r.display(F.setup, shadows=False, reflect=True, refract=True, bounces=depth, reflect_shadows=shadow)
        ctx.synchronize()
        frame = r.image.cpu().numpy().copy()
        frame_ids = r.intersect_id.cpu().numpy().copy()
        chain = [dict(rays=r.rays_levels[j].cpu().numpy(), active=r.active_levels[j].cpu().numpy(),
                      hit_t=r.hit_t_levels[j].cpu().numpy(), hit_id=r.hit_id_levels[j].cpu().numpy()) for j in range(depth)]
        r.display(F.setup, shadows=False, shade=False)
        acc, img, ids = _device_fresnel(ugrt, torch, G, r, ctx, depth, 0.0, 0.0, shadow)
        np.testing.assert_array_equal(img, frame, err_msg="depth %d shadow %s" % (depth, shadow))
        np.testing.assert_array_equal(ids, frame_ids)
        assert_words(acc, glass_sums(K, FRS, depth, 0.0, 0.0, shadow), "scale 0")
        want, det = glass_sums(K, FRS, depth, 0.5, 0.0, shadow, detail=True)
        for j, lv in enumerate(chain):
            np.testing.assert_array_equal(det["active"][j], lv["active"], err_msg="level %d" % (j + 1))
            assert_words(det["rays"][j], lv["rays"], "level %d rays" % (j + 1))
            on = lv["active"] != 0
            np.testing.assert_array_equal(det["id"][j][on], lv["hit_id"][on])
            assert_words(det["t"][j][on], lv["hit_t"][on], "level %d t" % (j + 1))
        acc, img, ids = _device_fresnel(ugrt, torch, G, r, ctx, depth, 0.5, 0.0, shadow)
        assert_words(acc, want, "scale 0.5")
        assert ctx.get_state("fresnel_nodes") == det["nodes"]
        want_img, want_ids = glass_image(K, FRS, want)
        np.testing.assert_array_equal(img, want_img)
        np.testing.assert_array_equal(ids, want_ids)


FRAME = dict(reflect=True, refract=True, bounces=3, reflect_shadows=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fresnel", [0.5, 1.0])
def test_fresnel_frames_equal_the_cpu_frames(ugrt, K, FRS, torch, fresnel):
    """display(fresnel=...) on scenes.glass() at 128 x 128, alone, with ao, with area, and with a cut: the CPU frame is
    frame_ref's composer with the checker's image in the place of its shading call's."""
    G = glass(K)
    F, P = G["F"], G["P"]
    radii = dict(ao_radius=float(np.float32(0.10 * F.extent)), area_radius=float(np.float32(0.25 * F.extent)))
    ctx, r = F.make()
    for extra, cut in ((dict(), 0.0), (dict(ao=8, ao_radius=radii["ao_radius"]), 0.0),
                       (dict(area=5, area_radius=radii["area_radius"]), 0.0), (dict(shadows=False), 1 / 256)):
        kw = dict(FRAME, **extra)
        acc = glass_sums(K, FRS, 3, fresnel, cut, True)
        F2 = FR.Frames(K, F.scene, F.W, F.H)
        # (the oracle's primary pass and the effects' words are shared, nobody writes to them; the shading call's entry is
        # the checker's image here and the refract frame's in F)
        key = ("shaded", FR._setup_key(F.setup), False, False, True, True, 3, True, False)
        F2.cache = {n: v for n, v in F.cache.items() if n != key}
        F2.cache[key] = glass_image(K, FRS, acc)
        want = FR.cpu_display(F2, **kw)
        F.cache.update({n: v for n, v in F2.cache.items() if n != key})
        r.display(F.setup, fresnel=fresnel, fresnel_cut=cut, **kw)
        ctx.synchronize()
        got = dict(image=r.image.cpu().numpy(), intersect_id=r.intersect_id.cpu().numpy(), is_shadowed=r.is_shadowed.cpu().numpy())
        for name in ("ao_mask", "area_mask"):
            if name in want:
                got[name] = getattr(r, name).cpu().numpy().view(np.uint32)
        bad = FR.differences(want, got, only=("image", "intersect_id", "is_shadowed", "ao_mask", "area_mask"))
        assert not bad, (extra, bad)
        assert_words(r.f_acc.cpu().numpy(), acc, "f_acc")
        plain = FR.cpu_display(F, **kw)["image"]
        assert key in F.cache and F.cache[key][0] is not F2.cache[key][0] and (plain != want["image"]).any()
    assert r.rays_levels.shape[0] == 1  # one level's rays: the tree's levels live in registers


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, RF, FRS, torch):
    z = tree(O, RF)
    fresh = ugrt.Context(SYN_W, SYN_H, light_grid=(16, 16), uniform_dims=SYN_DIMS)
    q = torch.zeros(6 * SYN_N, dtype=torch.float32, device=fresh.device)
    with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
        fresh.fresnel_gather(*[q] * 17, 5, 3, 1.0, 0.0, None, EPS, q)
    assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    d = _tree_context(ugrt, z)
    ctx = d.ctx
    acc = torch.full((4 * SYN_N + 4,), -7.0, dtype=torch.float32, device=ctx.device)
    img = torch.full((3 * SYN_N,), 200, dtype=torch.uint8, device=ctx.device)
    ids = d.base["ids"].clone()
    b, tb = d.base, d.tables
    args = [d.grid[0], d.grid[1], d.grid[2], d.dv, d.df, b["rays"], b["active"], b["normal"], b["t"], b["dirs"], ids, d.cam,
            b["mat_idx"], d.mat_list, tb["reflect"], tb["transmit"], tb["ior"], 5, 3, 1.0, 0.0, SYN_SHADOW_LIGHT, EPS, acc]
    gathers = ctx.get_state("fresnel_gathers")

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    def swap(a, h, v):
        return a[:h] + [v] + a[h + 1:]

    for bad in (0, 7, -1):
        fails(ctx.fresnel_gather, swap(args, 18, bad), b"depth")
    for bad in (-0.1, 1.5, float("nan")):
        fails(ctx.fresnel_gather, swap(args, 19, bad), b"scale")
    for bad in (-1e-9, float("nan")):
        fails(ctx.fresnel_gather, swap(args, 20, bad), b"min_weight")
    fails(ctx.fresnel_gather, swap(args, 22, float("nan")), b"eps")
    for bad in (0, -3):
        fails(ctx.fresnel_gather, swap(args, 17, bad), b"num_materials")
    fails(ctx.fresnel_gather, swap(args, 23, acc[1:]), b"aligned")
    for h in list(range(17)) + [23]:
        fails(ctx.fresnel_gather, swap(args, h, None), b"null")
    s_args = [img, b["normal"], b["t"], b["dirs"], ids, d.cam, b["mat_idx"], d.mat_list, 5, acc]
    for h in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        fails(ctx.shade_fresnel, swap(s_args, h, None), b"null")
    fails(ctx.shade_fresnel, swap(s_args, 9, acc[1:]), b"aligned")
    ctx.synchronize()
    assert (acc == -7.0).all() and (img == 200).all() and torch.equal(ids, d.base["ids"])  # nothing ran
    assert ctx.get_state("fresnel_gathers") == gathers
    want = tree_sums(FRS, z, 3, 1.0, 0.0, True)
    assert_words(_gather(torch, d, 3, 1.0, 0.0, True), want, "behind the errors")
    # the shading call on the tree: the checker's bytes, ids rewritten, and the whole range without a shadow light
    ctx.fresnel_gather(*swap(swap(args, 21, None), 23, acc[:4 * SYN_N]))
    ctx.shade_fresnel(*swap(s_args, 9, acc[:4 * SYN_N]))
    ctx.synchronize()
    want = tree_sums(FRS, z, 3, 1.0, 0.0, False)
    assert_words(acc[:4 * SYN_N].cpu().numpy(), want, "no shadow light")
    want_img, want_ids = FRS.shade(z["cc"], SYN_LIGHT, z["normal"], z["t"], z["dirs"], z["ids"], SYN_CAM, z["mat_idx"],
                                   z["mat_list"], want, 0, SYN_N, SYN_N)
    np.testing.assert_array_equal(img.cpu().numpy(), want_img)
    np.testing.assert_array_equal(ids.cpu().numpy(), want_ids)
