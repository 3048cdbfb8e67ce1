"""Refraction: ugrt_scene_transmitlist / _iorlist, ugrt_refract_rays / _next,
ugrt_trace_dda_any_thru / _lights_thru and Renderer / BandedRenderer.display(..., reflect=True, refract=True).

The checker of the rays is tests/refract_ref.c (built here with the oracle's flags): the formula of section 6.6 written
out.  The levels' nearest hits come from the oracle's orc_trace_dda; the images from the existing shading restatements
(reflect_depth_ref.c, occlusion_ref.c, reflect_lights_ref.c, ambient_ref.c) with the `continue` list in the place of
`reflect`.  The see-through any-hit walk has no restatement of its own: the expected flags are oc_trace_any of
tests/occlusion_ref.c on a grid from whose lists the see-through faces were dropped in numpy -- the set of visited cells
does not depend on the lists, so this is the specification exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_ambient as AM
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_shadows as RS
from test_ambient import AO  # noqa: F401  (fixtures)
from test_reflect_lights import RL  # noqa: F401
from test_reflect_shadows import REFS  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))

_p, _f32, _i32, bits, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.LG, RD.UD
W = H = 256
N = W * H
EPS = 1e-3
CALLS = ("ugrt_scene_transmitlist", "ugrt_scene_iorlist", "ugrt_refract_rays", "ugrt_refract_rays_next",
         "ugrt_trace_dda_any_thru", "ugrt_trace_dda_any_lights_thru")
MIRROR, FRONT, BACK, TOTAL = 1, 2, 3, 4  # refract_ref.c's kinds
AO_S = 8
GRID_UNIFORM = 2  # ugrt.GRID_UNIFORM


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class RefractRef:
    def __init__(self, lib):
        self.lib = lib

    def refract_rays(self, cam_pos, t, dirs, ids, mat_idx, reflect, transmit, ior, verts, faces, eps, p0, n, N):
        rays, active, kind = np.zeros(6 * N, np.float32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        reflect = _f32(reflect)
        self.lib.rf_refract_rays(_p(_f32(cam_pos)), _p(_f32(t)), _p(_f32(dirs)), _p(_i32(ids)), _p(_i32(mat_idx)),
                                 _p(reflect), _p(_f32(transmit)), _p(_f32(ior)), C.c_int(len(reflect)),
                                 _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)), C.c_float(eps), C.c_int(p0),
                                 C.c_int(n), _p(rays), _p(active), _p(kind))
        return rays, active, kind

    def refract_rays_next(self, rays, active, hit_t, hit_id, mat_idx, reflect, transmit, ior, verts, faces, eps, p0, n, N):
        rn, an, kind = np.zeros(6 * N, np.float32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        reflect = _f32(reflect)
        self.lib.rf_refract_rays_next(_p(_f32(rays)), _p(_i32(active)), _p(_f32(hit_t)), _p(_i32(hit_id)),
                                      _p(_i32(mat_idx)), _p(reflect), _p(_f32(transmit)), _p(_f32(ior)),
                                      C.c_int(len(reflect)), _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)),
                                      C.c_float(eps), C.c_int(p0), C.c_int(n), _p(rn), _p(an), _p(kind))
        return rn, an, kind


@pytest.fixture(scope="session")
def RF(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("refract_ref") / "librefract_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "refract_ref.c"), "-lm"], check=True, capture_output=True)
    return RefractRef(C.CDLL(out))


_SCENES = {}


def scene(ugrt, name):
    """"glass": scenes.glass(0.1); "mirrors": mirrors(0.1) with its sphere (material 5) made of glass, transmit 0.7 and
    ior 1.5; "hall": hall(0.1), no glass.  The glass scene is also made known to the frames of the other test modules,
    which look their scenes up by name."""
    if name not in _SCENES:
        if name == "glass":
            s = ugrt.scenes.glass(scale=0.1)
            RD.SCENES["glass"], RD.SIZES["glass"] = s, (W, H)
        else:
            s = dict(RD.scene(ugrt, name))
            s["transmit"] = np.zeros(len(s["reflect"]), np.float32)
            s["ior"] = np.ones(len(s["reflect"]), np.float32)
            if name == "mirrors":
                s["transmit"][5], s["ior"][5] = 0.7, 1.5
        s["continue"] = np.where(s["transmit"] > 0, s["transmit"], s["reflect"]).astype(np.float32)
        _SCENES[name] = s
    return _SCENES[name]


def see_through(s):
    """Per face: its material is in range and transmits."""
    m = np.asarray(s["matidx"], np.int64)
    ok = (m >= 0) & (m < len(s["transmit"]))
    return ok & (np.asarray(s["transmit"], np.float32)[np.where(ok, m, 0)] > 0)


def filtered_grid(g, drop):
    """The uniform grid g with every list entry whose face is in `drop` (bool per face) taken out: span and offset
    recomputed, the order inside a list kept."""
    span, offset, vals = g["span"].astype(np.int64), g["offset"].astype(np.int64), g["vals"]
    cell = np.repeat(np.arange(len(span)), span)
    start = np.cumsum(span) - span
    at = np.repeat(offset, span) + (np.arange(int(span.sum())) - np.repeat(start, span))
    entries = vals[at]
    keep = ~drop[entries]
    nspan = np.bincount(cell[keep], minlength=len(span))
    out = dict(g)
    out["vals"] = _u32(np.concatenate([entries[keep], np.zeros(1, entries.dtype)]))  # (never empty)
    out["span"] = _u32(nspan)
    out["offset"] = _u32(np.cumsum(nspan) - nspan)
    return out


_FRAMES = {}


def cpu_frame(O, RF, REFS, ugrt, name, depth, rows=None):
    """The refract frame on the CPU: the oracle's frame (primary, shadows with every chunk, uniform grid), the levels
    from rf_refract_rays / _next + the oracle's trace_dda, per level the occlusion rays towards the light camera's eye
    with the plain flags ("occluded_plain") and the see-through ones ("occluded"), and the images "image_depth" and
    "image_occluded" with the continue list as reflect.  Computed once per key and shared: nobody writes to it."""
    key = (name, depth, rows)
    if key in _FRAMES:
        return _FRAMES[key]
    REF, OC = REFS
    s = scene(ugrt, name)
    setup = ugrt.FrameSetup.from_scene(s)
    want = O.frame(s, setup, W, H, rows=rows, light_grid=LG, reflect=True, uniform_dims=UD, all_chunks=True,
                   reflect_eps=EPS)
    p0, n = want["p0"], want["n"]
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    pr, cam_pos = want["primary"], want["cam"].worldori[:3].copy()
    mats = (s["matidx"], s["reflect"], s["transmit"], s["ior"])
    thru = filtered_grid(want["ugrid"], see_through(s))
    light = want["lcam"].worldori[:3].copy()
    levels = []
    for j in range(depth):
        if j == 0:
            rays, active, kind = RF.refract_rays(cam_pos, pr["t"], pr["dir"], pr["id"], *mats, verts, faces, EPS, p0, n, N)
        else:
            lv = levels[-1]
            rays, active, kind = RF.refract_rays_next(lv["rays"], lv["active"], lv["hit_t"], lv["hit_id"], *mats, verts,
                                                      faces, EPS, p0, n, N)
        hit_t, hit_id, _ = O.trace_dda(want["ugrid"], verts, faces, rays, active, p0, n, N)
        orays, oactive = OC.occlusion_rays(rays, active, hit_t, hit_id, verts, faces, light, EPS, p0, n, N)
        levels.append(dict(rays=rays, active=active, kind=kind, hit_t=hit_t, hit_id=hit_id, orays=orays, oactive=oactive,
                           occluded_plain=OC.trace_any(want["ugrid"], verts, faces, orays, oactive, 1.0, p0, n, N),
                           occluded=OC.trace_any(thru, verts, faces, orays, oactive, 1.0, p0, n, N)))
    stack = {k: np.concatenate([lv[k] for lv in levels]) for k in ("rays", "active", "hit_t", "hit_id", "occluded")}
    args = (want["lcam"].cc, setup.shading_light, pr["normal"], pr["t"], pr["dir"], pr["id"], cam_pos, s["matidx"],
            s["mat_list"], s["continue"], verts, faces, depth, stack["rays"], stack["active"], stack["hit_t"],
            stack["hit_id"])
    img, ids = REF.shade_depth(*args, p0, n, N)
    O.add_shadows(img, want["is_shadowed"], p0, n)
    oimg, oids = OC.shade_depth_occluded(*args, stack["occluded"], p0, n, N)
    O.add_shadows(oimg, want["is_shadowed"], p0, n)
    want.update(levels=levels, stack=stack, thru=thru, light=light, cam_pos=cam_pos, scene=s, image_depth=img,
                mat_ids_depth=ids, image_occluded=oimg, mat_ids_occluded=oids)
    _FRAMES[key] = want
    return want


def kinds(lv):
    return {k: int((lv["kind"] == k).sum()) for k in (MIRROR, FRONT, BACK, TOTAL)}


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_classes_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    for name in ("refract_rays", "refract_rays_next", "trace_dda_any_thru", "trace_dda_any_lights_thru"):
        assert hasattr(ugrt.Context, name), name
    for name in ("h_transmitlist", "h_iorlist"):
        assert hasattr(ugrt.Model, name), name


def test_scene_lists_round_trip_and_a_cache_reports_the_defaults(ugrt, tmp_path):
    g = ugrt.scenes.glass(str(tmp_path), 0.1)
    m = ugrt.Model()
    m.some_material(g["mat"])
    m.load_model(g["obj"])
    np.testing.assert_array_equal(m.h_transmitlist, g["transmit"])
    np.testing.assert_array_equal(m.h_iorlist, g["ior"])
    np.testing.assert_array_equal(m.h_reflectlist, g["reflect"])
    np.testing.assert_array_equal(g["transmit"], np.float32([0, 0, 0, 0, 1 - 0.15, 1 - 0.2, 0, 0, 0]))
    np.testing.assert_array_equal(g["ior"], np.float32([1, 1, 1, 1, 1.5, 1.33, 1, 1, 1]))
    assert g["reflect"][8] == np.float32(0.8)
    # the MTL names d and Ni for the glass materials only
    mtl = open(g["mtl"]).read()
    assert mtl.count("\nNi ") == 2 and mtl.count("\nd 1\n") == 7
    h = ugrt.scenes.hall(str(tmp_path), 0.1)
    mh = ugrt.Model()
    mh.load_model(h["obj"])
    nm = len(mh.h_reflectlist)  # (one entry per material of the mtllib)
    assert nm == len(h["materials"])
    np.testing.assert_array_equal(mh.h_transmitlist, np.zeros(nm, np.float32))
    np.testing.assert_array_equal(mh.h_iorlist, np.ones(nm, np.float32))
    # the cache format does not hold the lists: a cached glass scene is opaque
    cache = str(tmp_path / "glass.cache")
    m.save_cache(cache)
    c = ugrt.Model()
    c.load_cache(cache)
    np.testing.assert_array_equal(c.h_reflectlist, g["reflect"])
    np.testing.assert_array_equal(c.h_transmitlist, np.zeros(9, np.float32))
    np.testing.assert_array_equal(c.h_iorlist, np.ones(9, np.float32))
    # a dissolve outside [0, 1] is clamped
    odd = tmp_path / "odd.mtl"
    odd.write_text("newmtl a\nd -0.5\nnewmtl b\nd 2\nNi 0\nnewmtl c\n")
    (tmp_path / "odd.obj").write_text("mtllib odd.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl a\nf 1 2 3\n")
    o = ugrt.Model()
    o.load_model(str(tmp_path / "odd.obj"))
    np.testing.assert_array_equal(o.h_transmitlist, np.float32([1, 0, 0]))
    np.testing.assert_array_equal(o.h_iorlist, np.float32([1, 0, 1]))


def test_refract_is_checked_before_anything_runs(ugrt):
    from importlib import import_module

    rmod = import_module(ugrt.__name__ + ".renderer")
    with pytest.raises(ValueError):
        rmod.check_refract(True, False)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError):
            rmod.check_refract(bad, True)
    assert rmod.check_refract(True, True) is True
    assert rmod.check_refract(np.bool_(True), True) is True
    assert rmod.check_refract(False, False) is False and rmod.check_refract(False, True) is False

    class Never:
        def __getattr__(self, name):
            raise AssertionError("display reached %s" % name)

    import types

    for cls in (ugrt.Renderer, ugrt.BandedRenderer):
        fake = types.SimpleNamespace(ctx=Never(), aux=None)
        with pytest.raises(ValueError):
            cls.display(fake, None, reflect=False, refract=True)
        with pytest.raises(ValueError):
            cls.display(fake, None, reflect=True, refract=1)


def test_stages_enqueue_the_refract_calls_only_in_a_refract_frame(ugrt):
    from importlib import import_module

    rmod = import_module(ugrt.__name__ + ".renderer")
    f = RS._fake_frame(2)
    f.d_transmit, f.d_ior, f.d_continue, f.refract = "tr", "ni", "cont", True
    f.occluded_lights = ["ol1", "ol2"]
    c = RS._Recorder()
    rmod.reflect_rays(c, f, "cam")
    rmod.trace_reflections(c, f, 2, shadow_light=(1.0, 2.0, 3.0))
    rmod.trace_reflections(c, f, 1, shadow_lights=[(1.0, 2.0, 3.0)])
    assert [x[0] for x in c.calls] == ["refract_rays", "trace_dda", "occlusion_rays", "trace_dda_any_thru", "refract_rays_next",
                                       "trace_dda", "occlusion_rays", "trace_dda_any_thru", "trace_dda", "occlusion_rays",
                                       "trace_dda_any_lights_thru"]
    assert c.calls[0][6:10] == ("refl", "tr", "ni", 3) and c.calls[4][6:10] == ("refl", "tr", "ni", 3)
    assert c.calls[3][-3:] == ("mi", "tr", 3) and c.calls[-1][-3:] == ("mi", "tr", 3)
    for depth, shadows in ((1, False), (2, False), (2, True)):
        c, g = RS._Recorder(), RS._fake_frame(depth)
        g.d_continue, g.refract = "cont", True
        rmod.shade_frame(c, g, "cam", 1, False, True, depth, shadows)
        assert c.calls[0][9] == "cont", c.calls[0]
    f.refract = False
    c = RS._Recorder()
    rmod.reflect_rays(c, f, "cam")
    rmod.shade_frame(c, f, "cam", 1, False, True, 2)
    assert [x[0] for x in c.calls] == ["reflect_rays", "shade_reflect_depth"] and c.calls[1][9] == "refl"


def test_glass_solids_are_closed_and_wound_outwards(ugrt):
    s = scene(ugrt, "glass")
    v, f, m = np.asarray(s["verts"], np.float64), np.asarray(s["faces"]), np.asarray(s["matidx"])
    for mat in (4, 5):
        fs = f[m == mat]
        assert len(fs) >= 12
        a, b, c = v[fs[:, 0]], v[fs[:, 1]], v[fs[:, 2]]
        centroid = v[np.unique(fs)].mean(0)
        out = np.einsum("ij,ij->i", np.cross(b - a, c - a), (a + b + c) / 3 - centroid)
        assert (out > 0).all(), (mat, int((out <= 0).sum()))
        # closed: every edge (by position) is used by exactly two faces, once in each direction
        pos = {tuple(np.round(p, 6)) for p in v[np.unique(fs)]}
        index = {p: k for k, p in enumerate(sorted(pos))}
        ids = np.array([[index[tuple(np.round(v[i], 6))] for i in tri] for tri in fs])
        edges = {}
        for tri in ids:
            for e in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
                edges[e] = edges.get(e, 0) + 1
        assert all(n == 1 and edges.get((e[1], e[0])) == 1 for e, n in edges.items()), mat


def test_existing_scenes_did_not_change(ugrt, tmp_path):
    """The MTL writer's new branch leaves the other scenes' files as they were: "d 1" and no Ni per material."""
    s = ugrt.scenes.mirrors(str(tmp_path), 0.1)
    mtl = open(s["mtl"]).read()
    assert "Ni" not in mtl and mtl.count("\nd 1\n") == len(s["materials"])
    assert "transmit" not in s and "ior" not in s


def test_zero_transmit_gives_the_reflected_rays(ugrt, O, RF, REFS):
    """hall 0.1, 256 x 256: with transmit all zero rf_refract_rays writes the oracle's reflected rays bit for bit, and
    rf_refract_rays_next those of the depth restatement."""
    want = cpu_frame(O, RF, REFS, ugrt, "hall", 2)
    assert int(want["active"].sum()) > 1000
    l1, l2 = want["levels"]
    np.testing.assert_array_equal(l1["active"], want["active"])
    np.testing.assert_array_equal(bits(l1["rays"]), bits(want["rays"]))
    assert set(np.unique(l1["kind"])) == {0, MIRROR}
    s = scene(ugrt, "hall")
    rays, active = REFS[0].reflect_rays_next(l1["rays"], l1["active"], l1["hit_t"], l1["hit_id"], s["matidx"], s["reflect"],
                                             s["verts"], s["faces"], EPS, 0, N, N)
    assert int(active.sum()) > 100
    np.testing.assert_array_equal(l2["active"], active)
    np.testing.assert_array_equal(bits(l2["rays"]), bits(rays))
    np.testing.assert_array_equal(l1["occluded"], l1["occluded_plain"])


# -- the formula on a slab: faces z = 0 and z = 1 of a solid that lies between them, wound outwards

SLAB_VERTS = np.float32([(-50, -50, 0), (50, -50, 0), (0, 50, 0), (-50, -50, 1), (50, -50, 1), (0, 50, 1)])
SLAB_FACES = np.int32([(0, 2, 1), (3, 4, 5)])  # normals (0, 0, -1) and (0, 0, 1)
ANGLES = np.deg2rad(np.float64([0, 10, 20, 30, 40, 41.8, 60, 80]))


def _slab_ray(RF, o, d, t, face, ior, transmit=0.9, reflect=0.0):
    rays, active, kind = RF.refract_rays(o, np.float32([t]), np.float32(d), np.int32([face]), np.int32([0, 0]),
                                         np.float32([reflect]), np.float32([transmit]), np.float32([ior]), SLAB_VERTS,
                                         SLAB_FACES, EPS, 0, 1, 1)
    assert active[0] == 1
    return rays[:3].copy(), rays[3:].copy(), int(kind[0])


def _reflect_formula(o, d, t, n):
    """d_reflect_ray's operations in float32, n already turned against d."""
    f = np.float32
    o, d, n, t = np.float32(o), np.float32(d), np.float32(n), f(t)
    dn = f(f(f(d[0] * n[0]) + f(d[1] * n[1])) + f(d[2] * n[2]))
    P = np.float32([f(o[k] + f(t * d[k])) for k in range(3)])
    return (np.float32([f(P[k] + f(f(EPS) * n[k])) for k in range(3)]),
            np.float32([f(d[k] - f(f(f(2.0) * dn) * n[k])) for k in range(3)]))


def test_the_formula_obeys_snell_on_a_slab(RF):
    """Index 1.5, eight rays at 0..80 degrees going up through z = 0 and out through z = 1: the exit direction is the
    entry direction, all three directions and the normal lie in one plane, Snell's law holds inside; from inside, the
    rays beyond asin(1 / 1.5) = 41.81 degrees are mirrored with the reflect formula's bits and the others are not; an
    index of 0, -1 or NaN is 1."""
    nz = np.float64([0, 0, 1])
    for a in ANGLES:
        phi = 0.7
        d = np.float32([np.sin(a) * np.cos(phi), np.sin(a) * np.sin(phi), np.cos(a)]) * np.float32(2.5)  # not a unit vector
        o = np.float32([0.3, -0.2, -1.0])
        t = np.float32(1.0 / d[2])
        o1, d1, k1 = _slab_ray(RF, o, d, t, 0, 1.5)
        assert k1 == FRONT and o1[2] > 0  # through z = 0, on the far side
        sin_in, sin_t = np.sin(a), np.linalg.norm(np.cross(d1.astype(np.float64), nz)) / np.linalg.norm(d1)
        assert abs(sin_in - 1.5 * sin_t) < 1e-6
        t2 = np.float32((1.0 - o1[2]) / d1[2])
        o2, d2, k2 = _slab_ray(RF, o1, d1, t2, 1, 1.5)
        assert k2 == BACK and o2[2] > 1
        u = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64))
        assert np.abs(d2.astype(np.float64) - u).max() < 1e-6, (np.rad2deg(a), d2, u)
        for w in (d1, d2):
            assert abs(np.dot(np.cross(u, nz), w.astype(np.float64))) < 1e-6
        for bad in (0.0, -1.0, np.nan):
            _, db, kb = _slab_ray(RF, o, d, t, 0, bad)
            assert kb == FRONT and np.abs(db.astype(np.float64) - u).max() < 1e-6
    critical = np.arcsin(1 / 1.5)
    for a in np.deg2rad(np.float64([0, 10, 20, 30, 40, 41.5, 42.1, 50, 60, 80])):
        d = np.float32([np.sin(a), 0, np.cos(a)]) * np.float32(0.8)
        o = np.float32([0.1, 0.1, 0.5])
        t = np.float32(0.5 / d[2])
        o2, d2, k2 = _slab_ray(RF, o, d, t, 1, 1.5)
        if a > critical:
            wo, wd = _reflect_formula(o, d, t, [0, 0, -1])
            assert k2 == TOTAL
            np.testing.assert_array_equal(bits(o2), bits(wo))
            np.testing.assert_array_equal(bits(d2), bits(wd))
        else:
            assert k2 == BACK and o2[2] > 1 and d2[2] > 0
    # a material with both transmits; one with reflect alone mirrors, with the reflect formula's bits
    d, o = np.float32([0.3, 0.1, 1.0]), np.float32([0, 0, -1])
    assert _slab_ray(RF, o, d, 1.0, 0, 1.5, 0.5, 0.5)[2] == FRONT
    o2, d2, k2 = _slab_ray(RF, o, d, 1.0, 0, 1.5, 0.0, 0.5)
    wo, wd = _reflect_formula(o, d, 1.0, [0, 0, -1])
    assert k2 == MIRROR
    np.testing.assert_array_equal(bits(o2), bits(wo))
    np.testing.assert_array_equal(bits(d2), bits(wd))


# per level of glass(0.1) at 256 x 256: (active rays, refracted from the front, from the back, totally reflected, mirrored)
GLASS_LEVELS = [(39882, 34593, 0, 0, 5289), (35520, 927, 31895, 2698, 0), (5511, 0, 2965, 660, 1886), (660, 0, 118, 542, 0)]


def test_glass_frame_is_not_vacuous(ugrt, O, RF, REFS):
    """What DESIGN.md section 6.6 records: per level the active rays and how they were made.  All three kinds of glass
    ray occur by level 3."""
    want = cpu_frame(O, RF, REFS, ugrt, "glass", 4)
    got = []
    for j, lv in enumerate(want["levels"]):
        k = kinds(lv)
        got.append((int(lv["active"].sum()), k[FRONT], k[BACK], k[TOTAL], k[MIRROR]))
        print("glass level %d: %d active, %d front, %d back, %d total reflection, %d mirrored" % ((j + 1,) + got[-1]))
    seen = np.sum(got[:3], axis=0)
    assert seen[1] > 0 and seen[2] > 0 and seen[3] > 0, got
    assert got == GLASS_LEVELS
    # the glass changes the picture: against the reflect frame, which treats transmit as absent
    s = scene(ugrt, "glass")
    plain = RS.cpu_frame(O, REFS, ugrt, "glass", W, H, 4)
    assert int((plain["image_depth"] != want["image_depth"]).reshape(-1, 3).any(1).sum()) > 3000
    assert int((see_through(s)).sum()) == int(np.isin(s["matidx"], (4, 5)).sum()) > 0


BALL_CENTRE, BALL_RADIUS = np.float64([5.5, 2.4, 1.35]), 1.1
GLASS_OCCLUSION = (41446, 12195)  # (rays the plain walk marks and the see-through walk does not, of them from inside the ball)


def test_glass_does_not_occlude_and_every_opaque_triangle_agrees(ugrt, O, RF, REFS):
    want = cpu_frame(O, RF, REFS, ugrt, "glass", 4)
    s = scene(ugrt, "glass")
    opaque = np.asarray(s["faces"])[~see_through(s)]
    freed = inside = 0
    for j, lv in enumerate(want["levels"]):
        brute = REFS[1].brute_any(s["verts"], opaque, lv["orays"], lv["oactive"], 1.0, 0, N, N)
        np.testing.assert_array_equal(lv["occluded"], brute, err_msg="level %d" % (j + 1))
        assert not (lv["occluded"] & ~lv["occluded_plain"]).any()
        diff = (lv["occluded_plain"] == 1) & (lv["occluded"] == 0)
        o = lv["orays"].reshape(-1, 6)[:, :3].astype(np.float64)
        freed += int(diff.sum())
        inside += int((diff & (np.linalg.norm(o - BALL_CENTRE, axis=1) < BALL_RADIUS)).sum())
    print("glass levels 1..4: %d occlusion rays freed by the see-through walk, %d of them start inside the ball" % (freed, inside))
    assert freed >= 1000 and inside >= 1
    assert (freed, inside) == GLASS_OCCLUSION
    changed = (want["image_occluded"] != want["image_depth"]).reshape(-1, 3).any(1)
    assert int(changed.sum()) > 100


# -- synthetic lists: test_reflect_shadows' any-hit scene with the lattice triangles of a cell at staggered heights, so that
# one ray can pass two triangles of one list

SYN_N = 4096
SYN_TRANSMIT = np.float32([0.0, 0.5])
_SYN = {}


def _syn_point(n, m):
    i, j = RS.SYN_CELLS[n]
    cx, cy = RS._lattice_centre(i, j, m)
    return np.float64([cx, cy - 0.005, 1.3 + 0.4 * m / n])


def syn_glass(O):
    """verts, faces, grid, rays as test_reflect_shadows builds them, but triangle m of the cell with n triangles lies at
    z = 1.3 + 0.4 m / n (still in the layer k = 1, so the list lengths are the same); every third face is see-through
    (material 1).  Pixels 3600.. hold the pairs: a ray through triangle m1 and then m2 > m1 of one list, m1 see-through;
    "opaque": m2 is not (the ray stays occluded), "clear": m2 is see-through too."""
    if _SYN:
        return _SYN
    verts, faces, first = RS.synthetic_scene()
    verts = verts.copy()
    for n in RS.SYN_CELLS:
        for m in range(n):
            verts[3 * (first[n] + m):3 * (first[n] + m) + 3, 2] = np.float32(1.3 + 0.4 * m / n)
    grid = O.grid_uniform(faces, verts, verts.min(0), verts.max(0), RS.SYN_DIMS)
    rays, _, _ = RS.synthetic_rays(grid["ug"], verts)
    rays = rays.reshape(-1, 6).copy()
    matidx = (np.arange(len(faces)) % 3 == 0).astype(np.int32)
    pairs, q = {"opaque": [], "clear": []}, 3600
    for n in (9, 63, 64, 65, 129):
        glass = [m for m in range(n) if matidx[first[n] + m] == 1]
        solid = [m for m in range(n) if matidx[first[n] + m] == 0]
        for m1 in (glass[0], glass[len(glass) // 3]):
            for kind, later in (("opaque", solid), ("clear", glass)):
                # the last of the list, and for the lists of more than one round the first of a later round
                m2s = {max(later)} | (set([m for m in later if m >= 64][:1]) if n > 64 and m1 < 64 else set())
                for m2 in sorted(m2s):
                    if m2 <= m1:
                        continue
                    p1, p2 = _syn_point(n, m1), _syn_point(n, m2)
                    o = p1 - 0.1 * (p2 - p1) / np.linalg.norm(p2 - p1)
                    rays[q] = list(o) + list((p2 - o) * 1.5)
                    pairs[kind].append((q, n, m1, m2))
                    q += 1
    assert q < SYN_N
    _SYN.update(verts=verts, faces=faces, first=first, grid=grid, rays=_f32(rays.reshape(-1)), matidx=matidx, pairs=pairs,
                thru=filtered_grid(grid, matidx == 1))
    return _SYN


def test_synthetic_lists_put_glass_in_front_of_opaque_triangles(O, REFS):
    """CPU: the list lengths are those of test_reflect_shadows; every "opaque" pair ray hits a see-through and an opaque
    triangle, every "clear" pair ray two see-through ones (and
    at least half of them nothing else); the filtered walk equals brute force over the opaque faces;
    and the pairs cover the same list, the same round and a later round."""
    OC, S = REFS[1], syn_glass(O)
    g, dims = S["grid"], RS.SYN_DIMS
    for n, (i, j) in RS.SYN_CELLS.items():
        assert int(g["span"][(i * dims[1] + j) * dims[2] + 1]) == n
    act = np.ones(SYN_N, np.int32)
    glass, solid = S["faces"][S["matidx"] == 1], S["faces"][S["matidx"] == 0]
    for t_max in (1.0, 3e38):
        args = (S["rays"], act, t_max, 0, SYN_N, SYN_N)
        plain = OC.trace_any(g, S["verts"], S["faces"], *args)
        thru = OC.trace_any(S["thru"], S["verts"], S["faces"], *args)
        np.testing.assert_array_equal(thru, OC.brute_any(S["verts"], solid, *args))
        through_glass = OC.brute_any(S["verts"], glass, *args)
        np.testing.assert_array_equal(plain, thru | through_glass)
        assert int((plain & ~thru).sum()) > 300 and int(thru.sum()) > 500 and int((plain == 0).sum()) > 500
        for q, n, m1, m2 in S["pairs"]["opaque"]:
            assert through_glass[q] == 1 and thru[q] == 1, (n, m1, m2)
        for q, n, m1, m2 in S["pairs"]["clear"]:
            assert through_glass[q] == 1 and plain[q] == 1, (n, m1, m2)
        # (a clear ray may still meet an opaque triangle of the lattice on its way; most do not)
        assert sum(int(thru[q] == 0) for q, _, _, _ in S["pairs"]["clear"]) >= len(S["pairs"]["clear"]) // 2
    later = [(n, m1, m2) for _, n, m1, m2 in S["pairs"]["opaque"] if m1 // 64 < m2 // 64]
    same = [(n, m1, m2) for _, n, m1, m2 in S["pairs"]["opaque"] if m1 // 64 == m2 // 64 and n >= 64]
    assert later and same and len(S["pairs"]["clear"]) >= 5


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def make(ugrt, s, rows=None, **kw):
    ctx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD, rows=rows)
    return ctx, ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], s["transmit"], s["ior"],
                              **kw)


def setup_for(ugrt, s, lights=None):
    return ugrt.FrameSetup.from_scene(s, lights=lights)


def assert_levels(r, want, depth):
    a, b = want["p0"], want["p0"] + want["n"]
    for j, w in enumerate(want["levels"][:depth]):
        what = "level %d" % (j + 1)
        np.testing.assert_array_equal(r.active_levels[j].cpu().numpy()[a:b], w["active"][a:b], err_msg=what)
        np.testing.assert_array_equal(bits(r.rays_levels[j].cpu().numpy()[6 * a:6 * b]), bits(w["rays"][6 * a:6 * b]), err_msg=what)
        np.testing.assert_array_equal(r.hit_id_levels[j].cpu().numpy()[a:b], w["hit_id"][a:b], err_msg=what)
        np.testing.assert_array_equal(bits(r.hit_t_levels[j].cpu().numpy()[a:b]), bits(w["hit_t"][a:b]), err_msg=what)


def _bytes(t, torch):
    return t.contiguous().view(torch.uint8)


@pytest.mark.gpu
def test_zero_transmit_gives_the_reflect_calls_bytes(ugrt, O, RF, REFS, torch):
    """hall 0.1: refract_rays and refract_rays_next with transmit all zero against reflect_rays and reflect_rays_next."""
    s = scene(ugrt, "hall")
    ctx, r = make(ugrt, s)
    r.display(setup_for(ugrt, s), shadows=True, reflect=True, shade=False)
    r._ensure_reflect_buffers(2)
    mats = (r.d_matidx, r.d_reflect)
    geo = (r.num_materials, r.d_verts, r.d_faces, r.reflect_eps)
    ctx.reflect_rays(r.cam_pos, r.t, r.dir, r.intersect_id, *mats, *geo, r.rays, r.active)
    ctx.grid_build_uniform(r.d_faces, r.d_verts, r.F, r.bbmin, r.bbmax)
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    ctx.trace_dda(uvalue, uspan, uoffset, r.d_verts, r.d_faces, r.rays, r.active, r.hit_t, r.hit_id)
    ctx.reflect_rays_next(r.rays, r.active, r.hit_t, r.hit_id, *mats, *geo, r.rays_levels[1], r.active_levels[1])
    rays = torch.full((2, 6 * N), 7.0, device=ctx.device)
    active = torch.full((2, N), 7, dtype=torch.int32, device=ctx.device)
    assert not bool(r.d_transmit.any())
    ctx.refract_rays(r.cam_pos, r.t, r.dir, r.intersect_id, *mats, r.d_transmit, r.d_ior, *geo, rays[0], active[0])
    ctx.refract_rays_next(r.rays, r.active, r.hit_t, r.hit_id, *mats, r.d_transmit, r.d_ior, *geo, rays[1], active[1])
    ctx.synchronize()
    for j in range(2):
        assert torch.equal(_bytes(rays[j], torch), _bytes(r.rays_levels[j], torch)), j
        assert torch.equal(active[j], r.active_levels[j]), j
        assert int(active[j].sum()) > 100
    want = cpu_frame(O, RF, REFS, ugrt, "hall", 2)
    for j in range(2):
        np.testing.assert_array_equal(bits(rays[j].cpu().numpy()), bits(want["levels"][j]["rays"]))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["glass", "mirrors"])
def test_levels_equal_the_checker(ugrt, O, RF, REFS, torch, name, depth):
    """Rays, active, hit_t and hit_id of every level, and the image, on glass and on mirrors with a glass sphere."""
    s = scene(ugrt, name)
    want = cpu_frame(O, RF, REFS, ugrt, name, depth)
    ctx, r = make(ugrt, s)
    r.display(setup_for(ugrt, s), shadows=True, reflect=True, refract=True, bounces=depth)
    ctx.synchronize()
    assert_levels(r, want, depth)
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), want["mat_ids_depth"])
    np.testing.assert_array_equal(r.image.cpu().numpy(), want["image_depth"])
    k = kinds(want["levels"][min(depth, 2) - 1])
    assert k[FRONT] + k[BACK] > 100, k


def _walk_thru(ctx, r, torch, d_rays, d_active, t_max, d_transmit, verts=None, faces=None):
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(GRID_UNIFORM)
    occ = torch.full((N,), -7, dtype=torch.int32, device=ctx.device)
    ctx.trace_dda_any_thru(uvalue, uspan, uoffset, r.d_verts if verts is None else verts, r.d_faces if faces is None else faces,
                           d_rays, d_active, t_max, occ, r.d_matidx, d_transmit, r.num_materials)
    return occ


@pytest.mark.gpu
def test_see_through_walk_on_the_glass_scene(ugrt, O, RF, REFS, torch):
    """trace_dda_any_thru on the occlusion rays of levels 1..4 against the filtered CPU walk; with zero transmit it is
    trace_dda_any; vertex arrays that are not the grid's own take the gathering kernel."""
    s = scene(ugrt, "glass")
    want = cpu_frame(O, RF, REFS, ugrt, "glass", 4)
    ctx, r = make(ugrt, s)
    r.display(setup_for(ugrt, s), shadows=True, reflect=True, refract=True, bounces=4, reflect_shadows=True)
    ctx.synchronize()
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    zero = torch.zeros_like(r.d_transmit)
    for j, lv in enumerate(want["levels"]):
        what = "level %d" % (j + 1)
        np.testing.assert_array_equal(r.occluded_levels[j].cpu().numpy(), lv["occluded"], err_msg=what)
        d_rays, d_act = ctx.upload(lv["orays"]), ctx.upload(lv["oactive"])
        got = _walk_thru(ctx, r, torch, d_rays, d_act, 1.0, r.d_transmit)
        gathered = _walk_thru(ctx, r, torch, d_rays, d_act, 1.0, r.d_transmit, r.d_verts.clone(), r.d_faces.clone())
        opaque = _walk_thru(ctx, r, torch, d_rays, d_act, 1.0, zero)
        plain = torch.full((N,), -7, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda_any(uvalue, uspan, uoffset, r.d_verts, r.d_faces, d_rays, d_act, 1.0, plain)
        ctx.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), lv["occluded"], err_msg=what)
        np.testing.assert_array_equal(gathered.cpu().numpy(), lv["occluded"], err_msg=what)
        np.testing.assert_array_equal(plain.cpu().numpy(), lv["occluded_plain"], err_msg=what)
        assert torch.equal(opaque, plain), what
    assert int(sum(((lv["occluded_plain"] == 1) & (lv["occluded"] == 0)).sum() for lv in want["levels"])) >= 1000


@pytest.mark.gpu
def test_see_through_walk_on_synthetic_lists(ugrt, O, REFS, torch):
    """List lengths 1, 7, 8, 9, 63, 64, 65, 129 with every third face see-through; any_coop 1 (every list by the wave),
    8, and 2^30 (every list by its lane); t_max 1 and 3e38; the records' and the gathering kernel."""
    OC, S = REFS[1], syn_glass(O)
    ctx, dv, df, grid = RS._syn_context(ugrt, S)
    d_rays, d_mat, d_tr = ctx.upload(S["rays"]), ctx.upload(S["matidx"]), ctx.upload(SYN_TRANSMIT)
    d_zero = ctx.upload(np.zeros(2, np.float32))
    act = np.ones(SYN_N, np.int32)
    a67 = RS.syn_actives()["67"]
    for coop in (1, 8, 1 << 30):
        ctx.set_option("any_coop", coop)
        for t_max in (1.0, 3e38):
            for active in (act, a67):
                want = OC.trace_any(S["thru"], S["verts"], S["faces"], S["rays"], active, t_max, 0, SYN_N, SYN_N)
                plain = OC.trace_any(S["grid"], S["verts"], S["faces"], S["rays"], active, t_max, 0, SYN_N, SYN_N)
                d_act = ctx.upload(active)
                for v, f in ((dv, df), (dv.clone(), df.clone())):
                    occ = torch.full((SYN_N,), -7, dtype=torch.int32, device=ctx.device)
                    ctx.trace_dda_any_thru(grid[0], grid[1], grid[2], v, f, d_rays, d_act, float(t_max), occ, d_mat, d_tr, 2)
                    opq = torch.full((SYN_N,), -7, dtype=torch.int32, device=ctx.device)
                    ctx.trace_dda_any_thru(grid[0], grid[1], grid[2], v, f, d_rays, d_act, float(t_max), opq, d_mat, d_zero, 2)
                    ctx.synchronize()
                    np.testing.assert_array_equal(occ.cpu().numpy(), want, err_msg="any_coop %d t_max %g" % (coop, t_max))
                    np.testing.assert_array_equal(opq.cpu().numpy(), plain, err_msg="any_coop %d t_max %g" % (coop, t_max))
    # a material index out of range is opaque
    ctx.set_option("any_coop", -1)
    occ = torch.full((SYN_N,), -7, dtype=torch.int32, device=ctx.device)
    ctx.trace_dda_any_thru(grid[0], grid[1], grid[2], dv, df, d_rays, ctx.upload(act), 1.0, occ, d_mat, d_tr, 1)
    ctx.synchronize()
    np.testing.assert_array_equal(occ.cpu().numpy(), OC.trace_any(S["grid"], S["verts"], S["faces"], S["rays"], act, 1.0, 0,
                                                                  SYN_N, SYN_N))


def _glass_lights(ugrt, O):
    s = scene(ugrt, "glass")
    lw = TL.cpu_frame(O, ugrt, "glass", W, H, nlights=3)
    eyes = [O.cam_from(lt["params"], 45.0, 1.0).worldori[:3].copy() for lt in lw["lights"]]
    return s, lw, eyes


@pytest.mark.gpu
def test_lights_walk_equals_three_single_walks(ugrt, O, RF, REFS, torch):
    s, lw, eyes = _glass_lights(ugrt, O)
    want = cpu_frame(O, RF, REFS, ugrt, "glass", 4)
    ctx, r = make(ugrt, s)
    r.display(setup_for(ugrt, s), shadows=True, reflect=True, refract=True, bounces=1)
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    for j in (0, 1):
        lv = want["levels"][j]
        d_rays, d_act = ctx.upload(lv["orays"]), ctx.upload(lv["oactive"])
        for v, f in ((r.d_verts, r.d_faces), (r.d_verts.clone(), r.d_faces.clone())):
            occ = torch.full((4, N), -7, dtype=torch.int32, device=ctx.device)
            ctx.trace_dda_any_lights_thru(uvalue, uspan, uoffset, v, f, d_rays, d_act, [tuple(e) for e in eyes], occ, r.d_matidx,
                                          r.d_transmit, r.num_materials)
            ctx.synchronize()
            assert bool((occ[3] == -7).all())
            for l, eye in enumerate(eyes):
                o = lv["orays"].reshape(-1, 6)[:, :3]
                rays = np.concatenate([o, np.float32(eye)[None, :] - o], 1).astype(np.float32).reshape(-1)
                rays[np.repeat(lv["oactive"] == 0, 6)] = 0
                single = _walk_thru(ctx, r, torch, ctx.upload(rays), d_act, 1.0, r.d_transmit)
                ctx.synchronize()
                assert torch.equal(occ[l], single), (j, l)
                cpu = REFS[1].trace_any(want["thru"], s["verts"], s["faces"], rays, lv["oactive"], 1.0, 0, N, N)
                np.testing.assert_array_equal(single.cpu().numpy(), cpu)
        zero = torch.zeros_like(r.d_transmit)
        a = torch.full((3, N), -7, dtype=torch.int32, device=ctx.device)
        b = torch.full((3, N), -7, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda_any_lights_thru(uvalue, uspan, uoffset, r.d_verts, r.d_faces, d_rays, d_act, [tuple(e) for e in eyes], a,
                                      r.d_matidx, zero, r.num_materials)
        ctx.trace_dda_any_lights(uvalue, uspan, uoffset, r.d_verts, r.d_faces, d_rays, d_act, [tuple(e) for e in eyes], b)
        ctx.synchronize()
        assert torch.equal(a, b) and int((a != occ[:3]).sum()) > 100


@pytest.mark.gpu
def test_launch_options_and_a_band_change_no_flag(ugrt, O, RF, REFS, torch):
    s = scene(ugrt, "glass")
    want = cpu_frame(O, RF, REFS, ugrt, "glass", 4)
    lv = want["levels"][1]
    for opts, rows in (({"any_rays_per_wave": 1}, None), ({"any_rays_per_wave": 7}, None), ({"any_rays_per_wave": 64}, None),
                       ({"dda_blocks": 1}, None), ({}, (5, 21))):
        ctx, r = make(ugrt, s, rows=rows)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.grid_build_uniform(r.d_faces, r.d_verts, r.F, r.bbmin, r.bbmax)
        got = _walk_thru(ctx, r, torch, ctx.upload(lv["orays"]), ctx.upload(lv["oactive"]), 1.0, r.d_transmit)
        ctx.synchronize()
        expect = np.full(N, -7, np.int32)
        expect[ctx.p0:ctx.p0 + ctx.npix] = lv["occluded"][ctx.p0:ctx.p0 + ctx.npix]
        np.testing.assert_array_equal(got.cpu().numpy(), expect, err_msg=str((opts, rows)))
        if rows is not None:
            assert (ctx.p0, ctx.npix) == (5 * 8 * W, 16 * 8 * W)


@pytest.mark.gpu
def test_frames_equal_the_cpu_composition(ugrt, O, RF, REFS, RL, AO, torch):
    """Depth 4 on glass: the refract frame; with reflect_shadows; under three lights with reflect_lights and
    reflect_shadows; with ao = 8."""
    s, lw, eyes = _glass_lights(ugrt, O)
    want = cpu_frame(O, RF, REFS, ugrt, "glass", 4)
    setup = setup_for(ugrt, s)
    OC = REFS[1]
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    pr, st = want["primary"], want["stack"]
    ctx, r = make(ugrt, s)
    kw = dict(shadows=True, reflect=True, refract=True, bounces=4)
    r.display(setup, **kw)
    ctx.synchronize()
    assert_levels(r, want, 4)
    np.testing.assert_array_equal(r.image.cpu().numpy(), want["image_depth"])
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), want["mat_ids_depth"])
    # ao = 8 behind it: glass encloses, so the mask is the plain hemisphere walk's
    radius = float(np.float32(0.05 * float((verts.reshape(-1, 3).max(0) - verts.reshape(-1, 3).min(0)).max())))
    orays, oactive = AO.rays(want["cam_pos"], pr["t"], pr["dir"], pr["id"], verts, faces, EPS, 0, N, N)
    mask = AM.cpu_mask(OC, AO, want["ugrid"], verts, faces, orays, oactive, ugrt.scenes.ao_directions(AO_S), radius, 0, N, N)
    r.display(setup, ao=AO_S, ao_radius=radius, **kw)
    ctx.synchronize()
    np.testing.assert_array_equal(AM._words(r.ao_mask), mask)
    shaded = AO.shade(want["image_depth"], mask, AO_S, 0, N)
    np.testing.assert_array_equal(r.image.cpu().numpy(), shaded)
    assert int((shaded != want["image_depth"]).sum()) > 1000
    # reflect_shadows: the walk that sees through glass
    r.display(setup, reflect_shadows=True, **kw)
    ctx.synchronize()
    assert_levels(r, want, 4)
    for j, lv in enumerate(want["levels"]):
        np.testing.assert_array_equal(r.occluded_levels[j].cpu().numpy(), lv["occluded"], err_msg="level %d" % (j + 1))
    np.testing.assert_array_equal(r.image.cpu().numpy(), want["image_occluded"])
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), want["mat_ids_occluded"])
    assert int((want["image_occluded"] != want["image_depth"]).sum()) > 100
    # three lights
    lights = lw["lights"]
    occluded = np.zeros((4, 3, N), np.int32)
    for j, lv in enumerate(want["levels"]):
        for l, eye in enumerate(eyes):
            o_r, o_a = OC.occlusion_rays(lv["rays"], lv["active"], lv["hit_t"], lv["hit_id"], verts, faces, eye, EPS, 0, N, N)
            occluded[j, l] = OC.trace_any(want["thru"], verts, faces, o_r, o_a, 1.0, 0, N, N)
    flags = np.stack([lt["flags"] for lt in lights])
    img, ids = RL.shade(lights[-1]["cc"], pr["normal"], pr["t"], pr["dir"], pr["id"], want["cam_pos"], s["matidx"], s["mat_list"],
                        s["continue"], verts, faces, 4, st["rays"], st["active"], st["hit_t"], st["hit_id"],
                        [lt["pos"] for lt in lights], flags, occluded, 0, N, N)
    r.display(setup_for(ugrt, s, [(lt["params"], lt["pos"]) for lt in lights]), reflect_shadows=True, reflect_lights=True, **kw)
    ctx.synchronize()
    assert_levels(r, want, 4)
    np.testing.assert_array_equal(r.occluded_lights.cpu().numpy(), occluded)
    np.testing.assert_array_equal(r.shadowed_lights[:3].cpu().numpy(), flags)
    np.testing.assert_array_equal(r.image.cpu().numpy(), img)
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), ids)
    assert int((occluded[:, 0] != occluded[:, 1]).sum()) > 100


FORM_ARRAYS = ("image", "intersect_id", "is_shadowed")
FORM_LEVELS = ("rays_levels", "active_levels", "hit_t_levels", "hit_id_levels", "occluded_levels")


@pytest.mark.gpu
def test_renderer_forms_agree(ugrt, O, RF, REFS, torch):
    """Depth 3 with reflect_shadows: the overlapped, the inline two-stream and the banded renderer (2 bands) against the
    one-stream frame, which is the CPU frame."""
    s = scene(ugrt, "glass")
    setup = setup_for(ugrt, s)
    want = cpu_frame(O, RF, REFS, ugrt, "glass", 3)
    kw = dict(shadows=True, reflect=True, refract=True, bounces=3, reflect_shadows=True)
    outs = {}
    glass = (s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], s["transmit"], s["ior"])
    for form in ("plain", "overlapped", "inline", "banded"):
        if form == "banded":
            r = ugrt.BandedRenderer(ugrt.Context, W, H, *glass, bands=2, light_grid=LG, uniform_dims=UD,
                                    flags=ugrt.FLAG_SHADOW_ALL_CHUNKS)
        else:
            extra = {"plain": {}, "overlapped": dict(overlap=True), "inline": dict(overlap=True, helper_thread=False)}[form]
            r = make(ugrt, s, **extra)[1]
        try:
            for _ in range(2):
                r.display(setup, **kw)
            r.synchronize()
            torch.cuda.synchronize()
            outs[form] = {n: _bytes(getattr(r, n), torch).cpu().numpy() for n in FORM_ARRAYS}
            outs[form].update({n: _bytes(getattr(r, n)[:3], torch).cpu().numpy() for n in FORM_LEVELS})
            if form == "plain":
                np.testing.assert_array_equal(r.image.cpu().numpy(), want["image_occluded"])
                assert_levels(r, want, 3)
        finally:
            if hasattr(r, "close"):
                r.close()
    for form in ("overlapped", "inline", "banded"):
        for n in FORM_ARRAYS + FORM_LEVELS:
            np.testing.assert_array_equal(outs[form][n], outs["plain"][n], err_msg="%s: %s" % (form, n))


@pytest.mark.gpu
def test_without_refract_the_frame_is_the_reflect_frame(ugrt, O, RF, REFS, torch):
    """refract=False on a renderer that knows transmit and ior: the CPU reflect composition, which treats transmit as
    absent -- on a fresh renderer and behind a refract frame."""
    s = scene(ugrt, "glass")
    setup = setup_for(ugrt, s)
    want = RS.cpu_frame(O, REFS, ugrt, "glass", W, H, 4)
    ctx, r = make(ugrt, s)
    kw = dict(shadows=True, reflect=True, bounces=4, reflect_shadows=True)
    r.display(setup, **kw)
    ctx.synchronize()
    RS.assert_occluded_frame(r, want, 4)
    r.display(setup, refract=True, **kw)
    r.display(setup, refract=False, **kw)
    ctx.synchronize()
    RS.assert_occluded_frame(r, want, 4)
    assert int((want["image_occluded"] != cpu_frame(O, RF, REFS, ugrt, "glass", 4)["image_occluded"]).sum()) > 3000


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, RF, REFS, torch):
    s = scene(ugrt, "glass")
    setup = setup_for(ugrt, s)
    want = cpu_frame(O, RF, REFS, ugrt, "glass", 2)
    ctx, r = make(ugrt, s)
    kw = dict(shadows=True, reflect=True, refract=True, bounces=2, reflect_shadows=True)
    r.display(setup, **kw)
    ctx.synchronize()
    uvalue, uspan, uoffset, _ = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
    occ = torch.zeros((3, N), dtype=torch.int32, device=ctx.device)
    eye = [tuple(float(x) for x in want["light"])]
    calls = {
        "refract_rays": [r.cam_pos, r.t, r.dir, r.intersect_id, r.d_matidx, r.d_reflect, r.d_transmit, r.d_ior, r.num_materials,
                         r.d_verts, r.d_faces, EPS, r.rays_levels[1], r.active_levels[1]],
        "refract_rays_next": [r.rays, r.active, r.hit_t, r.hit_id, r.d_matidx, r.d_reflect, r.d_transmit, r.d_ior,
                              r.num_materials, r.d_verts, r.d_faces, EPS, r.rays_levels[1], r.active_levels[1]],
        "trace_dda_any_thru": [uvalue, uspan, uoffset, r.d_verts, r.d_faces, r.occlusion_rays, r.occlusion_active, 1.0, occ[0],
                               r.d_matidx, r.d_transmit, r.num_materials],
        "trace_dda_any_lights_thru": [uvalue, uspan, uoffset, r.d_verts, r.d_faces, r.occlusion_rays, r.occlusion_active, eye,
                                      occ, r.d_matidx, r.d_transmit, r.num_materials],
    }
    before = {n: getattr(r, n).clone() for n in FORM_LEVELS}
    tried = 0
    values = {"refract_rays": (8, 11), "refract_rays_next": (8, 11), "trace_dda_any_thru": (7, 11),
              "trace_dda_any_lights_thru": (11,)}  # num_materials, eps, t_max: not pointers
    for name, args in calls.items():
        for k, a in enumerate(args):
            if k in values[name]:
                continue
            bad = list(args)
            bad[k] = None
            with pytest.raises(ugrt.UgrtError) as e:
                getattr(ctx, name)(*bad)
            assert e.value.code == ugrt.UGRT_EINVAL and "null" in str(e.value), (name, k)
            tried += 1
    for name, bad_t in (("trace_dda_any_thru", 0.0), ("trace_dda_any_thru", float("nan"))):
        bad = list(calls[name])
        bad[7] = bad_t
        with pytest.raises(ugrt.UgrtError) as e:
            getattr(ctx, name)(*bad)
        assert e.value.code == ugrt.UGRT_EINVAL
    for n_l in ([], [eye[0]] * 9):
        bad = list(calls["trace_dda_any_lights_thru"])
        bad[7] = n_l
        with pytest.raises(ugrt.UgrtError) as e:
            ctx.trace_dda_any_lights_thru(*bad)
        assert e.value.code == ugrt.UGRT_EINVAL
    assert tried == 12 + 12 + 10 + 11
    ctx.synchronize()
    for n, b in before.items():
        assert torch.equal(getattr(r, n), b), n
    assert not bool(occ.any())
    r.display(setup, **kw)
    ctx.synchronize()
    assert_levels(r, want, 2)
    np.testing.assert_array_equal(r.image.cpu().numpy(), want["image_occluded"])
