"""Shadows on reflected hits: ugrt_occlusion_rays, ugrt_trace_dda_any,
ugrt_shade_reflect_depth_occluded and Renderer / BandedRenderer.display(..., reflect_shadows=True).

The checker is tests/occlusion_ref.c (built here with the oracle's flags): the occlusion rays, the any-hit walk over
ALL cells of the specified set (no early exit), the test against every triangle and the occluded depth-D shading,
restated on the CPU.  The reflection levels themselves come from the CPU frame of tests/test_reflect_depth.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_reflect_depth as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
GCC = ["gcc", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-I", os.path.join(ROOT, "include"),
       "-shared"]

_p, _f32, _i32, bits, scene, setup_for, SIZES, LG, UD = (RD._p, RD._f32, RD._i32, RD.bits, RD.scene, RD.setup_for,
                                                         RD.SIZES, RD.LG, RD.UD)
CALLS = ("ugrt_occlusion_rays", "ugrt_trace_dda_any", "ugrt_shade_reflect_depth_occluded")


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class OcclusionRef:
    def __init__(self, lib):
        self.lib = lib

    def occlusion_rays(self, rays, active, hit_t, hit_id, verts, faces, light, eps, p0, n, N):
        orays, oactive = np.zeros(6 * N, np.float32), np.zeros(N, np.int32)
        self.lib.oc_occlusion_rays(_p(_f32(rays)), _p(_i32(active)), _p(_f32(hit_t)), _p(_i32(hit_id)),
                                   _p(_f32(verts).reshape(-1)), _p(_i32(faces).reshape(-1)), _p(_f32(light)),
                                   C.c_float(eps), C.c_int(p0), C.c_int(n), _p(orays), _p(oactive))
        return orays, oactive

    def trace_any(self, ugrid, verts, faces, rays, active, t_max, p0, n, N, fill=0):
        occ = np.full(N, fill, np.int32)
        cnt = np.zeros(3, np.uint64)
        self.lib.oc_trace_any(_p(_f32(ugrid["ug"])), _p(_i32(ugrid["dims"])), _p(_u32(ugrid["vals"])),
                              _p(_u32(ugrid["span"])), _p(_u32(ugrid["offset"])), _p(_f32(verts).reshape(-1)),
                              _p(_i32(faces).reshape(-1)), _p(_f32(rays)), _p(_i32(active)), C.c_float(t_max),
                              C.c_int(p0), C.c_int(n), _p(occ), _p(cnt))
        return occ

    def brute_any(self, verts, faces, rays, active, t_max, p0, n, N, fill=0):
        occ = np.full(N, fill, np.int32)
        faces = _i32(faces).reshape(-1)
        self.lib.oc_brute_any(_p(_f32(verts).reshape(-1)), _p(faces), C.c_int(len(faces) // 3), _p(_f32(rays)),
                              _p(_i32(active)), C.c_float(t_max), C.c_int(p0), C.c_int(n), _p(occ))
        return occ

    def shade_depth_occluded(self, cc, light, normal, t, dirs, ids, cam_pos, mat_idx, mat_list, reflect, verts, faces,
                             depth, rays, active, hit_t, hit_id, occluded, p0, n, N):
        img = np.zeros(3 * N, np.uint8)
        ids = _i32(ids).copy()
        mat_list = _f32(mat_list).reshape(-1)
        rays, hit_t, active, hit_id, occluded = _f32(rays), _f32(hit_t), _i32(active), _i32(hit_id), _i32(occluded)
        self.lib.oc_shade_depth_occluded(_p(_f32(cc)), _p(_f32(light)), _p(img), _p(_f32(normal)), _p(_f32(t)),
                                         _p(_f32(dirs)), _p(ids), _p(_f32(cam_pos)), _p(_i32(mat_idx)), _p(mat_list),
                                         _p(_f32(reflect)), C.c_int(len(mat_list) // 6), _p(_f32(verts).reshape(-1)),
                                         _p(_i32(faces).reshape(-1)), C.c_int(depth), C.c_longlong(N), _p(rays),
                                         _p(active), _p(hit_t), _p(hit_id), _p(occluded), C.c_int(p0), C.c_int(n))
        return img, ids


@pytest.fixture(scope="session")
def REFS(tmp_path_factory):
    """(the depth-D restatement of tests/reflect_depth_ref.c, the occlusion restatement of tests/occlusion_ref.c)"""
    d = tmp_path_factory.mktemp("reflect_shadows_ref")
    libs = []
    for name in ("reflect_depth_ref", "occlusion_ref"):
        out = str(d / ("lib%s.so" % name))
        subprocess.run(GCC + ["-o", out, os.path.join(HERE, name + ".c"), "-lm"], check=True, capture_output=True)
        libs.append(C.CDLL(out))
    return RD.DepthRef(libs[0]), OcclusionRef(libs[1])


_FRAMES = {}


def cpu_frame(O, REFS, ugrt, name, W, H, depth, rows=None):
    """The CPU frame of test_reflect_depth.cpu_frame plus, per level, the occlusion rays towards the light camera's
    eye and their any-hit flags, and the occluded image ("image_occluded", "mat_ids_occluded").  Computed once per
    (scene, size, depth, rows) and shared: nobody writes to it."""
    key = (name, W, H, depth, rows)
    if key in _FRAMES:
        return _FRAMES[key]
    REF, OC = REFS
    s = scene(ugrt, name)
    setup = setup_for(ugrt, s)
    want = RD.cpu_frame(O, REF, s, setup, W, H, depth, rows=rows, lg=LG, ud=UD)
    p0, n, N = want["p0"], want["n"], W * H
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    light = want["lcam"].worldori[:3].copy()
    for lv in want["levels"]:
        lv["orays"], lv["oactive"] = OC.occlusion_rays(lv["rays"], lv["active"], lv["hit_t"], lv["hit_id"], verts, faces,
                                                       light, 1e-3, p0, n, N)
        lv["occluded"] = OC.trace_any(want["ugrid"], verts, faces, lv["orays"], lv["oactive"], 1.0, p0, n, N)
    pr = want["primary"]
    stack = {k: np.concatenate([lv[k] for lv in want["levels"]]) for k in ("rays", "active", "hit_t", "hit_id", "occluded")}
    img, ids = OC.shade_depth_occluded(want["lcam"].cc, setup.shading_light, pr["normal"], pr["t"], pr["dir"], pr["id"],
                                       want["cam"].worldori[:3], s["matidx"], s["mat_list"], s["reflect"], verts, faces,
                                       depth, stack["rays"], stack["active"], stack["hit_t"], stack["hit_id"],
                                       stack["occluded"], p0, n, N)
    O.add_shadows(img, want["is_shadowed"], p0, n)
    want.update(image_occluded=img, mat_ids_occluded=ids, light=light, stack=stack)
    _FRAMES[key] = want
    return want


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_and_prototypes_name_the_occlusion_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    for name in ("occlusion_rays", "trace_dda_any", "shade_reflect_depth_occluded"):
        assert hasattr(ugrt.Context, name), name


@pytest.mark.parametrize("name", ["hall", "crash", "mirrors"])
def test_cpu_walk_finds_what_every_triangle_finds(ugrt, O, REFS, name):
    """oc_trace_any == oc_brute_any on the occlusion rays of levels 1..3, exactly; and neither outcome is rare: at
    level 1 at least 1000 occluded and 1000 lit rays."""
    W, H = SIZES[name]
    want = cpu_frame(O, REFS, ugrt, name, W, H, 3)
    s = scene(ugrt, name)
    N = W * H
    for j, lv in enumerate(want["levels"]):
        brute = REFS[1].brute_any(s["verts"], s["faces"], lv["orays"], lv["oactive"], 1.0, 0, N, N)
        diff = int((brute != lv["occluded"]).sum())
        print("%s level %d: %d occlusion rays, %d occluded, %d differ from brute force"
              % (name, j + 1, int(lv["oactive"].sum()), int(lv["occluded"].sum()), diff))
        assert diff == 0, (name, j + 1, diff)
        assert set(np.unique(lv["occluded"])) <= {0, 1}
        assert not lv["occluded"][lv["oactive"] == 0].any()
        np.testing.assert_array_equal(lv["oactive"], ((lv["active"] != 0) & (lv["hit_t"] > 0) & (lv["hit_id"] >= 0)))
    l1 = want["levels"][0]
    occ, lit = int(l1["occluded"].sum()), int((l1["oactive"] == 1).sum() - l1["occluded"].sum())
    assert occ >= 1000 and lit >= 1000, (occ, lit)


@pytest.mark.parametrize("name", ["hall", "mirrors"])
def test_cpu_occlusion_changes_the_image(ugrt, O, REFS, name):
    W, H = SIZES[name]
    want = cpu_frame(O, REFS, ugrt, name, W, H, 3)
    changed = (want["image_occluded"] != want["image_depth"]).reshape(-1, 3).any(1)
    assert int(changed.sum()) >= 1000
    np.testing.assert_array_equal(want["mat_ids_occluded"], want["mat_ids_depth"])
    # only pixels that see an occluded level can change, and they only get darker
    seen = np.zeros(W * H, bool)
    for lv in want["levels"]:
        seen |= lv["occluded"] == 1
    assert not (changed & ~seen).any()
    assert (want["image_occluded"] <= want["image_depth"]).all()


@pytest.mark.parametrize("depth", [1, 3])
def test_cpu_nothing_occluded_is_the_depth_shading(ugrt, O, REFS, depth):
    """With d_occluded all zero, oc_shade_depth_occluded gives rd_shade_depth's bytes."""
    REF, OC = REFS
    W, H = SIZES["hall"]
    want = cpu_frame(O, REFS, ugrt, "hall", W, H, depth)
    s = scene(ugrt, "hall")
    pr, st, N = want["primary"], want["stack"], W * H
    args = (want["lcam"].cc, setup_for(ugrt, s).shading_light, pr["normal"], pr["t"], pr["dir"], pr["id"],
            want["cam"].worldori[:3], s["matidx"], s["mat_list"], s["reflect"], s["verts"], s["faces"], depth,
            st["rays"], st["active"], st["hit_t"], st["hit_id"])
    img_a, ids_a = REF.shade_depth(*args, 0, N, N)
    img_b, ids_b = OC.shade_depth_occluded(*args, np.zeros_like(st["occluded"]), 0, N, N)
    np.testing.assert_array_equal(img_a, img_b)
    np.testing.assert_array_equal(ids_a, ids_b)
    assert int((img_a != 0).sum()) > 10000


def test_reflect_shadows_is_checked_before_anything_runs(ugrt):
    from importlib import import_module

    rmod = import_module(ugrt.__name__ + ".renderer")
    with pytest.raises(ValueError):
        rmod.check_reflect_shadows(True, False)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError):
            rmod.check_reflect_shadows(bad, True)
    assert rmod.check_reflect_shadows(True, True) is True
    assert rmod.check_reflect_shadows(np.bool_(True), True) is True
    assert rmod.check_reflect_shadows(False, False) is False and rmod.check_reflect_shadows(False, True) is False


class _Recorder:
    """A context that records the calls a stage enqueues."""

    def __init__(self):
        self.calls = []

    def grid_ptrs(self, which):
        return "value", "span", "offset", None

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name,) + a)


def _fake_frame(depth):
    import types

    f = types.SimpleNamespace(d_matidx="mi", d_reflect="refl", num_materials=3, d_verts="v", d_faces="f", reflect_eps=1e-3,
                              occlusion_rays="orays", occlusion_active="oact", image="img", normal="n", t="t", dir="d",
                              intersect_id="ids", d_matlist="ml", is_shadowed="sh")
    for n in ("rays", "active", "hit_t", "hit_id", "occluded"):
        setattr(f, n + "_levels", ["%s%d" % (n, j + 1) for j in range(depth)])
    f.rays, f.active, f.hit_t, f.hit_id = f.rays_levels[0], f.active_levels[0], f.hit_t_levels[0], f.hit_id_levels[0]
    return f


def test_stages_enqueue_the_occlusion_calls_behind_each_level_and_nothing_with_the_option_off(ugrt):
    from importlib import import_module

    rmod = import_module(ugrt.__name__ + ".renderer")
    f = _fake_frame(3)
    off, on = _Recorder(), _Recorder()
    rmod.trace_reflections(off, f, 3)
    assert [c[0] for c in off.calls] == ["trace_dda", "reflect_rays_next", "trace_dda", "reflect_rays_next", "trace_dda"]
    rmod.trace_reflections(on, f, 3, shadow_light=(1.0, 2.0, 3.0))
    assert [c for c in on.calls if c[0] not in ("occlusion_rays", "trace_dda_any")] == off.calls
    names = [c[0] for c in on.calls]
    assert names == ["trace_dda", "occlusion_rays", "trace_dda_any", "reflect_rays_next"] * 2 + ["trace_dda", "occlusion_rays", "trace_dda_any"]
    for j in range(3):
        dda, rays, any_ = [c for c in on.calls if c[0] in ("trace_dda", "occlusion_rays", "trace_dda_any")][3 * j:3 * j + 3]
        lv = tuple("%s%d" % (n, j + 1) for n in ("rays", "active", "hit_t", "hit_id"))
        assert dda[6:] == lv
        assert rays[1:] == lv + ("v", "f", (1.0, 2.0, 3.0), 1e-3, "orays", "oact")
        assert any_[1:] == ("value", "span", "offset", "v", "f", "orays", "oact", 1.0, "occluded%d" % (j + 1))
    for depth, want in ((1, "shade_reflect"), (3, "shade_reflect_depth")):
        f, off, on = _fake_frame(depth), _Recorder(), _Recorder()
        rmod.shade_frame(off, f, "cam", 1, True, True, depth)
        rmod.shade_frame(on, f, "cam", 1, True, True, depth, True)
        assert [c[0] for c in off.calls] == [want, "shade_add_shadows"]
        assert [c[0] for c in on.calls] == ["shade_reflect_depth_occluded", "shade_add_shadows"]
        assert on.calls[0][13:] == (depth, f.rays_levels, f.active_levels, f.hit_t_levels, f.hit_id_levels, f.occluded_levels)


# ------------------------------------------------------------------------------------------- the synthetic any-hit scene

SYN_DIMS = (8, 8, 4)
SYN_CELLS = {1: (1, 1), 7: (3, 1), 8: (5, 1), 9: (1, 3), 63: (3, 3), 64: (5, 3), 65: (1, 5), 129: (3, 5)}  # length: (i, j); k = 1
LATTICE = 12


def _lattice_centre(i, j, m):
    return i + 0.1 + 0.07 * (m % LATTICE), j + 0.1 + 0.07 * (m // LATTICE)


def synthetic_scene():
    """Triangles over [0, 8] x [0, 8] x [0, 4] (grid 8 x 8 x 4, cells of ~1): per list length n a cell of the layer
    k = 1 that holds n small horizontal triangles at z = 1.5 on a lattice (triangle m of the cell is the m-th entry of
    its list: lists are in ascending triangle id), two anchors in the corner cells that pin the box, and six wide
    slanted triangles in z 2.5..3.8 that random rays hit and whose hits lie in other cells than most of their lists."""
    tris, first = [], {}
    tris.append([(0, 0, 0), (0.01, 0, 0), (0, 0.01, 0)])
    for n, (i, j) in SYN_CELLS.items():
        first[n] = len(tris)
        for m in range(n):
            cx, cy = _lattice_centre(i, j, m)
            tris.append([(cx - 0.02, cy - 0.02, 1.5), (cx + 0.02, cy - 0.02, 1.5), (cx, cy + 0.02, 1.5)])
    rng = np.random.RandomState(1234)
    for _ in range(6):
        c = rng.uniform([1.5, 1.5, 2.9], [6.5, 6.5, 3.4])
        a, b = rng.uniform(-1.4, 1.4, 3), rng.uniform(-1.4, 1.4, 3)
        a[2], b[2] = 0.3 * a[2], 0.3 * b[2]
        tris.append([c, c + a, c + b])
    tris.append([(8, 8, 4), (7.99, 8, 4), (8, 7.99, 4)])
    verts = np.asarray(tris, np.float32).reshape(-1, 3)
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    return verts, faces, first


def synthetic_rays(ug, verts, N=4096):
    """[6N] rays and, for the hand-made ones, what they must give at t_max = 1: {pixel: 0 / 1}.  The others are
    random: segments from around the box to a point inside it, and (pixels 2000..3499) rays aimed at a point of a
    random triangle that lies at t = 2/3, which are occluded by construction."""
    rng = np.random.RandomState(99)
    o = rng.uniform([-1, -1, -1], [9, 9, 5], (N, 3))
    target = rng.uniform([0, 0, 0], [8, 8, 4], (N, 3))
    rays = np.concatenate([o, target - o], 1).astype(np.float32)
    tri = verts.reshape(-1, 3, 3)[rng.randint(0, len(verts) // 3, 1500)].astype(np.float64)
    w = rng.dirichlet([2, 2, 2], 1500)
    rays[2000:3500, 3:] = ((w[:, :, None] * tri).sum(1) - o[2000:3500]) * 1.5
    # one and two zero direction components, through the wide triangles' layer and the lattice cells
    rays[1000:1200, 4] = 0.0
    rays[1200:1400, 3] = 0.0
    rays[1400:1500, 3:5] = 0.0
    rays[1500:1600, 4:6] = 0.0
    expect, q = {}, 0

    def put(origin, direction, want=None):
        nonlocal q
        rays[q] = list(origin) + list(direction)
        if want is not None:
            expect[q] = want
        q += 1
        return q - 1

    named = {}
    for n, (i, j) in SYN_CELLS.items():
        for m in sorted({0, n // 2, n - 1}):  # the only occluder first, in the middle, last in the list
            cx, cy = _lattice_centre(i, j, m)
            put((cx, cy - 0.005, 0.2), (0, 0, 2.0), 1)  # straight up: reaches z = 2.2 at t = 1
        cx, cy = _lattice_centre(i, j, 0)
        put((cx + 0.035, cy, 0.2), (0, 0, 2.0), 0)      # between two triangles of the lattice
        put((cx, cy - 0.005, 0.2), (0, 0, 1.2), 0)      # stops at z = 1.4 below the triangle
        put((cx, cy - 0.005, -3.0), (0, 0, 6.0), 1)     # starts outside the box, enters at t = 0.5
        put((cx - 0.3, cy - 0.005, 0.9), (0.5, 0, 1.0), 1)  # slanted, one zero component
    cx, cy = _lattice_centre(*SYN_CELLS[65], 64)
    named["exact"] = put((cx, cy - 0.005, 0.25), (0, 0, 1.7))  # its only occluder near t = 0.735: t_max is set from it
    # rays that miss the box: pointing away, beside it with a zero component, parallel outside a slab
    put((-5, -5, -5), (-1, -0.5, -0.2), 0)
    put((4, 4, 9), (0, 0, 3), 0)
    put((4, -2, 1.5), (1, 0, 0), 0)
    put((9.5, 4, 1.5), (0, 1, 0), 0)
    put((20, 20, 20), (1, 1, 1), 0)
    # along a cell boundary: x on the plane between the cells 2 and 3 as the grid computes it
    xb = np.float32(ug[0]) + np.float32(3) * np.float32(ug[3])
    named["boundary"] = put((xb, 0.5, 1.5), (0, 7, 0))
    put((xb, 0.5, 0.2), (0, 6.5, 3.0))
    yb = np.float32(ug[1]) + np.float32(5) * np.float32(ug[4])
    put((0.2, yb, 3.1), (7.5, 0, 0))
    assert q < 200
    return rays.reshape(-1), expect, named


@pytest.fixture(scope="module")
def SYN(O):
    verts, faces, first = synthetic_scene()
    grid = O.grid_uniform(faces, verts, verts.min(0), verts.max(0), SYN_DIMS)
    rays, expect, named = synthetic_rays(grid["ug"], verts)
    return dict(verts=verts, faces=faces, first=first, grid=grid, rays=rays, expect=expect, named=named)


def syn_actives(N=4096):
    a67 = np.zeros(N, np.int32)
    a67[np.random.RandomState(5).choice(N, 67, replace=False)] = 1
    return {"none": np.zeros(N, np.int32), "all": np.ones(N, np.int32), "67": a67}


def test_synthetic_scene_has_the_list_lengths_and_the_references_agree(O, REFS, SYN):
    """CPU: the hand-built cells hold exactly the lengths asked for, the hand-made rays give what they were made for,
    and the walk equals brute force on every ray at both t_max."""
    OC, g, N = REFS[1], SYN["grid"], 4096
    dims = SYN_DIMS
    for n, (i, j) in SYN_CELLS.items():
        cell = (i * dims[1] + j) * dims[2] + 1
        assert int(g["span"][cell]) == n, (n, int(g["span"][cell]))
        off = int(g["offset"][cell])
        np.testing.assert_array_equal(g["vals"][off:off + n], np.arange(SYN["first"][n], SYN["first"][n] + n))
    assert 0 in set(g["span"].tolist())
    act = np.ones(N, np.int32)
    for t_max in (1.0, 3e38):
        walk = OC.trace_any(g, SYN["verts"], SYN["faces"], SYN["rays"], act, t_max, 0, N, N)
        brute = OC.brute_any(SYN["verts"], SYN["faces"], SYN["rays"], act, t_max, 0, N, N)
        np.testing.assert_array_equal(walk, brute)
        assert 1000 < int(walk.sum()) < N - 1000, int(walk.sum())  # (1500 rays are aimed at a triangle, ~2400 at random)
        if t_max == 1.0:
            for p, w in SYN["expect"].items():
                assert walk[p] == w, (p, w)
    ht, hid = O.brute_nearest(SYN["verts"], SYN["faces"], SYN["rays"], act, 0, N, N)
    p = SYN["named"]["exact"]
    t = np.float32(ht[p])
    assert hid[p] == SYN["first"][65] + 64 and 0.5 < t < 1.0
    one = np.zeros(N, np.int32)
    one[p] = 1
    assert OC.trace_any(g, SYN["verts"], SYN["faces"], SYN["rays"], one, t, 0, N, N)[p] == 0
    assert OC.trace_any(g, SYN["verts"], SYN["faces"], SYN["rays"], one, np.nextafter(t, np.float32(2)), 0, N, N)[p] == 1


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def make(ugrt, s, W, H, **kw):
    return RD.make(ugrt, s, W, H, **kw)


def assert_occluded_frame(r, want, depth):
    """The reflection levels (unchanged by the option), the levels' occlusion flags, image and material ids."""
    a, b = want["p0"], want["p0"] + want["n"]
    for j, w in enumerate(want["levels"][:depth]):
        what = "level %d" % (j + 1)
        np.testing.assert_array_equal(r.active_levels[j].cpu().numpy()[a:b], w["active"][a:b], err_msg=what)
        np.testing.assert_array_equal(bits(r.rays_levels[j].cpu().numpy()[6 * a:6 * b]), bits(w["rays"][6 * a:6 * b]), err_msg=what)
        np.testing.assert_array_equal(r.hit_id_levels[j].cpu().numpy()[a:b], w["hit_id"][a:b], err_msg=what)
        np.testing.assert_array_equal(bits(r.hit_t_levels[j].cpu().numpy()[a:b]), bits(w["hit_t"][a:b]), err_msg=what)
        np.testing.assert_array_equal(r.occluded_levels[j].cpu().numpy()[a:b], w["occluded"][a:b], err_msg=what)
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy()[a:b], want["mat_ids_occluded"][a:b])
    np.testing.assert_array_equal(r.image.cpu().numpy()[3 * a:3 * b], want["image_occluded"][3 * a:3 * b])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 4])
@pytest.mark.parametrize("name", ["hall", "crash", "mirrors"])
def test_frame_equals_the_cpu_frame(ugrt, O, REFS, torch, name, depth):
    s = scene(ugrt, name)
    W, H = SIZES[name]
    ctx, r = make(ugrt, s, W, H)
    r.display(setup_for(ugrt, s), shadows=True, reflect=True, bounces=depth, reflect_shadows=True)
    ctx.synchronize()
    want = cpu_frame(O, REFS, ugrt, name, W, H, depth)
    assert_occluded_frame(r, want, depth)
    assert int(want["levels"][0]["occluded"].sum()) >= 1000
    assert int((want["image_occluded"] != want["image_depth"]).sum()) > 0


@pytest.mark.gpu
def test_occlusion_rays_equal_the_cpu_rays(ugrt, O, REFS, torch):
    """ugrt_occlusion_rays on levels 1 and 2 of mirrors: rays bit-equal, oactive equal, also for diffuse hits."""
    s = scene(ugrt, "mirrors")
    W, H = SIZES["mirrors"]
    N = W * H
    want = cpu_frame(O, REFS, ugrt, "mirrors", W, H, 2)
    ctx, r = make(ugrt, s, W, H)
    r.display(setup_for(ugrt, s), shadows=True, reflect=True, bounces=2)
    for j in range(2):
        orays, oactive = torch.full((6 * N,), 7.0, device=ctx.device), torch.full((N,), 7, dtype=torch.int32, device=ctx.device)
        ctx.occlusion_rays(r.rays_levels[j], r.active_levels[j], r.hit_t_levels[j], r.hit_id_levels[j], r.d_verts,
                           r.d_faces, want["light"], 1e-3, orays, oactive)
        ctx.synchronize()
        w = want["levels"][j]
        np.testing.assert_array_equal(oactive.cpu().numpy(), w["oactive"])
        np.testing.assert_array_equal(bits(orays.cpu().numpy()), bits(w["orays"]))
        assert int(w["oactive"].sum()) > 1000
    # hits on materials that do not reflect get a ray too (they do not go on to level 2)
    l1, l2 = want["levels"]
    assert int(((l1["oactive"] == 1) & (l2["active"] == 0)).sum()) > 100


def _syn_context(ugrt, SYN, rows=None):
    ctx = ugrt.Context(64, 64, light_grid=(16, 16), uniform_dims=SYN_DIMS, rows=rows)
    dv, df = ctx.upload(SYN["verts"].reshape(-1)), ctx.upload(SYN["faces"].reshape(-1))
    ctx.grid_build_uniform(df, dv, len(SYN["faces"]), SYN["verts"].min(0), SYN["verts"].max(0))
    value, key, span, offset, gi = ctx.grid_arrays(ugrt.GRID_UNIFORM)
    np.testing.assert_array_equal(span.cpu().numpy().view(np.uint32), SYN["grid"]["span"])
    return ctx, dv, df, ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3]


def _syn_trace(ctx, grid, dv, df, d_rays, active, t_max, torch, sentinel=-7):
    occ = torch.full((4096,), sentinel, dtype=torch.int32, device=ctx.device)
    ctx.trace_dda_any(grid[0], grid[1], grid[2], dv, df, d_rays, ctx.upload(active), float(t_max), occ)
    ctx.synchronize()
    return occ.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [None, (2, 5)])
def test_synthetic_any_hit(ugrt, O, REFS, SYN, torch, rows):
    """4096 rays over the hand-built scene against the walk over all cells and against every triangle: list lengths
    0, 1, 7, 8, 9, 63, 64, 65, 129 with the only occluder first / in the middle / last, t_max 1 and 3e38, the occluder
    at t == t_max and one float below it, rays from outside, misses, zero components, a ray along a cell boundary;
    none / all / 67 rays active; a band whose p0 is not 0 and whose other pixels keep the sentinel."""
    OC, N = REFS[1], 4096
    ctx, dv, df, grid = _syn_context(ugrt, SYN, rows)
    p0, n = ctx.p0, ctx.npix
    assert (p0, n) == ((0, N) if rows is None else (1024, 1536))
    d_rays = ctx.upload(SYN["rays"])
    args = (SYN["verts"], SYN["faces"], SYN["rays"])
    for which, active in syn_actives().items():
        for t_max in (1.0, 3e38):
            got = _syn_trace(ctx, grid, dv, df, d_rays, active, t_max, torch)
            walk = OC.trace_any(SYN["grid"], *args, active, t_max, p0, n, N, fill=-7)
            brute = OC.brute_any(*args, active, t_max, p0, n, N, fill=-7)
            np.testing.assert_array_equal(got, walk, err_msg="%s t_max %g" % (which, t_max))
            np.testing.assert_array_equal(got, brute, err_msg="%s t_max %g" % (which, t_max))
            assert (got[:p0] == -7).all() and (got[p0 + n:] == -7).all()
            if which == "all" and t_max == 1.0 and rows is None:
                for p, w in SYN["expect"].items():
                    assert got[p] == w, (p, w)
                assert 1000 < int(got.sum()) < N - 1000
    if rows is None:
        act = np.ones(N, np.int32)
        ht, _ = O.brute_nearest(*args, act, 0, N, N)
        p = SYN["named"]["exact"]
        t = np.float32(ht[p])
        assert _syn_trace(ctx, grid, dv, df, d_rays, act, t, torch)[p] == 0
        above = np.nextafter(t, np.float32(2))
        got = _syn_trace(ctx, grid, dv, df, d_rays, act, above, torch)
        assert got[p] == 1
        np.testing.assert_array_equal(got, OC.trace_any(SYN["grid"], *args, act, above, 0, N, N))
        # vertex and face arrays that are not the ones the grid was built from: the kernel gathers instead of
        # reading the context's triangle records
        got = _syn_trace(ctx, grid, dv.clone(), df.clone(), d_rays, act, 1.0, torch)
        np.testing.assert_array_equal(got, OC.trace_any(SYN["grid"], *args, act, 1.0, 0, N, N))


@pytest.mark.gpu
def test_synthetic_launch_shapes(ugrt, O, REFS, SYN, torch):
    """Every any_rays_per_wave, and any_coop around every list length of the scene and at the ends of its range: the
    same flags."""
    OC, N = REFS[1], 4096
    ctx, dv, df, grid = _syn_context(ugrt, SYN)
    d_rays = ctx.upload(SYN["rays"])
    act = syn_actives()["all"]
    want = {t: OC.trace_any(SYN["grid"], SYN["verts"], SYN["faces"], SYN["rays"], act, t, 0, N, N) for t in (1.0, 3e38)}
    d_act = ctx.upload(act)
    d_want = {t: ctx.upload(w) for t, w in want.items()}
    shapes = [("any_rays_per_wave", v) for v in range(0, 65)]
    shapes += [("any_coop", v) for v in (1, 2, 7, 8, 9, 10, 63, 64, 65, 66, 129, 130, 1 << 30)]
    for key, v in shapes:
        ctx.set_option(key, v)
        for t in (1.0, 3e38):
            occ = torch.full((N,), -7, dtype=torch.int32, device=ctx.device)
            ctx.trace_dda_any(grid[0], grid[1], grid[2], dv, df, d_rays, d_act, t, occ)
            assert torch.equal(occ, d_want[t]), (key, v, t)
        ctx.set_option(key, -1)
    for key, bad in (("any_rays_per_wave", 65), ("any_coop", 0)):
        with pytest.raises(ugrt.UgrtError):
            ctx.set_option(key, bad)


PROF_STAGES = ("worklist", "trace_dda", "reflect_gen")


def _secondary_calls(ctx, torch, SYN, dv, df, grid, sentinel=-7):
    """One call of each of the nine any-hit exports and of each of the six ray generators on the synthetic scene, as
    (name, function) pairs; every call writes into buffers of its own.  3 lights, 4 hemisphere directions, 5 samples and
    a 2 x 2 tile of sample sets: more than one layer to clear, and a sample table in LDS.  Returns the pairs and the
    lights call's flags [3, N]."""
    N, nf = 4096, len(SYN["faces"])
    i32, f32 = torch.int32, torch.float32
    rng = np.random.RandomState(11)
    rays, act = ctx.upload(SYN["rays"]), ctx.upload(np.ones(N, np.int32))
    mat_idx = torch.zeros(nf, dtype=i32, device=ctx.device)
    reflect, transmit, ior = (ctx.upload(np.asarray([v], np.float32)) for v in (0.5, 0.5, 1.5))
    lights = [(4.0, 4.0, 3.9), (1.5, 6.5, 3.9), (6.5, 1.5, 3.95)]  # above the wide triangles: they shadow what lies below
    dirs = [(0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, 0.6, 0.8), (-0.6, 0.0, 0.8)]
    samples = rng.uniform([1, 1, 3.5], [7, 7, 3.9], (5, 3)).astype(np.float32)
    sets = ctx.upload(rng.uniform([1, 1, 3.5], [7, 7, 3.9], (4, 5, 3)).astype(np.float32).reshape(-1))
    flags = lambda n=N: torch.full((n,), sentinel, dtype=i32, device=ctx.device)
    occ_lights = flags(3 * N)
    g, thru = (grid[0], grid[1], grid[2], dv, df, rays, act), (mat_idx, transmit, 1)
    any_hit = [
        ("trace_dda_any", lambda o=flags(): ctx.trace_dda_any(*g, 1.0, o)),
        ("trace_dda_any_thru", lambda o=flags(): ctx.trace_dda_any_thru(*g, 1.0, o, *thru)),
        ("trace_dda_any_lights", lambda: ctx.trace_dda_any_lights(*g, lights, occ_lights)),
        ("trace_dda_any_lights_thru", lambda o=flags(3 * N): ctx.trace_dda_any_lights_thru(*g, lights, o, *thru)),
        ("trace_dda_any_hemi", lambda o=flags(): ctx.trace_dda_any_hemi(*g, dirs, 2.0, o)),
        ("trace_dda_any_area", lambda o=flags(): ctx.trace_dda_any_area(*g, samples, o)),
        ("trace_dda_any_area_thru", lambda o=flags(): ctx.trace_dda_any_area_thru(*g, samples, o, *thru)),
        ("trace_dda_any_area_sets", lambda o=flags(): ctx.trace_dda_any_area_sets(*g, 5, 2, 2, sets, o)),
        ("trace_dda_any_area_sets_thru", lambda o=flags(): ctx.trace_dda_any_area_sets_thru(*g, 5, 2, 2, sets, o, *thru)),
    ]
    # the generators' inputs: hits of random triangles (or none) at t = 1/2 along the synthetic rays, seen from a camera
    cam = ctx.upload(np.asarray([4.0, 4.0, -2.0], np.float32))
    ids = ctx.upload(rng.randint(-1, nf, N).astype(np.int32))
    t = torch.full((N,), 0.5, dtype=f32, device=ctx.device)
    pdir = ctx.upload(np.ascontiguousarray(SYN["rays"].reshape(N, 6)[:, 3:]).reshape(-1))
    out = lambda: (torch.empty(6 * N, dtype=f32, device=ctx.device), torch.empty(N, dtype=i32, device=ctx.device))
    generators = [
        ("reflect_rays", lambda o=out(): ctx.reflect_rays(cam, t, pdir, ids, mat_idx, reflect, 1, dv, df, 1e-3, *o)),
        ("reflect_rays_next", lambda o=out(): ctx.reflect_rays_next(rays, act, t, ids, mat_idx, reflect, 1, dv, df, 1e-3, *o)),
        ("refract_rays", lambda o=out(): ctx.refract_rays(cam, t, pdir, ids, mat_idx, reflect, transmit, ior, 1, dv, df, 1e-3, *o)),
        ("refract_rays_next", lambda o=out(): ctx.refract_rays_next(rays, act, t, ids, mat_idx, reflect, transmit, ior, 1, dv, df,
                                                                   1e-3, *o)),
        ("occlusion_rays", lambda o=out(): ctx.occlusion_rays(rays, act, t, ids, dv, df, lights[0], 1e-3, *o)),
        ("ao_rays", lambda o=out(): ctx.ao_rays(cam, t, pdir, ids, dv, df, 1e-3, *o)),
    ]
    return any_hit, generators, occ_lights


@pytest.mark.gpu
def test_secondary_calls_open_their_profiler_brackets_once(ugrt, SYN, torch):
    """The stage profiler's launch counts around the any-hit walk's host path and the generators' launcher: each of the
    nine any-hit exports adds one `worklist` and one `trace_dda` launch and no `reflect_gen`, each of the six generators
    one `reflect_gen` and nothing else, and with profiling off none of them adds anything.  The lights call of a band
    context (its layers are not contiguous: one clear per layer) gives the full frame's flags on its rows and leaves the
    other rows alone."""
    N = 4096
    ctx, dv, df, grid = _syn_context(ugrt, SYN)
    any_hit, generators, occ_lights = _secondary_calls(ctx, torch, SYN, dv, df, grid)
    counts = lambda: {k: v[1] for k, v in ctx.prof_get().items() if k in PROF_STAGES}
    ctx.prof_enable(True, stages=PROF_STAGES)
    ctx.prof_reset()
    assert counts() == dict.fromkeys(PROF_STAGES, 0)
    for calls, adds in ((any_hit, {"worklist": 1, "trace_dda": 1, "reflect_gen": 0}),
                        (generators, {"worklist": 0, "trace_dda": 0, "reflect_gen": 1})):
        for name, call in calls:
            before = counts()
            call()
            assert counts() == {k: before[k] + adds[k] for k in PROF_STAGES}, name
    assert counts() == {"worklist": 9, "trace_dda": 9, "reflect_gen": 6}
    ctx.prof_enable(False)
    before = ctx.prof_get()
    for name, call in any_hit + generators:
        call()
    assert ctx.prof_get() == before
    # the band: rows 2..4 of 8
    full = occ_lights.cpu().numpy().reshape(3, N)
    assert set(np.unique(full)) == {0, 1} and all(0 < int(full[l].sum()) < N for l in range(3))
    band, bv, bf, bgrid = _syn_context(ugrt, SYN, rows=(2, 5))
    p0, n = band.p0, band.npix
    assert (p0, n) == (1024, 1536)
    band.prof_enable(True, stages=PROF_STAGES)
    band_any, _, band_lights = _secondary_calls(band, torch, SYN, bv, bf, bgrid)
    dict(band_any)["trace_dda_any_lights"]()
    assert {k: v[1] for k, v in band.prof_get().items() if k in PROF_STAGES} == {"worklist": 1, "trace_dda": 1, "reflect_gen": 0}
    got = band_lights.cpu().numpy().reshape(3, N)
    np.testing.assert_array_equal(got[:, p0:p0 + n], full[:, p0:p0 + n])
    assert (got[:, :p0] == -7).all() and (got[:, p0 + n:] == -7).all()


@pytest.mark.gpu
def test_launch_options_do_not_change_the_frame(ugrt, O, REFS, torch):
    """The new options, and dda_kernel 0/1 x dda_split 0/1/4 for the levels around the occlusion launches: two frames
    each, the same flags, image and reflection levels (level 1's arrays included) as the CPU frame."""
    name, depth = "mirrors", 2
    s = scene(ugrt, name)
    W, H = SIZES[name]
    setup = setup_for(ugrt, s)
    want = cpu_frame(O, REFS, ugrt, name, W, H, depth)
    combos = [{"dda_kernel": k, "dda_split": sp} for k in (0, 1) for sp in (0, 1, 4)]
    combos += [{"dda_split": 1, "dda_split_load": 50}]
    combos += [{"any_rays_per_wave": v} for v in (1, 5, 16, 32, 64)] + [{"any_coop": v} for v in (1, 8, 64, 1 << 30)]
    for opts in combos:
        ctx, r = make(ugrt, s, W, H)
        for k, v in opts.items():
            ctx.set_option(k, v)
        for _ in range(2):
            r.display(setup, shadows=True, reflect=True, bounces=depth, reflect_shadows=True)
        ctx.synchronize()
        try:
            assert_occluded_frame(r, want, depth)
        except AssertionError as e:
            raise AssertionError("options %s: %s" % (opts, e))


@pytest.mark.gpu
def test_display_paths_agree(ugrt, O, REFS, torch):
    """mirrors 320x192, depth 2: the plain, the overlapped and the inline two-stream renderer and three bands."""
    name, (W, H), depth = "mirrors", (320, 192), 2
    s = scene(ugrt, name)
    setup = setup_for(ugrt, s)
    want = cpu_frame(O, REFS, ugrt, name, W, H, depth)
    for pname, r in RD._paths_renderers(ugrt, s, W, H).items():
        r.display(setup, shadows=True, reflect=True, bounces=depth, reflect_shadows=True)
        r.synchronize()
        torch.cuda.synchronize()
        assert_occluded_frame(r, want, depth)
        r.close()
    br = ugrt.BandedRenderer(ugrt.Context, W, H, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"],
                             bands=3, light_grid=LG, uniform_dims=UD, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS)
    for _ in range(2):
        br.display(setup, shadows=True, reflect=True, bounces=depth, reflect_shadows=True)
    br.synchronize()
    torch.cuda.synchronize()
    assert_occluded_frame(br, want, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("async_build", [1, 0])
def test_four_renderers_in_flight_equal_a_sequential_context(ugrt, torch, async_build):
    """As tests/test_reflect_depth.py's test of the same name, with the option on."""
    s = scene(ugrt, "crash")
    W, H = 384, 216
    setup = setup_for(ugrt, s)
    kw = dict(shadows=True, reflect=True, bounces=3, reflect_shadows=True)
    seq_ctx, seq = make(ugrt, s, W, H)
    seq.display(setup, **kw)
    seq_ctx.synchronize()
    renderers = []
    for i in range(4):
        stream = torch.cuda.Stream() if i else None
        with torch.cuda.stream(stream):
            cx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)
            rr = ugrt.Renderer(cx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], overlap=True,
                               helper_thread=False)
        for c in (rr.ctx, rr.aux):
            c.set_option("async_build", async_build)
        rr._stream = stream
        renderers.append(rr)
    for k in range(8):
        rr = renderers[k % 4]
        with torch.cuda.stream(rr._stream):
            rr.display(setup, **kw)
    for rr in renderers:
        rr.synchronize()
    torch.cuda.synchronize()
    for i, rr in enumerate(renderers):
        for n in ("image", "intersect_id", "is_shadowed", "rays_levels", "active_levels", "hit_t_levels",
                  "hit_id_levels", "occluded_levels"):
            a, b = getattr(rr, n), getattr(seq, n)
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (i, n)
    assert int(seq.occluded_levels[0].sum()) > 1000 and int(seq.occluded_levels[2].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_option_off_is_the_frame_as_it_was(ugrt, torch, depth):
    """A renderer that has rendered with the option and then without gives, byte for byte, the image and every level
    of a renderer that never heard of it."""
    s = scene(ugrt, "hall")
    W, H = SIZES["hall"]
    setup = setup_for(ugrt, s)
    ctx_a, a = make(ugrt, s, W, H)
    a.display(setup, shadows=True, reflect=True, bounces=depth)
    ctx_a.synchronize()
    assert a.occluded_levels is None and a.occlusion_rays is None
    ctx_b, b = make(ugrt, s, W, H)
    b.display(setup, shadows=True, reflect=True, bounces=depth, reflect_shadows=True)
    ctx_b.synchronize()
    assert not torch.equal(a.image, b.image)
    b.display(setup, shadows=True, reflect=True, bounces=depth, reflect_shadows=False)
    ctx_b.synchronize()
    for n in ("image", "intersect_id", "is_shadowed", "rays_levels", "active_levels", "hit_t_levels", "hit_id_levels"):
        x, y = getattr(a, n), getattr(b, n)
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), n


@pytest.mark.gpu
def test_bad_arguments_leave_the_context_usable(ugrt, O, REFS, torch):
    name = "hall"
    s = scene(ugrt, name)
    W, H = SIZES[name]
    N = W * H
    setup = setup_for(ugrt, s)
    fresh = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD)
    z = fresh.torch.zeros(6 * N, dtype=fresh.torch.int32, device=fresh.device)
    for call in (lambda: fresh.trace_dda(z, z, z, z, z, z, z, z, z), lambda: fresh.trace_dda_any(z, z, z, z, z, z, z, 1.0, z)):
        with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: the same error from both
            call()
        assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    ctx, r = make(ugrt, s, W, H)
    r.display(setup, shadows=True, reflect=True, bounces=2, reflect_shadows=True)
    ctx.synchronize()
    g = ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3]
    occ = r.occluded_levels[0]
    for t_max in (0.0, -1.0, float("nan")):
        with pytest.raises(ugrt.UgrtError) as e:
            ctx.trace_dda_any(g[0], g[1], g[2], r.d_verts, r.d_faces, r.occlusion_rays, r.occlusion_active, t_max, occ)
        assert e.value.code == ugrt.UGRT_EINVAL and b"t_max" in ugrt.lib.ugrt_last_error()
    any_args = [g[0], g[1], g[2], r.d_verts, r.d_faces, r.occlusion_rays, r.occlusion_active, 1.0, occ]
    ray_args = [r.rays, r.active, r.hit_t, r.hit_id, r.d_verts, r.d_faces, [0.0, 1.0, 2.0], 1e-3, r.occlusion_rays,
                r.occlusion_active]
    shade_args = [r.image, r.normal, r.t, r.dir, r.intersect_id, r.cam_pos, r.d_matidx, r.d_matlist, r.d_reflect,
                  r.num_materials, r.d_verts, r.d_faces, 2, r.rays_levels, r.active_levels, r.hit_t_levels,
                  r.hit_id_levels, r.occluded_levels]
    for fn, args, holes in ((ctx.trace_dda_any, any_args, (0, 5, 8)), (ctx.occlusion_rays, ray_args, (0, 3, 9)),
                            (ctx.shade_reflect_depth_occluded, shade_args, (0, 13, 17))):
        for h in holes:
            bad = list(args)
            bad[h] = None
            with pytest.raises(ugrt.UgrtError) as e:
                fn(*bad)
            assert e.value.code == ugrt.UGRT_EINVAL and b"null" in ugrt.lib.ugrt_last_error()
    for depth in (0, 9):
        with pytest.raises(ugrt.UgrtError) as e:
            ctx.shade_reflect_depth_occluded(*(shade_args[:12] + [depth] + shade_args[13:]))
        assert e.value.code == ugrt.UGRT_EINVAL and b"depth" in ugrt.lib.ugrt_last_error()
    br = ugrt.BandedRenderer(ugrt.Context, W, H, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"],
                             bands=2, light_grid=LG, uniform_dims=UD, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS)
    for rr in (r, br):
        with pytest.raises(ValueError):
            rr.display(setup, shadows=True, reflect=False, reflect_shadows=True)
        with pytest.raises(ValueError):
            rr.display(setup, shadows=True, reflect=True, reflect_shadows=1)
    r.display(setup, shadows=True, reflect=True, bounces=2, reflect_shadows=True)
    ctx.synchronize()
    assert_occluded_frame(r, cpu_frame(O, REFS, ugrt, name, W, H, 2), 2)
