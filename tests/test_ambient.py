"""Ambient occlusion: ugrt_ao_rays, ugrt_trace_dda_any_hemi, ugrt_shade_ao and
Renderer.display(..., ao=S, ao_radius=r).

The checker is tests/ambient_ref.c (built here with the oracle's flags): the rays, the explicit ray set of one
hemisphere direction (the basis written out) and the integer shading, restated on the CPU.  The any-hit walk has no
restatement of its own: the expected mask is oc_trace_any of tests/occlusion_ref.c on the explicit rays, once per
direction.  The frames underneath come from the CPU frames of tests/test_lights.py, tests/test_reflect_shadows.py and
tests/test_reflect_lights.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
from test_lights import LT  # noqa: F401  (fixtures)
from test_reflect_lights import RL  # noqa: F401
from test_reflect_shadows import REFS, SYN  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))

_p, _f32, _i32, bits, scene, SIZES, LG, UD = RD._p, RD._f32, RD._i32, RD.bits, RD.scene, RD.SIZES, RD.LG, RD.UD
CALLS = ("ugrt_ao_rays", "ugrt_trace_dda_any_hemi", "ugrt_shade_ao")
EPS = 1e-3
S_FRAME = 16  # hemisphere rays per pixel in the frame tests
DEPTH = 3     # of the reflecting frames


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class AmbientRef:
    def __init__(self, lib):
        self.lib = lib

    def rays(self, cam_pos, t, dirs, ids, verts, faces, eps, p0, n, N, fill=None):
        orays = np.zeros(6 * N, np.float32) if fill is None else np.full(6 * N, fill, np.float32)
        oactive = np.zeros(N, np.int32) if fill is None else np.full(N, int(fill), np.int32)
        self.lib.ao_rays(_p(_f32(cam_pos)), _p(_f32(t)), _p(_f32(dirs)), _p(_i32(ids)), _p(_f32(verts).reshape(-1)),
                         _p(_i32(faces).reshape(-1)), C.c_float(eps), C.c_int(p0), C.c_int(n), _p(orays), _p(oactive))
        return orays, oactive

    def basis(self, n):
        n, T, B = _f32(n), np.zeros(3, np.float32), np.zeros(3, np.float32)
        self.lib.ao_basis(_p(n), _p(T), _p(B))
        return T, B

    def expand(self, orays, oactive, direction, p0, n, N):
        """[6N] explicit rays {o, D_s} of one local direction."""
        rays = np.zeros(6 * N, np.float32)
        self.lib.ao_expand(_p(_f32(orays)), _p(_i32(oactive)), _p(_f32(direction)), C.c_int(p0), C.c_int(n), _p(rays))
        return rays

    def shade(self, img, mask, num_dirs, p0, n):
        img = np.ascontiguousarray(img, np.uint8).copy()
        self.lib.ao_shade(_p(img), _p(_u32(mask)), C.c_int(num_dirs), C.c_int(p0), C.c_int(n))
        return img


@pytest.fixture(scope="session")
def AO(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ambient_ref") / "libambient_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "ambient_ref.c"), "-lm"], check=True, capture_output=True)
    return AmbientRef(C.CDLL(out))


def cpu_mask(OC, AO, grid, verts, faces, orays, oactive, dirs, radius, p0, n, N, fill=0, keep=None):
    """The expected mask words: per direction s the explicit rays of ao_expand walked by oc_trace_any at
    t_max = radius, its flags OR-ed into bit s.  Pixels outside the band keep `fill`.  keep: a list that receives the
    explicit rays of every direction."""
    mask = np.full(N, fill, np.uint32)
    mask[p0:p0 + n] = 0
    for s, d in enumerate(np.asarray(dirs, np.float32).reshape(-1, 3)):
        rays = AO.expand(orays, oactive, d, p0, n, N)
        occ = OC.trace_any(grid, verts, faces, rays, oactive, radius, p0, n, N)
        assert set(np.unique(occ[p0:p0 + n])) <= {0, 1}
        mask[p0:p0 + n] |= occ[p0:p0 + n].astype(np.uint32) << np.uint32(s)
        if keep is not None:
            keep.append(rays)
    return mask


def mask_counts(mask, oactive, S):
    hit = oactive != 0
    return dict(nonzero=int((mask[hit] != 0).sum()), zero=int((mask[hit] == 0).sum()),
                per_bit=[int(((mask[hit] >> np.uint32(s)) & 1).sum()) for s in range(S)])


def feasible(c):
    """The feasibility conditions of section 6.5 on mask_counts' figures."""
    return c["nonzero"] >= 1000 and c["zero"] >= 1000 and min(c["per_bit"]) >= 100


_AMBIENT = {}


def cpu_ambient(O, REFS, AO, ugrt, name):
    """The CPU side of a frame's ambient occlusion at S_FRAME directions: {o', n} of the primary hits of
    test_reflect_shadows' frame, the radius, the explicit rays per direction and the mask.  The radius is picked on the
    CPU alone: 5 % of the scene's largest extent (1.4 on both fixtures), at which the feasibility conditions hold.
    Computed once per scene and shared: nobody writes to it."""
    if name in _AMBIENT:
        return _AMBIENT[name]
    W, H = SIZES[name]
    base = RS.cpu_frame(O, REFS, ugrt, name, W, H, DEPTH)
    s = scene(ugrt, name)
    pr, N = base["primary"], W * H
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    cam_pos = base["cam"].worldori[:3].copy()
    orays, oactive = AO.rays(cam_pos, pr["t"], pr["dir"], pr["id"], verts, faces, EPS, 0, N, N)
    dirs = ugrt.scenes.ao_directions(S_FRAME)
    v = verts.reshape(-1, 3)
    radius = float(np.float32(0.05 * float((v.max(0) - v.min(0)).max())))
    expanded = []
    mask = cpu_mask(REFS[1], AO, base["ugrid"], verts, faces, orays, oactive, dirs, radius, 0, N, N, keep=expanded)
    counts = mask_counts(mask, oactive, S_FRAME)
    out = dict(base=base, scene=s, orays=orays, oactive=oactive, dirs=dirs, radius=radius, mask=mask, counts=counts,
               expanded=expanded, cam_pos=cam_pos, N=N)
    _AMBIENT[name] = out
    return out


# the normals of the basis cases: the axes (+-z: a tie for the smallest, axis 0 wins), |n0| == |n1| above |n2|, an oblique one
_R2 = float(np.float32(1.0) / np.sqrt(np.float32(2.0)))
NORMALS = np.asarray([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (_R2, _R2, 0), (0, .6, .8)],
                     np.float32)


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    for name in ("ao_rays", "trace_dda_any_hemi", "shade_ao"):
        assert hasattr(ugrt.Context, name), name
    assert ugrt.MAX_AO_DIRS == 32
    d = ugrt.scenes.ao_directions(16)
    assert d.dtype == np.float32 and d.shape == (16, 3)
    np.testing.assert_allclose((d.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-6)
    assert (d[:, 2] > 0).all() and (np.diff(d[:, 2]) < 0).all()
    np.testing.assert_array_equal(bits(d), bits(ugrt.scenes.ao_directions(16)))


@pytest.mark.parametrize("name", ["hall", "crash"])
def test_cpu_masks_are_feasible_and_the_walk_finds_what_every_triangle_finds(ugrt, O, REFS, AO, name):
    """S = 16 on the fixtures of section 6.2: neither outcome is rare, every direction is occluded somewhere, and
    oc_trace_any == oc_brute_any on every explicit ray.  The counts are those of DESIGN.md section 6.5."""
    a = cpu_ambient(O, REFS, AO, ugrt, name)
    s, N, c = a["scene"], a["N"], a["counts"]
    print("%s: radius %r, %d hit pixels, mask non-zero %d, zero %d, per bit %s"
          % (name, a["radius"], int(a["oactive"].sum()), c["nonzero"], c["zero"], c["per_bit"]))
    assert c["nonzero"] >= 1000 and c["zero"] >= 1000, c
    assert min(c["per_bit"]) >= 100, c
    pr = a["base"]["primary"]
    np.testing.assert_array_equal(a["oactive"], ((pr["t"] > 0) & (pr["id"] >= 0)).astype(np.int32))
    assert not a["mask"][a["oactive"] == 0].any() and not (a["mask"] >> np.uint32(S_FRAME)).any()
    for k, rays in enumerate(a["expanded"]):
        brute = REFS[1].brute_any(s["verts"], s["faces"], rays, a["oactive"], a["radius"], 0, N, N)
        np.testing.assert_array_equal(brute.astype(np.uint32), (a["mask"] >> np.uint32(k)) & 1, err_msg="direction %d" % k)


def test_basis_is_orthonormal_and_the_pole_is_the_normal(AO):
    for n in NORMALS:
        T, B = AO.basis(n)
        n64, T64, B64 = n.astype(np.float64), T.astype(np.float64), B.astype(np.float64)
        for x, y in ((T64, n64), (B64, n64), (T64, B64)):
            assert abs(float(x @ y)) <= 1e-6, (n, T, B)
        assert abs(float(T64 @ T64) - 1) <= 1e-6 and abs(float(B64 @ B64) - 1) <= 1e-6
        orays = np.concatenate([np.asarray([1, 2, 3], np.float32), n])
        rays = AO.expand(orays, np.ones(1, np.int32), (0, 0, 1), 0, 1, 1)
        np.testing.assert_array_equal(bits(rays[3:]), bits(n))
        np.testing.assert_array_equal(bits(rays[:3]), bits(orays[:3]))
    # a tie for the smallest: +-z has |n0| == |n1| == 0 and must choose axis 0, u = (0, n2, -n1), T = (0, +-1, 0); axis 1
    # would give T = (-+1, 0, 0)
    for n, want in ((NORMALS[4], (0, 1, 0)), (NORMALS[5], (0, -1, 0))):
        T, _ = AO.basis(n)
        assert tuple(float(x) for x in T) == want, (n, T)
    # (1,1,0)/sqrt(2): |n0| == |n1| tie in the first comparison and axis 0 stays the winner of it, but |n2| = 0 is
    # smaller than both, so the rule of section 6.5 ends on axis 2: u = (n1, -n0, 0)
    T, _ = AO.basis(NORMALS[6])
    assert T[2] == 0 and T[0] > 0 and T[1] < 0 and bits(T)[0] == bits(-T)[1]
    # a strict winner in each place: (0, .6, .8) -> axis 0; (.6, 0, .8) -> axis 1; (.8, .6, 0) -> axis 2
    for n, zero in (((0, .6, .8), 0), ((.6, 0, .8), 1), ((.8, .6, 0), 2)):
        T, _ = AO.basis(np.asarray(n, np.float32))
        assert T[zero] == 0 and np.count_nonzero(T) == 2, (n, T)


def np_shade(img, mask, S, p0, n):
    img = img.copy().reshape(-1, 3)
    low = np.uint32(0xFFFFFFFF) if S == 32 else np.uint32((1 << S) - 1)
    m = mask[p0:p0 + n] & low
    closed = np.zeros(n, np.uint32)
    for s in range(S):
        closed += (m >> np.uint32(s)) & np.uint32(1)
    open_ = np.uint32(S) - closed
    img[p0:p0 + n] = ((img[p0:p0 + n].astype(np.uint32) * open_[:, None]) // np.uint32(S)).astype(np.uint8)
    return img.reshape(-1)


@pytest.mark.parametrize("S", [1, 5, 32])
def test_cpu_shade_is_the_integer_restatement(AO, S):
    rng = np.random.RandomState(S)
    N, p0, n = 1000, 100, 800
    img = rng.randint(0, 256, 3 * N).astype(np.uint8)
    img[3 * p0:3 * p0 + 30] = 255
    mask = rng.randint(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    mask[p0:p0 + 200] &= np.uint32(0x1F)
    mask[p0 + 200:p0 + 300] = 0
    mask[p0 + 300:p0 + 320] = 0xFFFFFFFF
    got = AO.shade(img, mask, S, p0, n)
    np.testing.assert_array_equal(got, np_shade(img, mask, S, p0, n))
    np.testing.assert_array_equal(got[:3 * p0], img[:3 * p0])
    np.testing.assert_array_equal(got[3 * (p0 + n):], img[3 * (p0 + n):])
    zero = slice(3 * (p0 + 200), 3 * (p0 + 300))
    np.testing.assert_array_equal(got[zero], img[zero])               # a zero mask leaves the bytes unchanged
    assert not got[3 * (p0 + 300):3 * (p0 + 320)].any()              # every direction occluded: black
    if S < 32:                                                       # bits at or above S are ignored
        high = mask.copy()
        high[p0:p0 + n] |= np.uint32((0xFFFFFFFF << S) & 0xFFFFFFFF)
        np.testing.assert_array_equal(AO.shade(img, high, S, p0, n), got)
        only_high = np.full(N, (0xFFFFFFFF << S) & 0xFFFFFFFF, np.uint32)
        np.testing.assert_array_equal(AO.shade(img, only_high, S, p0, n), img)


def test_ao_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    for bad in (-1, 33, 1.5, True, "4", None, np.float32(2)):
        with pytest.raises(ValueError):
            rmod.check_ao(bad, 1.0)
    for bad in (None, 0, 0.0, -1.0, float("nan"), "1", True, 1e-60):
        with pytest.raises(ValueError):
            rmod.check_ao(4, bad)
    with pytest.raises(ValueError):
        rmod.check_ao(4, 1.0, True)  # two streams / bands: the uniform grid lives on the side context
    assert rmod.check_ao(0, None) == (0, None) and rmod.check_ao(0, -3.0, True) == (0, None)
    assert rmod.check_ao(16, 0.5) == (16, 0.5) and rmod.check_ao(np.int64(32), np.float32(2)) == (32, 2.0)
    assert rmod.check_ao(1, 3) == (1, 3.0)
    s = scene(ugrt, "hall")
    for kw in (dict(ao=33, ao_radius=1.0), dict(ao=4), dict(ao=4, ao_radius=0.0), dict(ao=True, ao_radius=1.0)):
        r = RLT._fake_renderer(ugrt)
        with pytest.raises(ValueError):
            r.display(TL.setup_for(ugrt, s), **kw)
        assert r.ctx.calls == []
    r = RLT._fake_renderer(ugrt, aux=object())  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s), ao=4, ao_radius=1.0)
    assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    with pytest.raises(ValueError):
        br.display(TL.setup_for(ugrt, s), ao=4, ao_radius=1.0)


def test_ao_pass_enqueues_the_rays_and_one_walk(ugrt):
    import types

    rmod = RLT._rmod(ugrt)
    f = types.SimpleNamespace(t="t", dir="d", intersect_id="ids", d_verts="v", d_faces="f", reflect_eps=1e-3, ao_rays="orays",
                              ao_active="oact", ao_mask="mask")
    c = RS._Recorder()
    rmod.ao_pass(c, f, "cam", "dirs", 0.25)
    assert c.calls == [("ao_rays", "cam", "t", "d", "ids", "v", "f", 1e-3, "orays", "oact"),
                       ("trace_dda_any_hemi", "value", "span", "offset", "v", "f", "orays", "oact", "dirs", 0.25, "mask")]


# ------------------------------------------------------------------------------------------------- the synthetic rays

SYN_N = 4096
SYN_RADII = (0.5, 3.0, 3e38)  # half a cell, three cells (the cells are ~1 wide), every cell of the walk


def syn_ambient():
    """{o, n} for the 4096 pixels of the synthetic any-hit scene: origins on the plane z = 1.45 inside the box, just
    below the lattices of small triangles at z = 1.5 (three quarters of them under the lattices of the cells with 63,
    64, 65 and 129 triangles and next to them, the others anywhere on the plane), the eight normals of the basis cases in
    turn; 4035 = 126 * 32 + 3 pixels are active."""
    rng = np.random.RandomState(77)
    o = np.empty((SYN_N, 3), np.float64)
    o[:, :2] = rng.uniform(0.2, 7.8, (SYN_N, 2))
    cells = [RS.SYN_CELLS[k] for k in (63, 64, 65, 129)]
    for p in range(SYN_N):
        if p % 4:
            i, j = cells[(p // 4) % 4]
            o[p, :2] = rng.uniform([i - 0.5, j - 0.5], [i + 1.2, j + 1.2])
    o[:, 2] = 1.45
    orays = np.concatenate([o, NORMALS[np.arange(SYN_N) % len(NORMALS)]], 1).astype(np.float32).reshape(-1)
    oactive = np.ones(SYN_N, np.int32)
    oactive[rng.choice(SYN_N, 61, replace=False)] = 0
    return orays, oactive


_SYN_MASKS = {}


def syn_mask(REFS, AO, SYN, ugrt, S, radius, p0=0, n=SYN_N, keep=None):
    key = (S, radius, p0, n)
    if key not in _SYN_MASKS or keep is not None:
        orays, oactive = syn_ambient()
        _SYN_MASKS[key] = cpu_mask(REFS[1], AO, SYN["grid"], SYN["verts"], SYN["faces"], orays, oactive,
                                   ugrt.scenes.ao_directions(S), radius, p0, n, SYN_N, fill=0xFFFFFFFF, keep=keep)
    return _SYN_MASKS[key]


def test_synthetic_masks_are_not_vacuous(ugrt, O, REFS, AO, SYN):
    """CPU: 4035 active rays (no multiple of 32); at S = 32 bit 31 -- formed as 1u << 31 -- is set on at least 31 rays
    and clear on at least 31 at every radius; the walk equals brute force on every explicit ray."""
    orays, oactive = syn_ambient()
    assert int(oactive.sum()) == 4035 and int(oactive.sum()) % 32
    act = oactive != 0
    for radius in SYN_RADII:
        expanded = []
        mask = syn_mask(REFS, AO, SYN, ugrt, 32, radius, keep=expanded)
        top = (mask[act] >> np.uint32(31)) & 1
        print("radius %g: bit 31 set on %d rays, clear on %d; %d masks non-zero"
              % (radius, int(top.sum()), int((top == 0).sum()), int((mask[act] != 0).sum())))
        assert int(top.sum()) >= 31 and int((top == 0).sum()) >= 31
        assert not mask[~act].any()
        for s in (0, 13, 31):
            brute = REFS[1].brute_any(SYN["verts"], SYN["faces"], expanded[s], oactive, radius, 0, SYN_N, SYN_N)
            np.testing.assert_array_equal(brute.astype(np.uint32), (mask >> np.uint32(s)) & 1)


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _hemi(ctx, grid, dv, df, d_orays, d_oactive, dirs, radius, torch):
    mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)  # 0xFFFFFFFF
    ctx.trace_dda_any_hemi(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, dirs, radius, mask)
    ctx.synchronize()
    return _words(mask)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [None, (5, 21)])
def test_ao_rays_equal_the_cpu_rays(ugrt, O, REFS, AO, torch, rows):
    """hall 256 x 256, the whole frame and a band context: rays bit-equal and flags equal over the band, which is
    rewritten whole (the buffers start as garbage), and nothing outside it is touched."""
    a = cpu_ambient(O, REFS, AO, ugrt, "hall")
    s, N = a["scene"], a["N"]
    W, H = SIZES["hall"]
    ctx, r = RD.make(ugrt, s, W, H)
    r.display(RD.setup_for(ugrt, s), shadows=True, shade=False)  # the ids stay triangle ids
    ctx.synchronize()
    pr = a["base"]["primary"]
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), pr["id"])
    c = ctx if rows is None else ugrt.Context(W, H, light_grid=LG, uniform_dims=UD, rows=rows)
    p0, n = c.p0, c.npix
    assert (p0, n) == ((0, N) if rows is None else (5 * 8 * W, 16 * 8 * W))
    orays = torch.full((6 * N,), 7.0, device=ctx.device)
    oactive = torch.full((N,), 7, dtype=torch.int32, device=ctx.device)
    c.ao_rays(r.cam_pos, r.t, r.dir, r.intersect_id, r.d_verts, r.d_faces, EPS, orays, oactive)
    c.synchronize()
    w_rays, w_act = AO.rays(a["cam_pos"], pr["t"], pr["dir"], pr["id"], s["verts"], s["faces"], EPS, p0, n, N, fill=7.0)
    np.testing.assert_array_equal(oactive.cpu().numpy(), w_act)
    np.testing.assert_array_equal(bits(orays.cpu().numpy()), bits(w_rays))
    assert int(w_act[p0:p0 + n].sum()) > 1000
    # every pixel of the hall is a hit: the same with some t at or below 0 and some ids below 0
    t2, id2 = pr["t"].copy(), pr["id"].copy()
    t2[::7], t2[3::11], id2[5::13], id2[6::17] = 0.0, -1.0, -1, -2
    c.ao_rays(r.cam_pos, ctx.upload(t2), r.dir, ctx.upload(id2), r.d_verts, r.d_faces, EPS, orays, oactive)
    c.synchronize()
    m_rays, m_act = AO.rays(a["cam_pos"], t2, pr["dir"], id2, s["verts"], s["faces"], EPS, p0, n, N, fill=7.0)
    np.testing.assert_array_equal(oactive.cpu().numpy(), m_act)
    np.testing.assert_array_equal(bits(orays.cpu().numpy()), bits(m_rays))
    off = m_act[p0:p0 + n] == 0
    assert int(off.sum()) > 1000 and not m_rays.reshape(-1, 6)[p0:p0 + n][off].any()
    if rows is None:  # hits on materials that do not reflect get a ray too
        assert int(((w_act == 1) & (a["base"]["levels"][0]["active"] == 0)).sum()) > 1000
        np.testing.assert_array_equal(bits(w_rays), bits(a["orays"]))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 31, 32])
def test_synthetic_hemisphere_walk(ugrt, O, REFS, AO, SYN, torch, S):
    """List lengths 1, 7, 8, 9, 63, 64, 65 and 129, eight kinds of normals, 4035 rays, three radii, the mask
    pre-filled with ones: equal to the checker, and to S launches of ugrt_trace_dda_any on the explicit rays."""
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = syn_ambient()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    dirs = ugrt.scenes.ao_directions(S)
    for radius in SYN_RADII:
        expanded = []
        want = syn_mask(REFS, AO, SYN, ugrt, S, radius, keep=expanded)
        got = _hemi(ctx, grid, dv, df, d_orays, d_oactive, dirs, radius, torch)
        np.testing.assert_array_equal(got, want, err_msg="S %d radius %g" % (S, radius))
        assert not (got >> np.uint32(S)).any() if S < 32 else True
        assert not got[oactive == 0].any()
        composed = np.zeros(SYN_N, np.uint32)
        for s in range(S):
            occ = torch.full((SYN_N,), -7, dtype=torch.int32, device=ctx.device)
            ctx.trace_dda_any(grid[0], grid[1], grid[2], dv, df, ctx.upload(expanded[s]), d_oactive, radius, occ)
            composed |= occ.cpu().numpy().astype(np.uint32) << np.uint32(s)
        np.testing.assert_array_equal(got, composed, err_msg="S %d radius %g" % (S, radius))
        assert int((got != 0).sum()) >= 31
    if S == 32:
        top = (got[oactive != 0] >> np.uint32(31)) & 1
        assert int(top.sum()) >= 31 and int((top == 0).sum()) >= 31


@pytest.mark.gpu
def test_launch_shapes_change_no_mask(ugrt, O, REFS, AO, SYN, torch):
    """any_rays_per_wave x any_coop, dda_blocks = 1 (every later group comes from the ticket) and a band context whose
    other pixels keep their words."""
    S, radius = 32, 3.0
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = syn_ambient()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    dirs = ugrt.scenes.ao_directions(S)
    want = syn_mask(REFS, AO, SYN, ugrt, S, radius)
    for rpw in (1, 7, 32, 64):
        for coop in (1, 8, 1 << 30):
            ctx.set_option("any_rays_per_wave", rpw)
            ctx.set_option("any_coop", coop)
            got = _hemi(ctx, grid, dv, df, d_orays, d_oactive, dirs, radius, torch)
            np.testing.assert_array_equal(got, want, err_msg="rays per wave %d, coop %d" % (rpw, coop))
    ctx.set_option("any_rays_per_wave", -1)
    ctx.set_option("any_coop", -1)
    ctx.set_option("dda_blocks", 1)
    np.testing.assert_array_equal(_hemi(ctx, grid, dv, df, d_orays, d_oactive, dirs, radius, torch), want)
    ctx.set_option("dda_blocks", -1)
    band, bv, bf, bgrid = RS._syn_context(ugrt, SYN, (2, 5))
    p0, n = band.p0, band.npix
    assert (p0, n) == (1024, 1536)
    got = _hemi(band, bgrid, bv, bf, band.upload(orays), band.upload(oactive), dirs, radius, torch)
    np.testing.assert_array_equal(got, syn_mask(REFS, AO, SYN, ugrt, S, radius, p0, n))
    assert (got[:p0] == 0xFFFFFFFF).all() and (got[p0 + n:] == 0xFFFFFFFF).all()
    np.testing.assert_array_equal(got[p0:p0 + n], want[p0:p0 + n])


@pytest.mark.gpu
def test_the_walk_leaves_the_shared_dda_state_alone(ugrt, O, REFS, AO, torch):
    """hall: a ugrt_trace_dda before and after a hemisphere launch gives identical hits, and the split walks' figures
    stay what they were."""
    a = cpu_ambient(O, REFS, AO, ugrt, "hall")
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
    ctx.trace_dda_any_hemi(g[0], g[1], g[2], r.d_verts, r.d_faces, ctx.upload(a["orays"]), ctx.upload(a["oactive"]),
                           a["dirs"], a["radius"], mask)
    ctx.synchronize()
    np.testing.assert_array_equal(_words(mask), a["mask"])
    assert ctx.stats_dda_split() == before
    ht1, hid1 = level1()
    assert torch.equal(hid0, hid1) and torch.equal(ht0.view(torch.int32), ht1.view(torch.int32))
    np.testing.assert_array_equal(hid1.cpu().numpy(), a["base"]["levels"][0]["hit_id"])
    assert ctx.stats_dda_split() == before


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, REFS, AO, SYN, torch):
    fresh = ugrt.Context(64, 64, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS)
    z = torch.zeros(6 * SYN_N, dtype=torch.int32, device=fresh.device)
    dirs = ugrt.scenes.ao_directions(4)
    with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
        fresh.trace_dda_any_hemi(z, z, z, z, z, z, z, dirs, 1.0, z)
    assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = syn_ambient()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)
    args = [grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, dirs, 3.0, mask]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    for bad in (np.zeros((0, 3), np.float32), np.zeros((33, 3), np.float32)):
        fails(ctx.trace_dda_any_hemi, args[:7] + [bad] + args[8:], b"num_dirs")
    for bad in (0.0, -1.0, float("nan")):
        fails(ctx.trace_dda_any_hemi, args[:8] + [bad] + args[9:], b"radius")
    for h in (0, 3, 5, 6, 7, 9):
        fails(ctx.trace_dda_any_hemi, args[:h] + [None] + args[h + 1:], b"null")
    img = torch.full((3 * SYN_N,), 200, dtype=torch.uint8, device=ctx.device)
    for bad in (0, 33, -1):
        fails(ctx.shade_ao, [img, mask, bad], b"num_dirs")
    for h in (0, 1):
        a = [img, mask, 4]
        fails(ctx.shade_ao, a[:h] + [None] + a[h + 1:], b"null")
    ray_args = [d_orays, d_orays, d_orays, d_oactive, dv, df, EPS, d_orays, d_oactive]
    for h in (0, 1, 2, 3, 4, 5, 7, 8):
        fails(ctx.ao_rays, ray_args[:h] + [None] + ray_args[h + 1:], b"null")
    ctx.synchronize()
    assert (_words(mask) == 0xFFFFFFFF).all() and (img == 200).all()  # nothing was enqueued
    want = syn_mask(REFS, AO, SYN, ugrt, 4, 3.0)
    np.testing.assert_array_equal(_hemi(ctx, grid, dv, df, d_orays, d_oactive, dirs, 3.0, torch), want)
    # the shading on the device against the checker: S = 4 and 32 on that mask (bits at or above S are ignored)
    rng = np.random.RandomState(3)
    h_img = rng.randint(0, 256, 3 * SYN_N).astype(np.uint8)
    h_mask = rng.randint(0, 1 << 32, SYN_N, dtype=np.uint64).astype(np.uint32)
    h_mask[::3] = 0
    for S in (1, 4, 5, 32):
        d_img = ctx.upload(h_img)
        ctx.shade_ao(d_img, ctx.upload(h_mask.view(np.int32)), S)
        ctx.synchronize()
        np.testing.assert_array_equal(d_img.cpu().numpy(), AO.shade(h_img, h_mask, S, 0, SYN_N))


def _frames(O, REFS, LT, RL, ugrt, name):
    """(display keywords, uses lights, CPU image, CPU material ids) of the four one-stream frames."""
    W, H = SIZES[name]
    base = RS.cpu_frame(O, REFS, ugrt, name, W, H, DEPTH)
    plain = TL.cpu_frame(O, ugrt, name, W, H)
    l_img, l_ids = TL.cpu_image(LT, plain, 3)
    rl = RLT.cpu_frame(O, REFS, RL, ugrt, name, W, H, DEPTH)
    return [("plain", dict(shadows=True), False, plain["image"], plain["mat_ids"]),
            ("reflect", dict(shadows=True, reflect=True, bounces=DEPTH, reflect_shadows=True), False,
             base["image_occluded"], base["mat_ids_occluded"]),
            ("lights", dict(shadows=True), True, l_img, l_ids),
            ("reflect_lights", dict(bounces=DEPTH, **RLT.KW), True, rl["image"], rl["mat_ids"])]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "crash"])
def test_frames_with_ao_equal_the_cpu_frames(ugrt, O, REFS, AO, LT, RL, torch, name):
    """Plain with shadows, reflections of depth 3 with shadows, three lights, reflections under three lights: the
    image is the CPU frame's followed by ao_shade with the CPU mask, the material ids are the frame's own, ao_mask is
    the CPU mask; ao = 0 gives the CPU frame itself, also behind an ao frame on the same renderer."""
    a = cpu_ambient(O, REFS, AO, ugrt, name)
    s, N = a["scene"], a["N"]
    W, H = SIZES[name]
    assert feasible(a["counts"]), a["counts"]
    lights = TL.lights_for(s, 3)
    for what, kw, with_lights, w_img, w_ids in _frames(O, REFS, LT, RL, ugrt, name):
        setup = TL.setup_for(ugrt, s, lights if with_lights else None)
        ctx, r = RD.make(ugrt, s, W, H)
        r.display(setup, ao=0, **kw)
        ctx.synchronize()
        assert r.ao_mask is None
        np.testing.assert_array_equal(r.image.cpu().numpy(), w_img, err_msg=what)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        r.display(setup, ao=S_FRAME, ao_radius=a["radius"], **kw)
        ctx.synchronize()
        np.testing.assert_array_equal(_words(r.ao_mask), a["mask"], err_msg=what)
        np.testing.assert_array_equal(r.ao_active.cpu().numpy(), a["oactive"], err_msg=what)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        shaded = AO.shade(w_img, a["mask"], S_FRAME, 0, N)
        np.testing.assert_array_equal(r.image.cpu().numpy(), shaded, err_msg=what)
        assert int((shaded != w_img).sum()) > 1000
        r.display(setup, **kw)
        ctx.synchronize()
        np.testing.assert_array_equal(r.image.cpu().numpy(), w_img, err_msg=what + ", behind an ao frame")
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
