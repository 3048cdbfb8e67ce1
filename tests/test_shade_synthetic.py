"""The float shading calls on a g-buffer of their own: every guard, every branch, the level walk's three copies.

ugrt_shade_simple, _spotlight, _add_shadows, _lights, _reflect, _reflect_depth, _reflect_depth_occluded and
_reflect_lights are otherwise fed scene frames only: unit normals, t well above zero, consistent level chains, flags
0 or 1, reflect in [0, 1].  Here one seeded fixture, built with numpy in float64 and rounded once to float32, holds what
a scene never does.  It needs no scene and no tracing.

Image 136 x 72 = 9 792 pixels (38 blocks of PX_THREADS and a tail of 64; 9 tile rows).  The camera block is a fixed light
camera's as oracle_lib forms it (eye (3,4,5), looking along (12,0,5)/13: `up` is the y axis exactly, right and forward are
generic in the xz plane, so a projection can vanish exactly and an acosf argument can round past 1); the shading light
is its eye, lights 1..7 lie dyadic offsets from it; the eye of the image is the origin.

Every pixel has three classes, dealt independently with seeded permutations (PRIMARY, CHAIN, flag value of light 0):
* PRIMARY: id -1 with t 0, id -2, each out-of-range material (-1, -2, num_materials, INT_MAX); t +0, -0, negative,
  denormal, 1e30, +inf, NaN; normals of length 1e-20, 1e-30, 1e20, zero, with a NaN, exactly perpendicular to the light
  direction (dot 0, +-denormal); the point on light l bit for bit (l = 0..7), 1e-6 and 1e6 from the light; colours of
  exactly 1, the float below and the float above before the clamp (Kd = 2/3 and its neighbours); colours whose product
  with 255 is an integer to within 2 ulps either side; spot angles within 16 ulps of +-pi/4 in x, in y and in both;
  points on the light's axes (the projected vector is 0: 0/0) and points whose acosf argument rounds past 1.
* CHAIN (8 levels): ends at every level 0..8; active values 2, -1, INT_MIN; a missed level and a level with an
  out-of-range material, each followed by an active and by an inactive level; hits on degenerate triangles (two equal
  vertices, collinear, edges of 1e-20 and 1e20); hit_t 0, negative, denormal, 1e30, NaN; reflect 1e-10 all the way (w
  reaches a denormal, then 0); reflect 1.5 all the way; levels on the materials with NaN or negative Kd and NaN reflect.
* flags: is_shadowed and occluded values 0, 1, 2, 7, -1 per light and per level; only 1 darkens.

"Undefined cast" rows: the last 9 pixel rows (1 224 pixels, 1/8) hold the PRIMARY classes whose colour before the byte
conversion is NaN or negative, which are the materials with a NaN or a negative Kd, and nothing else.  ugrt_f2u
defines the conversion (0 for both); host-compiled C does not, so tests/golden/ref_kernels_shadesyn.npz, the record of
the reference's own lambertian_shade + shadow_kernel and spot_shade on these inputs, leaves those rows out by their row
index.  The point on the light and the normals that normalise to NaN are NOT there: a NaN dot product fails
`dot_diffuse > 0` twice, the colour is the ambient term alone, which is defined, and the reference's kernels are
compared on those pixels too.  Because the rows lie behind tile row 7 no class of them is in the band 3..6, and the
frame's tail block lies inside them; so the band (0, 1), 1 088 pixels with a tail block of its own, and the band (6, 9)
are run besides the frame and the band (3, 7), and every other class has a pixel in the tail block of band (0, 1).

CPU tests (unmarked): conditions on the checkers alone that let the GPU tests fail; the checkers against each other
where the header says two calls are equal; the oracle, and the live binary where built, against the record.
GPU tests: the eight exports against their checkers, image bytes, ids as written back and the spot dump's bits equal, on
the frame and the three bands, depths 1, 2, 3, 5, 8, lights 1, 2, 3, 8, with and without flags; the header's identities
on the device; libugrt.so against the record.  No tolerance anywhere.

Figures of the fixture (seed 20261020), measured on the CPU:
  PRIMARY classes 43: 41 in the first 63 rows with 208 or 209 pixels each (90 to 121 of them in the band 3..6, one or more
  in the tail block of band 0), 2 in the last 9 rows with 612 each; CHAIN classes 23 with 425 to 427 pixels each (176 to
  208 in the band); flag classes 5 with 1 958 or 1 959 each (844 to 895 in the band).  348 triangles (300 ordinary, 32 on
  the out-of-range, undefined-cast and black materials, 16 degenerate), 14 materials.
  Normals whose colour * 255 lies within 2.5 ulps of an integer: 484 found for k = 128..254 (209 pixels, 121 distinct k).
  Points whose acosf argument rounds past 1 or -1: 448 of 200 000 tried near the light's forward axis (209 pixels).
  Spot angles: the oracle's acosf returns neither the float of pi/4 nor the one above it; within 18 ulps the angles found
  are -17 -16 -15 -13 -11 -10 -8 -7 -6 -4 -3 -2 -1 | +2 +3 +4 +6 +7 +8 +10 +11 +12 +15 +16 +17 +18 ulps from +-pi/4 (the
  first float outside the face is 2 ulps out), every one of them in x alone, in y alone and in both, on both signs.
  Observability, pixels of the class whose bytes change under the tame counterpart:
    denormal t -> 0 209 of 209; active 2 -> 0 354 of 426; flag 2 -> 1 1 509 of 1 958; out-of-range material -> material 0
    836 of 836; kr reset to 0 on a missed level 350 of 425; chain cut at depth 7 332 of 426; spot point moved 16 to 24
    ulps across the face 627 of 627; clamp removed 209 of 209; a miss / a bad material followed by an active level made
    consistent 350 / 330 of 425.
Measured on an MI355X: the 82 GPU tests of this file take 3.3 s together (the slowest, the first, 0.7 s: it makes the four
contexts), and all pass: no export differs from its checker, and the record equals both.  The device keeps fp32 denormals in
every operation these kernels use: the classes "t denormal" (the comparison t > 0), "normal 1e-20" (the squares, the square
root and the division of D_NORMALIZE), "normal perpendicular, dot +-denormal", the 1e-20 triangle and "reflect 1e-10 all the
way" (the products of w) give the checker's bytes; a build of the shading unit that flushes them
(-fgpu-flush-denormals-to-zero) fails 71 of the 82 (ugrt_shade_simple on 401 pixels of the frame, first of class "normal
1e-20").  Builds with other single faults: `!= 0` in place of `== 1` on the flags fails 34; `== 1` in place of non-zero on
d_active 54 (1 049 pixels, first "active INT_MIN"); k reset to 0 on a level without colour in k_shade_reflect_lights alone 26
(that export's tests from depth 3 on and the two identities that pair it with the depth kernel; 118 to 684 pixels, first
"miss, then active"); d_clamp1 left out of k_shade 11.
"""
import functools
import types

import numpy as np
import pytest

import test_lights as TL
import test_reflect_depth as RD
import test_reference_kernels as RK
from test_lights import LT  # noqa: F401  (fixtures)
from test_reflect_lights import RL  # noqa: F401
from test_reflect_shadows import REFS  # noqa: F401

W, H = TL.ODD
N = W * H
DEPTH, LIGHTS = 8, 8
UNDEF_ROWS = 9
U0 = (H - UNDEF_ROWS) * W  # the first pixel of the undefined-cast rows
BANDS = {"frame": None, "band 3..6": (3, 7), "band 0": (0, 1), "band 6..8": (6, 9)}
MAIN_BAND = (3, 7)
TAIL = (1024, 1088)  # the tail block of band (0, 1)
SEED = 20261020
LIGHT = dict(eye=(3.0, 4.0, 5.0), look=(15.0, 4.0, 10.0), up=(0.0, 1.0, 0.0), near=0.1, far=100.0)
LIGHT_OFFSETS = np.array([(0, 0, 0), (2, 0, 0), (0, -4, 0), (0, 0, 8), (-1, 1, 0), (0.5, 0, -2), (16, 16, 16), (-8, 0, 4)],
                         np.float64)
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
DEN = np.float32(1e-40)
F23 = np.float32(2.0 / 3.0)
QPI = np.float32(np.pi / 4)
BYTE, ID, DUMP = 0xA5, -7, np.float32(7.0)  # the sentinels
# Kd and reflect per material; 10..12 are used by the undefined-cast rows and by the chains alone, 13 is black
MATERIALS = [((0.6, 0.4, 0.25), 0.0), ((0.0, 0.25, F23), 1.0), ((1.0, 1.0, 1.0), 0.5), ((3.0, 0.25, 1.0), 0.25),
             ((DEN, F23, 0.25), 1.5), ((0.25, 0.25, 0.25), -0.5),
             ((np.nextafter(F23, np.float32(0)), F23, np.nextafter(F23, np.float32(1))), DEN),
             ((0.5, 0.75, 0.125), 0.5), ((0.9, 0.1, 0.4), 1e-10), ((0.3, 0.3, 0.9), 1.0),
             ((-0.25, 0.5, 0.25), 0.5), ((np.nan, 0.5, 0.25), 0.5), ((0.5, 0.5, 0.5), np.nan), ((0.0, 0.0, 0.0), 0.0)]
M = len(MATERIALS)
TAME = tuple(range(10))
BAD_MATERIALS = (-1, -2, M, INT_MAX)
FLAG_VALUES = np.int32([0, 1, 2, 7, -1])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def band_of(rows):
    lo, hi = rows if rows is not None else (0, H // 8)
    return lo * 8 * W, (hi - lo) * 8 * W


# ------------------------------------------------------------------------------------------------ the spot light's points

def spot_angles(O, cc, P):
    """(x, y) of the oracle's spot shading for points P ([n, 3] float32; the eye at the origin, t = 1)."""
    P = np.ascontiguousarray(P, np.float32)
    n = len(P)
    dump = np.zeros(2 * n, np.float32)
    O.shade(cc, cc[:3], np.zeros(3 * n, np.uint8), np.zeros(3 * n, np.float32), np.ones(n, np.float32), P.reshape(-1),
            np.full(n, -2, np.int32), np.zeros(3, np.float32), np.zeros(1, np.int32), np.zeros(6, np.float32), 0, n,
            spot=True, dump=dump)
    return dump[0::2].copy(), dump[1::2].copy()


def spot_frame(cc):
    E = cc[:3].astype(np.float64)
    r, u, f = (np.array([cc[16 + k], cc[20 + k], cc[24 + k]], np.float64) for k in range(3))
    return E, r, u, f


def spot_root(O, cc, which):
    """theta > 0 at which the oracle's angle `which` (0: x, 1: y) of E + 8 (f + tan(theta) axis) crosses pi/4."""
    E, r, u, f = spot_frame(cc)
    axis = r if which == 0 else u
    lo, hi = 0.05, 1.5
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        a = spot_angles(O, cc, (E + 8.0 * (f + np.tan(mid) * axis))[None, :])[which][0]
        lo, hi = (mid, hi) if abs(a) < QPI else (lo, mid)
    return 0.5 * (lo + hi)


def ulps_from_qpi(a):
    """|a| in ulps from pi/4: negative inside the cone's face (|a| < pi/4), 0 and up outside."""
    return bits(np.abs(a)).astype(np.int64) - int(bits(QPI)[0])


def spot_points(O, cc, rng):
    """Points whose spot angles lie within 24 ulps of +-pi/4: {(kind, sx, sy): (P, ulps x, ulps y)}, kind "x" (y well
    inside), "y" (x well inside) or "both"."""
    E, r, u, f = spot_frame(cc)
    roots = (spot_root(O, cc, 0), spot_root(O, cc, 1))
    out, n = {}, 60000
    for kind in ("x", "y", "both"):
        for sx in (1, -1):
            for sy in (1, -1):
                if (kind == "x" and sy < 0) or (kind == "y" and sx < 0):
                    continue
                near = lambda root: root + rng.uniform(-40, 40, n) * 6e-8
                tx = sx * (near(roots[0]) if kind != "y" else np.full(n, 0.2))
                ty = sy * (near(roots[1]) if kind != "x" else np.full(n, 0.2))
                s = rng.uniform(2.0, 40.0, n)
                P = (E + s[:, None] * (f + np.tan(tx)[:, None] * r + np.tan(ty)[:, None] * u)).astype(np.float32)
                x, y = spot_angles(O, cc, P)
                ux, uy = ulps_from_qpi(x), ulps_from_qpi(y)
                ok = (np.sign(x) == sx) & (np.sign(y) == sy)
                ok &= (np.abs(ux) <= 24) if kind != "y" else (ux < -1000)
                ok &= (np.abs(uy) <= 24) if kind != "x" else (uy < -1000)
                out[(kind, sx, sy)] = (P[ok], ux[ok], uy[ok])
    return out


def pick_spot(found, count, rng):
    """`count` points of one kind: first one per attainable offset within 18 ulps on either side (for "both", of x and
    of y), then at random within 2 ulps; and per point the counterpart 16 to 24 ulps on the other side of the face (the
    drop-off flips)."""
    P, ux, uy, kinds = [], [], [], []
    for key, (p, x, y) in sorted(found.items()):
        P.append(p), ux.append(x), uy.append(y), kinds.append(np.full(len(p), key[0] == "y"))
    P, ux, uy, is_y = np.concatenate(P), np.concatenate(ux), np.concatenate(uy), np.concatenate(kinds)
    wanted = range(-18, 19)
    chosen = []
    for axis_ulps in ((uy,) if is_y.all() else (ux,) if abs(uy).min() > 1000 else (ux, uy)):
        for o in wanted:
            hit = np.flatnonzero(axis_ulps == o)
            chosen += list(rng.choice(hit, min(1, hit.size), replace=False))
    close = np.flatnonzero((np.abs(ux) <= 2) | (np.abs(uy) <= 2))
    chosen = (chosen + list(rng.choice(close, count)))[:count]
    inside = (ux < 0) & (uy < 0)
    deep_in = np.flatnonzero((ux <= -16) & (uy <= -16))
    deep_out = np.flatnonzero(((ux >= 16) & (uy < 0)) | ((uy >= 16) & (ux < 0)))
    other = np.where(inside[chosen], rng.choice(deep_out, len(chosen)), rng.choice(deep_in, len(chosen)))
    return P[chosen], ux[chosen], uy[chosen], P[other]


def past_one_points(O, cc, rng, count):
    """Points near the light's forward axis and behind it whose acosf argument in d_along_x rounds past +1 or -1: the
    angle is NaN though the projected vector is nowhere near 0."""
    E, r, u, f = spot_frame(cc)
    n = 200000
    s = rng.uniform(1.0, 60.0, n) * rng.choice([1.0, -1.0], n)
    aside, above = rng.uniform(-2e-3, 2e-3, n)[:, None] * r, rng.uniform(-0.5, 0.5, n)[:, None] * u
    P = (E + s[:, None] * (f + aside + above)).astype(np.float32)
    x, _ = spot_angles(O, cc, P)
    hit = np.flatnonzero(np.isnan(x))
    return P[hit[:count]], hit.size, n


# ------------------------------------------------------------------------------------------------ the fixture

def deal(rng, names, lo, hi, forced):
    """A class index per pixel of [lo, hi): a seeded permutation deals the classes round robin; the pixels of
    `forced` (the tail block of band (0, 1)) are dealt first, so that every class has one there."""
    idx = np.full(N, -1)
    px = np.arange(lo, hi)
    first = px[(px >= forced[0]) & (px < forced[1])]
    rest = rng.permutation(px[(px < forced[0]) | (px >= forced[1])])
    order = np.concatenate([rng.permutation(first), rest])
    idx[order] = np.arange(order.size) % len(names)
    return idx


@functools.lru_cache(maxsize=None)
def synthetic(O):
    rng = np.random.default_rng(SEED)
    S = types.SimpleNamespace(W=W, H=H, N=N)
    lcam = O.cam_from(LIGHT, 45.0, float(np.float32(W) / np.float32(H)))
    cc = S.cc = lcam.cc
    assert cc[21] == 1.0 and cc[17] == 0 and cc[25] == 0 and cc[20] == 0 and cc[22] == 0  # `up` is the y axis exactly
    E = cc[:3].astype(np.float64)
    S.lights = (E + LIGHT_OFFSETS).astype(np.float32)
    assert (S.lights.astype(np.float64) == E + LIGHT_OFFSETS).all()
    S.light = S.lights[0]
    S.cam_pos = np.zeros(3, np.float32)
    # -- materials
    S.mat_list = np.zeros((M, 6), np.float32)
    S.mat_list[:, :3] = 0.1
    S.mat_list[:, 3:] = [kd for kd, _ in MATERIALS]
    S.reflect = np.float32([k for _, k in MATERIALS])
    # -- triangles: ordinary ones over three decades of size, materials 0..9 in turn; then ordinary ones on each
    # out-of-range and each undefined-cast material and on black; then the degenerate ones
    tris, mats, S.tri = [], [], {}

    def add(key, t9, m):
        S.tri.setdefault(key, []).append(len(tris))
        tris.append(np.asarray(t9, np.float64).reshape(3, 3))
        mats.append(m)

    def ordinary():
        c = rng.uniform(-20.0, 20.0, 3)
        return c + rng.normal(size=(3, 3)) * np.exp(rng.uniform(np.log(1e-2), np.log(1e1)))

    for i in range(300):
        add(("mat", i % 10), ordinary(), i % 10)
    for m in BAD_MATERIALS + (10, 11, 12, 13):
        for _ in range(4):
            add(("mat", m), ordinary(), m)
    for i in range(4):
        v = ordinary()
        add(("deg", "equal"), [v[0], v[0], v[2]], i)
        add(("deg", "collinear"), [v[0], v[0] + (v[1] - v[0]) * 0.5, v[0] + (v[1] - v[0]) * 2.0], i)
        add(("deg", "1e-20"), rng.normal(size=(3, 3)) * 1e-20, i)
        add(("deg", "1e20"), rng.normal(size=(3, 3)) * 1e20, i)
    S.verts = np.ascontiguousarray(np.asarray(tris).reshape(-1), np.float32)
    v = S.verts.reshape(-1, 3, 3)
    for k in S.tri[("deg", "collinear")]:  # (collinear after the rounding too: dyadic steps along one axis)
        v[k, 1], v[k, 2] = v[k, 0] + np.float32([0.5, 0, 0]), v[k, 0] + np.float32([2, 0, 0])
    S.faces = np.arange(3 * len(tris), dtype=np.int32)
    S.F = len(tris)
    S.mat_idx = np.asarray(mats, np.int64).astype(np.int32)
    of = lambda key, n: rng.choice(S.tri[key], n)
    tame_tri = np.flatnonzero(np.isin(S.mat_idx, TAME) & (np.arange(S.F) < 300))

    # -- the ordinary pixel
    P = E + unit(rng.normal(size=(N, 3))) * np.exp(rng.uniform(np.log(0.5), np.log(50.0), N))[:, None]
    t = np.linalg.norm(P, axis=1)
    dirs = P / t[:, None]
    normal = unit(rng.normal(size=(N, 3)))
    # (the ordinary pixel reflects: reflect 0, denormal and 1e-10 start a chain only in the classes that are about them)
    ids = rng.choice(tame_tri[np.isin(S.mat_idx[tame_tri], (1, 2, 3, 4, 5, 7, 9))], N).astype(np.int64)
    alt = np.full((N, 3), np.nan)  # the spot classes' counterpart points

    def point(px, p):  # exact: the eye is the origin, t = 1, dir = the point
        t[px] = 1.0
        dirs[px] = p

    # -- PRIMARY classes
    classes = []  # (name, undefined cast, builder(px))

    def cls(name, undefined=False):
        def reg(fn):
            classes.append((name, undefined, fn))
            return fn
        return reg

    cls("ordinary")(lambda px: None)
    cls("ordinary 2")(lambda px: None)

    @cls("id -1, t 0")
    def _(px):
        ids[px], t[px] = -1, 0.0

    @cls("id -2")
    def _(px):
        ids[px] = -2

    for m in BAD_MATERIALS:
        cls("material %d" % m)(lambda px, m=m: ids.__setitem__(px, of(("mat", m), px.size)))
    for name, val in (("t +0", 0.0), ("t -0", -0.0), ("t denormal", float(DEN)), ("t 1e30", 1e30), ("t +inf", np.inf),
                      ("t NaN", np.nan)):
        cls(name)(lambda px, val=val: t.__setitem__(px, val))

    @cls("t negative")
    def _(px):
        t[px] = -t[px]

    for name, scale in (("normal 1e-20", 1e-20), ("normal 1e-30", 1e-30), ("normal 1e20", 1e20), ("normal zero", 0.0)):
        def _(px, scale=scale):
            normal[px] *= scale
            ids[px] = rng.choice(S.tri[("mat", 0)] + S.tri[("mat", 2)] + S.tri[("mat", 7)], px.size)  # Kd > 0
        cls(name)(_)

    @cls("normal with a NaN")
    def _(px):
        normal[px, rng.integers(0, 3, px.size)] = np.nan

    # the light direction in the xz plane (the point at the light's height), the normal along y: the dot product is 0;
    # a normal with 1e-40 of x besides gives +-6e-41 or so
    for name, dx in (("normal perpendicular, dot 0", 0.0), ("normal perpendicular, dot denormal", 1e-40),
                     ("normal perpendicular, dot -denormal", -1e-40)):
        def _(px, dx=dx):
            a = rng.uniform(0, 2 * np.pi, px.size)
            point(px, E + np.stack([np.cos(a), 0 * a, np.sin(a)], 1) * rng.uniform(1.0, 9.0, px.size)[:, None])
            normal[px] = np.stack([dx * np.sign(np.cos(a)), 1 + 0 * a, 0 * a], 1)
        cls(name)(_)

    for l in range(LIGHTS):
        cls("point on light %d" % l)(lambda px, l=l: point(px, S.lights[l].astype(np.float64)))
    cls("1e-6 from the light")(lambda px: point(px, E + unit(rng.normal(size=(px.size, 3))) * 1e-6))
    cls("1e6 from the light")(lambda px: point(px, E + unit(rng.normal(size=(px.size, 3))) * 1e6))

    # material 6 two units above the light, the normal along y: the colour is 1.5 Kd = the float below 1, 1, the float
    # above 1
    @cls("colour below 1, 1, above 1")
    def _(px):
        point(px, E + [0.0, 2.0, 0.0])
        normal[px] = [0.0, 2.0, 0.0]
        ids[px] = of(("mat", 6), px.size)

    # material 2 (Kd 1) there: the colour is 0.5 + the y of a normal whose squares sum to 1 exactly
    targets = near_integer_normals(cc)
    S.near_integer = len(targets)

    @cls("colour * 255 near an integer")
    def _(px):
        point(px, E + [0.0, 2.0, 0.0])
        normal[px] = targets[np.linspace(0, len(targets) - 1, px.size).astype(int)]
        ids[px] = of(("mat", 2), px.size)

    @cls("Kd 3")
    def _(px):
        ids[px] = of(("mat", 3), px.size)

    found = spot_points(O, cc, rng)
    S.spot_offsets = {}
    for kind in ("x", "y", "both"):
        def _(px, kind=kind):
            p, ux, uy, other = pick_spot({k: v for k, v in found.items() if k[0] == kind}, px.size, rng)
            point(px, p.astype(np.float64))
            alt[px] = other
            S.spot_offsets[kind] = (sorted(set(ux[np.abs(ux) <= 24])), sorted(set(uy[np.abs(uy) <= 24])))
        cls("spot angle at the face, " + kind)(_)

    _, r_, u_, f_ = spot_frame(cc)

    @cls("point on the light's axes")
    def _(px):
        axes = np.array([f_, -f_, r_, -r_, u_, -u_]).astype(np.float32).astype(np.float64)
        point(px, E + axes[np.arange(px.size) % 6] * np.float64(2.0) ** rng.integers(0, 4, px.size)[:, None])

    past, S.past_one_found, S.past_one_tried = past_one_points(O, cc, rng, 400)

    @cls("acosf argument past 1")
    def _(px):
        point(px, past[np.arange(px.size) % len(past)].astype(np.float64))

    cls("Kd negative", True)(lambda px: ids.__setitem__(px, of(("mat", 10), px.size)))
    cls("Kd NaN", True)(lambda px: ids.__setitem__(px, of(("mat", 11), px.size)))

    S.primary_names = [c[0] for c in classes]
    S.undefined = np.array([c[1] for c in classes])
    defined = [i for i, c in enumerate(classes) if not c[1]]
    undefined = [i for i, c in enumerate(classes) if c[1]]
    S.primary = np.full(N, -1)
    S.primary[:U0] = np.asarray(defined)[deal(rng, defined, 0, U0, TAIL)[:U0]]
    S.primary[U0:] = np.asarray(undefined)[deal(rng, undefined, U0, N, (N - 64, N))[U0:]]
    for i, (_, _, fn) in enumerate(classes):
        fn(np.flatnonzero(S.primary == i))
    S.t = t.astype(np.float32)
    S.dirs = np.ascontiguousarray(dirs.astype(np.float32).reshape(-1))
    S.normal = np.ascontiguousarray(normal.astype(np.float32).reshape(-1))
    S.ids = ids.astype(np.int32)
    S.alt_dirs = alt.astype(np.float32)
    exact = np.flatnonzero(np.isin(S.primary, [S.primary_names.index("point on light %d" % l) for l in range(LIGHTS)]))
    lit_by = S.primary[exact] - S.primary_names.index("point on light 0")
    assert (S.cam_pos + S.t[exact, None] * S.dirs.reshape(-1, 3)[exact] == S.lights[lit_by]).all()

    # -- CHAIN classes: level j (0-based) of the stacked arrays is level j + 1 of the header
    NL = DEPTH * N
    ray_o = rng.uniform(-20.0, 20.0, (DEPTH, N, 3))
    rays = np.concatenate([ray_o, unit(rng.normal(size=(DEPTH, N, 3)))], 2)
    active = np.ones((DEPTH, N), np.int64)
    hit_t = rng.uniform(0.5, 20.0, (DEPTH, N))
    hit_id = rng.choice(tame_tri, (DEPTH, N)).astype(np.int64)
    chains = []

    def chain(name):
        def reg(fn):
            chains.append((name, fn))
            return fn
        return reg

    for j in range(DEPTH + 1):
        def _(px, j=j):
            # mirrors (reflect 1) all the way, so that the last level reached is what the pixel shows
            hit_id[:, px] = rng.choice(S.tri[("mat", 1)] + S.tri[("mat", 9)], (DEPTH, px.size))
            if j < DEPTH:
                active[j, px] = 0
                active[j + 1:, px] = rng.integers(0, 2, (DEPTH - j - 1, px.size))  # (never reached)
        chain("chain ends at level %d" % j if j < DEPTH else "chain of full depth")(_)
    for name, val in (("active 2", 2), ("active -1", -1), ("active INT_MIN", INT_MIN)):
        chain(name)(lambda px, val=val: active.__setitem__((slice(None), px), val))
    for what, then in (("miss", 1), ("miss", 0), ("bad material", 1), ("bad material", 0)):
        def _(px, what=what, then=then):
            # mirrors in front; m: the level that has no colour; the one before it reflects half
            hit_id[:, px] = rng.choice(S.tri[("mat", 1)] + S.tri[("mat", 9)], (DEPTH, px.size))
            m = rng.integers(1, DEPTH - 1, px.size)
            hit_id[m - 1, px] = rng.choice(S.tri[("mat", 2)] + S.tri[("mat", 7)], px.size)
            hit_id[m + 1, px] = rng.choice(tame_tri, px.size)
            if what == "miss":
                hit_id[m, px] = rng.choice([-1, -2], px.size)
            else:
                hit_id[m, px] = [of(("mat", b), 1)[0] for b in rng.choice(BAD_MATERIALS, px.size)]
            active[m + 1, px] = then
        chain("%s, then %s" % (what, "active" if then else "inactive"))(_)

    @chain("hit on a degenerate triangle")
    def _(px):
        kinds = ("equal", "collinear", "1e-20", "1e20")
        for i, p in enumerate(px):
            hit_id[rng.integers(0, DEPTH), p] = of(("deg", kinds[i % 4]), 1)[0]

    @chain("odd hit_t")
    def _(px):
        vals = (0.0, -3.0, float(DEN), 1e30, np.nan)
        for i, p in enumerate(px):
            hit_t[rng.integers(0, DEPTH), p] = vals[i % 5]

    @chain("reflect 1e-10 all the way")
    def _(px):
        hit_id[:, px] = rng.choice(S.tri[("mat", 8)], (DEPTH, px.size))

    @chain("reflect 1.5 all the way")
    def _(px):
        hit_id[:, px] = rng.choice(S.tri[("mat", 4)], (DEPTH, px.size))

    @chain("reflect -0.5 and denormal")
    def _(px):
        hit_id[:, px] = rng.choice(S.tri[("mat", 5)] + S.tri[("mat", 6)], (DEPTH, px.size))

    @chain("NaN or negative Kd, NaN reflect on a level")
    def _(px):
        for i, p in enumerate(px):
            hit_id[rng.integers(0, DEPTH), p] = of(("mat", 10 + i % 3), 1)[0]

    chain("random chain")(lambda px: active.__setitem__((slice(None), px), rng.integers(0, 2, (DEPTH, px.size))))
    S.chain_names = [c[0] for c in chains]
    S.chain = np.concatenate([deal(rng, chains, 0, U0, TAIL)[:U0], deal(rng, chains, U0, N, (N - 64, N))[U0:]])
    for i, (_, fn) in enumerate(chains):
        fn(np.flatnonzero(S.chain == i))
    # the chains that are about their reflect values start on them: the primary material, where the pixel is ordinary
    plain = S.primary <= 1
    for name, m in (("reflect 1e-10 all the way", 8), ("reflect 1.5 all the way", 4)):
        px = np.flatnonzero(plain & (S.chain == S.chain_names.index(name)))
        S.ids[px] = of(("mat", m), px.size)
    mirrors = np.flatnonzero(plain & (S.chain <= S.chain_names.index("active INT_MIN")))
    S.ids[mirrors] = rng.choice(S.tri[("mat", 1)] + S.tri[("mat", 9)] + S.tri[("mat", 2)], mirrors.size)
    S.rays = np.ascontiguousarray(rays.astype(np.float32).reshape(-1))
    S.active = active.astype(np.int32).reshape(-1)
    S.hit_t = hit_t.astype(np.float32).reshape(-1)
    S.hit_id = hit_id.astype(np.int32).reshape(-1)
    assert S.rays.size == 6 * NL and S.active.size == NL

    # -- flags: light 0's value is the pixel's flag class
    S.flag_class = deal(rng, FLAG_VALUES, 0, N, TAIL)
    S.shadowed = rng.choice(FLAG_VALUES, (LIGHTS, N), p=[0.35, 0.35, 0.1, 0.1, 0.1]).astype(np.int32)
    S.shadowed[0] = FLAG_VALUES[S.flag_class]
    S.occluded = rng.choice(FLAG_VALUES, (DEPTH, LIGHTS, N), p=[0.35, 0.35, 0.1, 0.1, 0.1]).astype(np.int32)
    for a in (S.t, S.dirs, S.normal, S.ids, S.rays, S.active, S.hit_t, S.hit_id, S.shadowed, S.occluded, S.verts,
              S.mat_idx, S.mat_list, S.reflect, S.lights, S.cc):
        a.setflags(write=False)
    return S


def near_integer_normals(cc):
    """Normals (0, x, z) for the colour 0.5 + x of a Kd 1 material lit along y: x + 0.5 is the float nearest to k / 255
    or one of its two neighbours on either side, k = 128..254, and z is nudged until the squares of the view-space normal
    sum to exactly 1, so that the normalisation multiplies by 1."""
    f = np.float32
    out = []
    for k in range(128, 255):
        c0 = f(k / 255.0)
        for step in range(-2, 3):
            c = c0
            for _ in range(abs(step)):
                c = np.nextafter(c, f(2.0 if step > 0 else 0.0))
            x = f(c - f(0.5))
            z = f(np.sqrt(1.0 - float(x) ** 2))
            for cand in z + np.arange(-3, 4).astype(f) * np.spacing(z):
                n = np.array([0, x, cand], f)
                nv = [f(f(f(cc[16 + q] * n[0]) + f(cc[20 + q] * n[1])) + f(cc[24 + q] * n[2])) for q in range(3)]
                if f(f(f(nv[0] * nv[0]) + f(nv[1] * nv[1])) + f(nv[2] * nv[2])) == f(1.0) and nv[1] == x:
                    out.append(n)
                    break
    return np.asarray(out, np.float64)


def class_of(S, p):
    return "pixel %d (row %d): %s / %s / flag %d" % (p, p // W, S.primary_names[S.primary[p]], S.chain_names[S.chain[p]],
                                                      FLAG_VALUES[S.flag_class[p]])


# ------------------------------------------------------------------------------------------------ the checkers

def want(O, REFS, LT, RL, S, call, rows=None, depth=DEPTH, L=1, flags=True, **over):
    """(image, ids, dump or None) of the checker of `call` on the fixture (or on `over` in an array's place)."""
    p0, n = band_of(rows)
    g = lambda k: over.get(k, getattr(S, k))
    prim = (g("normal"), g("t"), g("dirs"), g("ids"), S.cam_pos, g("mat_idx"), S.mat_list)
    lev = (g("rays"), g("active"), g("hit_t"), g("hit_id"))
    geo = (g("reflect"), S.verts, S.faces)
    img, ids, dump = np.zeros(3 * N, np.uint8), g("ids").copy(), None
    if call in ("simple", "spotlight", "simple+shadows"):
        dump = np.zeros(2 * N, np.float32) if call == "spotlight" else None
        O.shade(S.cc, S.light, img, *prim[:3], ids, *prim[4:], p0, n, spot=call == "spotlight", dump=dump)
        if call == "simple+shadows":
            O.add_shadows(img, np.ascontiguousarray(g("shadowed")[0]), p0, n)
    elif call == "add_shadows":
        img = over["img"].copy()
        O.add_shadows(img, np.ascontiguousarray(g("shadowed")[0]), p0, n)
    elif call == "lights":
        img, ids = LT.shade_lights(S.cc, *prim, S.lights[:L], g("shadowed")[:L] if flags else None, p0, n, N)
    elif call == "reflect":
        O.shade_reflect(S.cc, S.light, img, *prim[:3], ids, *prim[4:], *geo, *lev, p0, n)
    elif call == "reflect_depth":
        img, ids = REFS[0].shade_depth(S.cc, S.light, *prim, *geo, depth, *lev, p0, n, N)
    elif call in ("reflect_depth_occluded", "reflect_depth_occluded+shadows"):
        occ = np.zeros((DEPTH, N), np.int32) if not flags else g("occluded")[:, 0]
        img, ids = REFS[1].shade_depth_occluded(S.cc, S.light, *prim, *geo, depth, *lev, np.ascontiguousarray(occ), p0, n, N)
        if call.endswith("+shadows"):
            O.add_shadows(img, np.ascontiguousarray(g("shadowed")[0]), p0, n)
    elif call == "reflect_lights":
        img, ids = RL.shade(S.cc, *prim, *geo, depth, *lev, S.lights[:L], g("shadowed")[:L] if flags else None,
                            np.ascontiguousarray(g("occluded")[:depth, :L]) if flags else None, p0, n, N)
    else:
        raise KeyError(call)
    return img, ids, dump


@pytest.fixture(scope="module")
def CHECK(O, REFS, LT, RL):
    """check(call, ...) -> (image, ids, dump) of a checker on the fixture; computed once per argument set and shared."""
    S, memo = synthetic(O), {}

    def check(call, rows=None, depth=DEPTH, L=1, flags=True, **over):
        if over:
            return want(O, REFS, LT, RL, S, call, rows, depth, L, flags, **over)
        key = (call, rows, depth, L, flags)
        if key not in memo:
            memo[key] = want(O, REFS, LT, RL, S, call, rows, depth, L, flags)
            for a in memo[key]:
                if a is not None:
                    a.setflags(write=False)
        return memo[key]

    return check


def model_colour(S, clamp=True, ids=None, t=None):
    """lambertian_shade's colour before the byte conversion, in numpy float32, operation for operation as orc_lambert
    takes them: ([N, 3] colours, which pixels have a material in range, their material).  t is not looked at (the spot
    light shades every pixel with a material)."""
    f = np.float32
    ids = S.ids if ids is None else ids
    idx = np.where(ids >= 0, S.mat_idx[np.maximum(ids, 0)], ids)
    ok = (idx >= 0) & (idx < M)
    kd = S.mat_list[np.where(ok, idx, 0), 3:]
    cc = S.cc
    with np.errstate(all="ignore"):
        point = S.cam_pos[None, :] + (S.t if t is None else t)[:, None] * S.dirs.reshape(-1, 3)
        row = lambda v, k: (cc[16 + k] * v[:, 0] + cc[20 + k] * v[:, 1]) + cc[24 + k] * v[:, 2]
        view = lambda v: np.stack([row(v, k) for k in range(3)], 1)
        norm = lambda v: v * (f(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))[:, None]
        nv = norm(view(S.normal.reshape(-1, 3)))
        ld = norm(view(point) - view(np.broadcast_to(S.light, (N, 3))))
        dot = (ld[:, 0] * nv[:, 0] + ld[:, 1] * nv[:, 1]) + ld[:, 2] * nv[:, 2]
        dot = np.where(dot > 0, dot, dot * f(-1))
        colour = f(0) + kd * f(0.5)
        colour = np.where((dot > 0)[:, None], colour + (kd * f(1.0)) * dot[:, None], colour)
        if clamp:
            colour = np.where(colour > 1, f(1), colour)
    assert colour.dtype == np.float32
    return colour, ok, idx


def to_u8(c):
    with np.errstate(all="ignore"):
        x = c * np.float32(255)
        x = np.where(np.isnan(x) | (x <= 0), 0, np.minimum(x, 4294967295.0))
    return (x.astype(np.uint64) & 0xFF).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ CPU: the inputs

def in_band(rows=MAIN_BAND):
    p0, n = band_of(rows)
    m = np.zeros(N, bool)
    m[p0:p0 + n] = True
    return m


def test_every_class_lies_in_the_band_outside_it_and_in_a_tail_block(O):
    S = synthetic(O)
    band, tail, frame_tail = in_band(), in_band((0, 1)), np.arange(N) >= N - 64
    tail &= np.arange(N) >= TAIL[0]
    print("primary classes %d, chain classes %d, near-integer normals %d, acosf past 1: %d of %d tried" % (
        len(S.primary_names), len(S.chain_names), S.near_integer, S.past_one_found, S.past_one_tried))
    for i, name in enumerate(S.primary_names):
        px = S.primary == i
        print("  %-40s %4d pixels, %3d in the band" % (name, px.sum(), (px & band).sum()))
        if S.undefined[i]:  # the last 9 rows and nowhere else; the frame's tail block is theirs
            assert px[U0:].sum() >= 30 and not px[:U0].any() and (px & frame_tail).any(), name
        else:
            assert (px & band).sum() >= 30 and (px & ~band).sum() >= 30 and (px & tail).any() and not px[U0:].any(), name
    assert (S.primary[U0:] >= 0).all() and S.undefined[S.primary[U0:]].all() and N - U0 == N // 8 == 1224
    for names, which, floor in ((S.chain_names, S.chain, 30), (["flag %d" % v for v in FLAG_VALUES], S.flag_class, 30)):
        for i, name in enumerate(names):
            px = which == i
            print("  %-40s %4d pixels, %3d in the band" % (name, px.sum(), (px & band).sum()))
            assert (px & band).sum() >= floor and (px & ~band).sum() >= floor and (px & tail).any(), name
            assert (px & frame_tail).any() and px[U0:].sum() >= 30, name
    # flags: every value with every light and every level
    for v in FLAG_VALUES:
        assert ((S.shadowed == v).sum(1) >= 100).all() and ((S.occluded == v).sum(2) >= 100).all()
    assert S.near_integer >= 200 and S.past_one_found >= 20
    print("  spot offsets found (ulps from pi/4, x / y):", S.spot_offsets)
    for kind, (ux, uy) in S.spot_offsets.items():
        for u in ((ux,) if kind == "x" else (uy,) if kind == "y" else (ux, uy)):
            # both sides of the face within 2 ulps, and 16 ulps off on both sides
            assert {-2, -1} & set(u) and {0, 1, 2} & set(u) and min(u) <= -16 and max(u) >= 16, (kind, u)


def test_undefined_colours_lie_in_the_last_rows_and_nowhere_else(O, CHECK):
    """The float32 model of lambertian_shade gives the oracle's bytes on every pixel, so its colours are the checker's:
    none outside the last 9 rows is NaN or negative (with t > 0 and without: the spot light looks at no t), and every
    pixel in them has one that is."""
    S = synthetic(O)
    colour, ok, _ = model_colour(S)
    lit = ok & (S.t > 0)
    img = CHECK("simple")[0].reshape(-1, 3)
    np.testing.assert_array_equal(to_u8(np.where(lit[:, None], colour, 0)), img)
    bad = ok & (np.isnan(colour) | (colour < 0)).any(1)
    assert not bad[:U0].any(), class_of(S, np.flatnonzero(bad)[0])
    assert bad[U0:].all()
    # the classes one might expect among them are not: a NaN dot product leaves the ambient term
    for name in ("point on light 0", "normal zero", "normal with a NaN", "normal 1e-30", "t NaN", "t +inf"):
        px = S.primary == S.primary_names.index(name)
        assert px.sum() >= 60 and not bad[px].any() and (colour[px & ok] >= 0).all(), name


def test_saturation_classes_are_what_they_say(O):
    S = synthetic(O)
    raw, ok, idx = model_colour(S, clamp=False)
    px = np.flatnonzero(S.primary == S.primary_names.index("colour below 1, 1, above 1"))
    one = np.float32(1)
    assert (raw[px] == [np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2))]).all()
    px = np.flatnonzero(S.primary == S.primary_names.index("colour * 255 near an integer"))
    c = raw[px, 0].astype(np.float64) * 255.0
    k = np.rint(c)
    ulps = (c - k) / np.spacing(k.astype(np.float32)).astype(np.float64)
    assert px.size >= 200 and (np.abs(ulps) <= 2.5).all() and (ulps < 0).sum() >= 50 and (ulps > 0).sum() >= 50
    assert len(np.unique(k)) >= 100
    # the denormal dot products are denormal, of both signs
    for name, sign in (("normal perpendicular, dot 0", 0), ("normal perpendicular, dot denormal", 1),
                       ("normal perpendicular, dot -denormal", -1)):
        px = S.primary == S.primary_names.index(name)
        n = S.normal.reshape(-1, 3)[px]
        assert (np.sign(n[:, 0]) != 0).sum() == (px.sum() if sign else 0), name


def changed(a, b, px):
    a, b = a.reshape(N, -1), b.reshape(N, -1)
    return int((a[px] != b[px]).any(1).sum()), int(px.sum())


OBSERVED = {}


def observe(what, count, of):
    OBSERVED[what] = (count, of)
    print("%-46s changes %4d of %4d pixels of its class" % (what, count, of))
    assert 2 * count >= of, (what, count, of)


def test_every_guard_is_observable(O, CHECK):
    """Replacing a class's inputs by their tame counterpart changes the checker's bytes on at least half of its pixels."""
    S = synthetic(O)
    prim = lambda name: S.primary == S.primary_names.index(name)
    chn = lambda name: S.chain == S.chain_names.index(name)
    simple, depth8 = CHECK("simple")[0], CHECK("reflect_depth")[0]
    # denormal t -> 0
    px = prim("t denormal")
    observe("denormal t -> 0", *changed(simple, CHECK("simple", t=np.where(px, np.float32(0), S.t))[0], px))
    # active 2 -> 0
    px = chn("active 2")
    act = S.active.reshape(DEPTH, N).copy()
    act[:, px] = 0
    observe("active 2 -> 0", *changed(depth8, CHECK("reflect_depth", active=act.reshape(-1))[0], px))
    # flag 2 -> 1
    px = S.flag_class == 2
    sh = S.shadowed.copy()
    sh[sh == 2] = 1
    observe("flag 2 -> 1", *changed(CHECK("simple+shadows")[0], CHECK("simple+shadows", shadowed=sh)[0], px))
    # out-of-range material -> material 0
    px = np.isin(S.primary, [S.primary_names.index("material %d" % m) for m in BAD_MATERIALS])
    ids = np.where(px, S.tri[("mat", 0)][0], S.ids).astype(np.int32)
    observe("out-of-range material -> material 0", *changed(simple, CHECK("simple", ids=ids)[0], px))
    # kr reset to 0 on a missed level = the level hit black with reflect 0 (material 13)
    px = chn("miss, then active")
    hid = S.hit_id.reshape(DEPTH, N).copy()
    hid[:, px] = np.where(hid[:, px] < 0, S.tri[("mat", 13)][0], hid[:, px])
    observe("kr reset to 0 on a missed level", *changed(depth8, CHECK("reflect_depth", hit_id=hid.reshape(-1))[0], px))
    # chain cut at depth D - 1
    px = chn("chain of full depth")
    observe("chain cut at depth D - 1", *changed(depth8, CHECK("reflect_depth", depth=DEPTH - 1)[0], px))
    # spot point moved 16 ulps or more across the face
    px = np.isin(S.primary, [S.primary_names.index("spot angle at the face, " + k) for k in ("x", "y", "both")])
    moved = S.dirs.reshape(-1, 3).copy()
    moved[px] = S.alt_dirs[px]
    moved = CHECK("spotlight", dirs=moved.reshape(-1))[0]
    observe("spot point moved across +-pi/4", *changed(CHECK("spotlight")[0], moved, px))
    # clamp removed
    px = prim("Kd 3")
    raw, ok, _ = model_colour(S, clamp=False)
    observe("clamp removed", *changed(simple, to_u8(np.where((ok & (S.t > 0))[:, None], raw, 0)), px))
    # ... and the inconsistent chains differ from the consistent ones they would be in a frame
    for name in ("miss, then active", "bad material, then active"):
        px = chn(name)
        act = S.active.reshape(DEPTH, N).copy()
        hid = S.hit_id.reshape(DEPTH, N)
        bad = (hid[:, px] < 0) | ~np.isin(S.mat_idx[np.maximum(hid[:, px], 0)], list(range(M)))
        cut = np.cumsum(np.concatenate([np.zeros((1, bad.shape[1]), bool), bad[:-1]]), 0) > 0
        act[:, px] = np.where(cut, 0, act[:, px])
        observe(name + " -> then inactive", *changed(depth8, CHECK("reflect_depth", active=act.reshape(-1))[0], px))


IDENTITIES = ["depth without an active level = simple", "depth 1 = reflect", "lights, one light = simple + add_shadows",
              "reflect_lights, one light = occluded + add_shadows", "reflect_lights, no flags = depth",
              "reflect_lights without levels = lights", "occluded, all zero = depth"]


def identity_pairs(run, S):
    """{identity: ((image, ids), (image, ids))} from run(call, depth=, L=, flags=, active=)."""
    none = np.zeros(DEPTH * N, np.int32)
    two = lambda a, b: (a[:2], b[:2])
    return {
        IDENTITIES[0]: two(run("reflect_depth", active=none), run("simple")),
        IDENTITIES[1]: two(run("reflect_depth", depth=1), run("reflect")),
        IDENTITIES[2]: two(run("lights", L=1), run("simple+shadows")),
        IDENTITIES[3]: two(run("reflect_lights", L=1), run("reflect_depth_occluded+shadows")),
        IDENTITIES[4]: two(run("reflect_lights", L=1, flags=False), run("reflect_depth")),
        IDENTITIES[5]: two(run("reflect_lights", L=3, active=none), run("lights", L=3)),
        IDENTITIES[6]: two(run("reflect_depth_occluded", flags=False), run("reflect_depth")),
    }


def assert_same(S, a, b, what, px=None):
    for k, name in enumerate(("image", "ids")):
        x, y = a[k].reshape(N, -1), b[k].reshape(N, -1)
        bad = np.flatnonzero((x != y).any(1) & (True if px is None else px))
        assert bad.size == 0, "%s: %s differs on %d pixels, first: %s: %s against %s" % (
            what, name, bad.size, class_of(S, bad[0]), x[bad[0]], y[bad[0]])


@pytest.mark.parametrize("identity", IDENTITIES)
def test_checkers_agree_where_the_header_says_two_calls_are_equal(O, CHECK, identity):
    """Byte for byte and in the ids, on the whole synthetic image, the undefined-cast rows included."""
    S = synthetic(O)
    a, b = identity_pairs(CHECK, S)[identity]
    assert_same(S, a, b, identity)
    assert int((a[0] != 0).sum()) > 5000


# ------------------------------------------------------------------------------------------------ the reference's kernels

RECORD = "shadesyn"
REF_STAGES = ("shade", "spot")


def ref_stage_inputs(O):
    """The fixture as the reference's lambertian_shade + shadow_kernel and spot_shade take it (oracle/ref_kernels.cpp)."""
    S = synthetic(O)
    shade = dict(cc=S.cc, light_pos=S.light, normal=S.normal, t=S.t, dir=S.dirs, id=S.ids, cam_pos=S.cam_pos,
                 mat_idx=S.mat_idx, mat_list=S.mat_list.reshape(-1), W=W, H=H)
    return {"shade": dict(shade, is_shadowed=np.ascontiguousarray(S.shadowed[0])), "spot": shade}


def pinned(stage, out):
    """What of a stage's outputs is compared with the reference's kernels: every pixel in front of the undefined-cast
    rows.  They are left out by their row index: host-compiled C does not define (unsigned char) of a NaN or a negative
    float, the device and ugrt_f2u do (0)."""
    per = dict(image=3, image_unshadowed=3, mat_ids=1, dump=2)
    return {k: np.ascontiguousarray(out[k]).reshape(-1)[:per[k] * U0] for k in RK.STAGE_OUTPUTS[stage]}


def test_oracle_equals_reference_kernels_on_the_fixture(O, CHECK):
    """The record of the reference's kernels against the oracle, always; the live kernels where built.  The record
    leaves out exactly 1/8 of the image."""
    rec = RK.load_record(RECORD)
    ins = ref_stage_inputs(O)
    assert 8 * (N - U0) == N
    img_u, ids, _ = CHECK("simple")
    img = CHECK("simple+shadows")[0]
    spot, spot_ids, dump = CHECK("spotlight")
    outs = {"shade": dict(image_unshadowed=img_u, mat_ids=ids, image=img),
            "spot": dict(image=spot, mat_ids=spot_ids, dump=dump)}
    for stage in REF_STAGES:
        assert RK.input_sha(ins[stage]) == str(rec[stage + "/input_sha"]), \
            "%s: stage inputs differ from the recorded ones (generator or oracle drift)" % stage
        RK.assert_matches_record(rec, RECORD, stage, pinned(stage, outs[stage]), "oracle")
    if O.ref_kernels_live():
        for stage in REF_STAGES:
            got = O.run_ref_kernels(stage, **ins[stage])
            RK.assert_matches_record(rec, RECORD, stage, pinned(stage, got), "reference")


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Device:
    """One context per band with the camera block and the shading light current, and the fixture on the device."""

    def __init__(self, ugrt, S):
        self.u, self.S, self.ctx = ugrt, S, {}
        for name, rows in BANDS.items():
            self.ctx[rows] = c = ugrt.Context(W, H, light_grid=RD.LG, uniform_dims=RD.UD, rows=rows)
            c.upload_camera(S.cc)
            c.set_light_position(S.light)
            assert (c.p0, c.npix) == band_of(rows), name
        up = self.ctx[None].upload
        names = ("normal", "t", "dirs", "cam_pos", "mat_idx", "mat_list", "reflect", "verts", "faces", "rays", "active",
                 "hit_t", "hit_id")
        self.a = {k: up(np.array(getattr(S, k)).reshape(-1)) for k in names}
        self.zero_active = up(np.zeros(DEPTH * N, np.int32))
        self.zero_occluded = up(np.zeros(DEPTH * N, np.int32))
        self.flags = {}

    def shadowed(self, L):
        if ("s", L) not in self.flags:
            self.flags[("s", L)] = self.ctx[None].upload(np.array(self.S.shadowed[:L]).reshape(-1))
        return self.flags[("s", L)]

    def occluded(self, depth, L):
        if L is None:  # one light's, stacked like active
            L, key, arr = 1, ("o", None), self.S.occluded[:, 0]
        else:
            key, arr = ("o", depth, L), self.S.occluded[:depth, :L]
        if key not in self.flags:
            self.flags[key] = self.ctx[None].upload(np.array(arr).reshape(-1))
        return self.flags[key]

    def run(self, call, rows=None, depth=DEPTH, L=1, flags=True, active=None, img=None):
        """(image, ids, dump) on the host; outside the band the sentinels."""
        c, a, t = self.ctx[rows], self.a, self.ctx[None].torch
        full = lambda n, v, dt: t.full((n,), v, dtype=dt, device=c.device)
        d_img = full(3 * N, BYTE, t.uint8) if img is None else c.upload(np.array(img))
        d_ids, d_dump = full(N, ID, t.int32), full(2 * N, float(DUMP), t.float32)
        p0, n = band_of(rows)
        d_ids[p0:p0 + n] = c.upload(np.array(self.S.ids[p0:p0 + n]))
        prim = [d_img, a["normal"], a["t"], a["dirs"], d_ids, a["cam_pos"], a["mat_idx"], a["mat_list"]]
        act = a["active"] if active is None else active
        lev = [a["rays"], act, a["hit_t"], a["hit_id"]]
        geo = [a["reflect"], M, a["verts"], a["faces"]]
        sh = lambda: c.shade_add_shadows(d_img, self.shadowed(1))
        if call in ("simple", "simple+shadows"):
            c.shade_simple(*prim, M)
            if call != "simple":
                sh()
        elif call == "spotlight":
            c.shade_spotlight(*prim, M, d_dump)
        elif call == "add_shadows":
            sh()
        elif call == "lights":
            c.shade_lights(*prim, M, self.S.lights[:L], self.shadowed(L) if flags else None)
        elif call == "reflect":
            c.shade_reflect(*prim, *geo, *lev)
        elif call == "reflect_depth":
            c.shade_reflect_depth(*prim, *geo, depth, *lev)
        elif call in ("reflect_depth_occluded", "reflect_depth_occluded+shadows"):
            occ = self.occluded(DEPTH, None) if flags else self.zero_occluded
            c.shade_reflect_depth_occluded(*prim, *geo, depth, *lev, occ)
            if call.endswith("+shadows"):
                sh()
        elif call == "reflect_lights":
            c.shade_reflect_lights(*prim, *geo, depth, *lev, self.S.lights[:L], self.shadowed(L) if flags else None,
                                   self.occluded(depth, L) if flags else None)
        else:
            raise KeyError(call)
        c.synchronize()
        return d_img.cpu().numpy(), d_ids.cpu().numpy(), d_dump.cpu().numpy()


@pytest.fixture(scope="module")
def DEV(ugrt, O, torch):
    return Device(ugrt, synthetic(O))


def assert_equals_checker(S, got, wanted, rows, what):
    """Inside the band the checker's bytes, ids and dump bits; outside it the sentinels."""
    p0, n = band_of(rows)
    inside = in_band(rows)
    for k, (name, per, sentinel) in enumerate((("image", 3, BYTE), ("ids", 1, ID), ("dump", 2, DUMP))):
        if wanted[k] is None:
            assert k == 2 and (got[k] == sentinel).all(), what + ": the dump is written"
            continue
        view = (lambda a: bits(a)) if name == "dump" else (lambda a: a)
        x, y = view(got[k]).reshape(N, per), view(wanted[k]).reshape(N, per)
        bad = np.flatnonzero((x != y).any(1) & inside)
        assert bad.size == 0, "%s: %s differs from the checker on %d pixels, first: %s: %s, checker %s" % (
            what, name, bad.size, class_of(S, bad[0]), x[bad[0]], y[bad[0]])
        out = got[k].reshape(N, per)[~inside]
        assert (out == sentinel).all(), "%s: %s written outside the band" % (what, name)


ROWS = list(BANDS.values())
ROW_IDS = list(BANDS)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("call", ["simple", "spotlight", "reflect"])
def test_primary_exports_equal_their_checkers(O, CHECK, DEV, call, rows):
    assert_equals_checker(DEV.S, DEV.run(call, rows), CHECK(call, rows), rows, call)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS, ids=ROW_IDS)
def test_add_shadows_equals_its_checker(O, CHECK, DEV, rows):
    """On the simple image and on random bytes: every value of a byte with every flag value."""
    S = DEV.S
    for what, img in (("the simple image", CHECK("simple")[0]),
                      ("random bytes", np.random.default_rng(3).integers(0, 256, 3 * N).astype(np.uint8))):
        wanted = CHECK("add_shadows", rows, img=img)[0]
        got = DEV.run("add_shadows", rows, img=img)[0]
        p0, n = band_of(rows)
        bad = np.flatnonzero((got != wanted).reshape(N, 3).any(1) & in_band(rows))
        assert bad.size == 0, "add_shadows on %s: %d pixels differ, first: %s" % (what, bad.size, class_of(S, bad[0]))
        np.testing.assert_array_equal(got.reshape(N, 3)[~in_band(rows)], img.reshape(N, 3)[~in_band(rows)])


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [True, False], ids=["flags", "no flags"])
@pytest.mark.parametrize("L", [1, 2, 3, 8])
def test_shade_lights_equals_its_checker(O, CHECK, DEV, L, flags):
    for rows in ROWS:
        what = "lights %d, %s" % (L, rows)
        got = DEV.run("lights", rows, L=L, flags=flags)
        assert_equals_checker(DEV.S, got, CHECK("lights", rows, L=L, flags=flags), rows, what)


@pytest.mark.gpu
@pytest.mark.parametrize("call", ["reflect_depth", "reflect_depth_occluded"])
@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8])
def test_depth_exports_equal_their_checkers(O, CHECK, DEV, depth, call):
    for rows in ROWS:
        what = "%s depth %d, %s" % (call, depth, rows)
        assert_equals_checker(DEV.S, DEV.run(call, rows, depth=depth), CHECK(call, rows, depth=depth), rows, what)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [True, False], ids=["flags", "no flags"])
@pytest.mark.parametrize("L", [1, 2, 3, 8])
@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8])
def test_reflect_lights_equals_its_checker(O, CHECK, DEV, depth, L, flags):
    for rows in (None, MAIN_BAND) if (depth, L) != (DEPTH, LIGHTS) else ROWS:
        what = "reflect_lights depth %d, lights %d, %s" % (depth, L, rows)
        assert_equals_checker(DEV.S, DEV.run("reflect_lights", rows, depth, L, flags),
                              CHECK("reflect_lights", rows, depth, L, flags), rows, what)


@pytest.mark.gpu
@pytest.mark.parametrize("identity", IDENTITIES)
def test_identities_hold_on_the_device(O, DEV, identity):
    def run(call, depth=DEPTH, L=1, flags=True, active=None):
        return DEV.run(call, None, depth, L, flags, active=None if active is None else DEV.zero_active)

    a, b = identity_pairs(run, DEV.S)[identity]
    assert_same(DEV.S, a, b, identity)


@pytest.mark.gpu
def test_product_equals_reference_record(O, DEV):
    """libugrt.so against the record of the reference's kernels, no oracle in between."""
    rec = RK.load_record(RECORD)
    img_u, ids, _ = DEV.run("simple")
    img = DEV.run("simple+shadows")[0]
    shade = dict(image_unshadowed=img_u, mat_ids=ids, image=img)
    RK.assert_matches_record(rec, RECORD, "shade", pinned("shade", shade), "product")
    spot, ids, dump = DEV.run("spotlight")
    RK.assert_matches_record(rec, RECORD, "spot", pinned("spot", dict(image=spot, mat_ids=ids, dump=dump)), "product")
