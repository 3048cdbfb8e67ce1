"""The six secondary-ray generators on hits of their own: every guard, every branch, the numeric edges of Snell's law.

ugrt_reflect_rays, _reflect_rays_next, _refract_rays, _refract_rays_next, _occlusion_rays and _ao_rays are otherwise fed
the hits of four scenes: t finite and positive, triangles with area, ior 1.5, active 0 or 1, nearly no ray at the critical
angle, none edge-on.  Here one seeded fixture, built with numpy, holds what a scene never does.  It needs no scene, no grid
and no tracing: the generators read only the arrays they are handed.

Image 136 x 72 = 9 792 pixels (38 blocks of PX_THREADS and a tail of 64; 9 tile rows), the four launches of
tests/test_shade_synthetic.py: the frame and the bands (3, 7), (0, 1) and (6, 9).  Every pixel belongs to ONE named class
(CLASS TABLE below), dealt with a seeded permutation as the shading fixture deals its classes: every class has pixels in
the band (3, 7), outside it, in the tail block of band (0, 1) and in eight blocks or more.  One hit per pixel serves the
primary forms ({cam, dir}, t, id) and the level forms ({o, dir}, active, hit_t = t, hit_id = id; o at the coordinate
origin, about 1e3 and about 1e6 from it).

No input lets even a broken kernel read outside an allocation: triangle ids are in [0, F) or -1 or -2, material indices
in [0, M) or one of -1, -2, M, M + 1, and mat_idx, the triangle list, reflect, transmit and ior are handed to the device as
views into the middle of larger tensors whose margins (MARGIN entries on either side) hold valid indices and positive
coefficients: a kernel that dropped `id >= 0` or the range check of the material would write an active ray where the checker
writes zeros.  An inactive pixel of a level form carries an in-range id, a positive t and a reflecting material: only its
active word keeps it out.

Comparison rule (GPU): inside the band the active words are equal and the six ray words are equal bit for bit (-0.0 and
+0.0 are distinct words), except where the checker's float is a NaN: there the kernel's must be a NaN of any payload (the
sign and payload that x86 and gfx950 give a generated NaN are not known to agree).  The number of NaN words whose bits
differ is printed.  Outside the band the sentinels (7.0f and -7) are untouched.  The pixels with a NaN word in the checker's
ray stay below a quarter of the active pixels of every call (asserted on the CPU).

The checkers are the existing restatements: rd_reflect_rays / _next (reflect_depth_ref.c), rf_refract_rays / _next
(refract_ref.c, with a `kind` per pixel), oc_occlusion_rays (occlusion_ref.c), ao_rays (ambient_ref.c), orc_reflect_rays
(the oracle).  A numpy float32 restatement (np_generate) stands beside them: it equals them word for word, and with one
guard or branch flipped it changes words of that guard's class (the CPU test of observability).  A float64 restatement of
the three rules (mirror, Snell, total reflection) bounds the checkers' own rounding on the ordinary classes.

What the spec leaves open and this file pins, all checkers agreeing: t must be > 0 (NaN, -0, +0 and negative t give no
ray; a denormal t gives one; +inf gives a ray with infinite, or where a direction component is 0 NaN, origin words); ids
below 0 and material indices outside [0, M) give no ray; a level pixel is live where active != 0, whatever the word;
reflect and transmit count where `> 0` (NaN, -0 and negatives do not; a denormal and +inf do), transmit wins over reflect;
ior <= 0 or NaN counts as 1, a denormal ior makes 1/ior infinite (total reflection from the front); an edge-on hit (d.n +0,
-0 or NaN) counts as front; k == 0 exactly refracts (k < 0 alone mirrors); a degenerate triangle gives an active ray with
NaN (or infinite, or for a normal whose squares overflow, unmoved) words.

CLASS TABLE (seed 20261021; printed by test_every_class_lies_in_the_band_outside_it_and_in_the_tail_block): 62 classes of
157 or 158 pixels each, 56 to 83 of them in the band (3, 7), one or two in the tail block of band (0, 1), in 35 blocks or
more; 375 triangles, 47 materials.
  ordinary (2 classes)
  t: smallest normal, denormal, +0, -0, negative, -inf, +inf, NaN, +inf with a zero in d (P is NaN in one lane only)
  id: -1, -2, 0, F - 1
  material index: -1, -2, M, M + 1, 0, M - 1
  coefficients: reflect, transmit, transmit over a mirror each over {+0, -0, -0.5, 1.4e-45, 1, 1.5, +inf, NaN}; reflect
    {-0, -0.5, NaN} under glass; ior over the same eight and 0.5 and 1e-40; transmit and reflect, transmit only, reflect
    only, neither
  side and incidence: front, back, edge-on with d.n exactly +0 and exactly -0 (an axis-aligned normal, both windings),
    normal incidence, grazing (d.n = +-1, 4, 64 times 2^-149 and times 2^-23)
  critical angle: ior 2, 1.5, 1.3 from the back, ior 1/2, 1/1.5, 1/1.3 from the front; the 49 adjacent floats of one
    direction component around it.  k == 0 exactly is reached for ior 2, 1.3, 1/2 and 1/1.3 (23, 8, 23 and 8 pixels); for
    ior 1.5 and 1/1.5 float32 has no such direction (critical_directions says why): the values nearest 0 are 6.0e-8 and
    -3.6e-7
  triangles: two equal vertices, three collinear, a cross product of denormals (an infinite normal), one that underflows
    to 0, one that overflows, a normal whose squares overflow (a normal of zeros: the ray leaves P unmoved), a vertex with
    a NaN, slivers, one triangle in both windings
  directions of length 1e-25, 1e-20, 1e-3, 1e3, 1e19, 1e20 (1e-25 and 1e20: the squared length is 0 and inf, u is not finite)
  active words (level forms, occlusion): 0, 2, -1, INT_MIN, 0x100
eps 1e-3 on every launch, 0 and 1 on the frame; occlusion towards the light (3, 4, 5), a light on one pixel's o' bit for bit
(its direction is three +0 words) and the light (+inf, 4, -inf).
NaN rule: the checker's ray holds a NaN on 714 to 737 of 4 080 active pixels of reflect (17.5 to 18.1 %; band (0, 1): 87 of
438, 19.9 %), 1 214 to 1 228 of 7 738 of refract, 948 to 1 227 of 8 528 of occlusion, 948 to 1 106 of 8 686 of ao.
Float64: the checkers deviate from the float64 rules by at most 1.211e-7 in the origin (relative to |o| + t |d|) and
1.398e-6 in the direction (relative to its length), on 2 099 to 3 415 ordinary pixels per call.

Measured on an MI355X: the 51 GPU tests take 3 s together (with the 43 CPU tests 4 s) and all pass; no generator differs
from its checker in an active word or in a word that is not a NaN.  NaN payloads do NOT match: gfx950 generates 0x7fc00000
where x86 generates 0xffc00000, so 1 085 of 3 473 NaN words of reflect, 2 615 of 5 696 of refract, 2 528 of 5 056 of
occlusion and 356 of 4 898 of ao differ from the checker's in the sign bit and in nothing else (every NaN word on either
side, in every launch, is one of these two).  Two kernels of the device differ from each other in the same way (refract
with transmit all zero against reflect: 1 202 of 3 473 NaN words; the compiler is free to form -x and x * y differently in
each), so the identities on the device apply the NaN rule too; the level forms fed with the
primary arrays give the primary forms' words, NaNs included.  The device keeps float32 denormals in t > 0, in d.n and in
the cross product.  Builds of ugrt_bounce.hip with one fault each, GPU tests of this file that fail: `t >= 0` in
d_secondary_ray 25, in k_occlusion_rays 14, in k_ao_rays 6; `active == 1` in d_secondary_ray 13, in k_occlusion_rays 14;
`k <= 0` 13; `front = dn < 0` 13; `+eps` on the refracted origin 12; `ior_m >= 0` 13; -ffp-contract=fast 47.
"""
import functools
import types

import numpy as np
import pytest

import test_lights as TL
import test_reflect_depth as RD
import test_shade_synthetic as SS
from test_ambient import AO  # noqa: F401  (fixtures)
from test_reflect_shadows import REFS  # noqa: F401
from test_refract import RF  # noqa: F401

f = np.float32
W, H = TL.ODD
N = W * H
BANDS, MAIN_BAND, TAIL = SS.BANDS, SS.MAIN_BAND, SS.TAIL
band_of, in_band, deal = SS.band_of, SS.in_band, SS.deal
ROWS, ROW_IDS = list(BANDS.values()), list(BANDS)
PX_THREADS = 256
SEED = 20261021
MARGIN = 8  # entries in front of and behind mat_idx, the triangle list, reflect, transmit and ior on the device
EPS = 1e-3  # the renderer's
OTHER_EPS = (0.0, 1.0)
INT_MIN = -2 ** 31
RAY, ACT = f(7.0), -7  # the sentinels
CAM = np.array([1.5, -2.25, 0.75], f)
MIRROR, FRONT, BACK, TOTAL = 1, 2, 3, 4  # refract_ref.c's kinds
CALLS = ("reflect", "reflect_next", "refract", "refract_next", "occlusion", "ao")
LEVEL = ("reflect_next", "refract_next", "occlusion")
DEN1 = float(f(1e-45))  # the smallest positive denormal
SWEEP = [("+0", 0.0), ("-0", -0.0), ("negative", -0.5), ("denormal", DEN1), ("1", 1.0), ("above 1", 1.5),
         ("+inf", np.inf), ("NaN", np.nan)]
IOR_SWEEP = SWEEP + [("0.5", 0.5), ("1e-40", 1e-40)]  # (1e-40: 1 / ior is infinite)
CRITICAL = [("ior 2, back", "glass 2", False), ("ior 1.5, back", "glass 1.5", False), ("ior 1.3, back", "glass 1.3", False),
            ("ior 1/2, front", "glass 1/2", True), ("ior 1/1.5, front", "glass 1/1.5", True),
            ("ior 1/1.3, front", "glass 1/1.3", True)]
# (name, reflect, transmit, ior)
MATERIALS = ([("mirror", 0.5, 0.0, 1.0), ("glass 1.5", 0.0, 0.7, 1.5), ("glass 2", 0.0, 0.7, 2.0), ("glass 1.3", 0.0, 0.7, 1.3),
              ("glass 1/2", 0.0, 0.7, 0.5), ("glass 1/1.5", 0.0, 0.7, float(f(1) / f(1.5))),
              ("glass 1/1.3", 0.0, 0.7, float(f(1) / f(1.3))), ("both", 0.5, 0.5, 1.5), ("neither", 0.0, 0.0, 1.5)]
             + [("reflect " + n, v, 0.0, 1.5) for n, v in SWEEP] + [("transmit " + n, 0.0, v, 1.5) for n, v in SWEEP]
             + [("transmit %s over a mirror" % n, 0.5, v, 1.5) for n, v in SWEEP]
             + [("reflect %s under glass" % n, v, 0.7, 1.5) for n, v in SWEEP if n in ("-0", "negative", "NaN")]
             + [("ior " + n, 0.0, 0.7, v) for n, v in IOR_SWEEP] + [("last", 0.25, 0.6, 1.5)])
M = len(MATERIALS)
MAT = {m[0]: i for i, m in enumerate(MATERIALS)}
BAD_MATERIALS = (-1, -2, M, M + 1)
# the ordinary pixel's materials: three in four reflect (and two of those transmit as well), one in four is glass alone
SENDS_ON, SENDS_THROUGH = ("mirror", "both", "last"), ("glass 1.5", "glass 2", "glass 1.3", "glass 1/2")
AXIS = ("mirror", "glass 1.5", "glass 2", "glass 1.3", "glass 1/2", "glass 1/1.5", "glass 1/1.3", "both")
ODD_TRIANGLES = ("two equal vertices", "three collinear vertices", "cross product of denormals", "cross product underflows to 0",
                 "cross product overflows", "squares of the normal overflow", "vertex with a NaN", "sliver")
LENGTHS = (1e-25, 1e-20, 1e-3, 1e3, 1e19, 1e20)  # (1 is the ordinary pixel's; 1e-25 and 1e20: the squares reach 0 and inf)
ACTIVE_WORDS = (0, 2, -1, INT_MIN, 0x100)  # (1 is the ordinary pixel's)
GRAZING = [s * k * 2.0 ** e for e in (-149, -23) for k in (1, 4, 64) for s in (1, -1)]  # d.n exactly, in ulps of 0 and of 1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------ float32 in numpy

def np_dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def np_unit(a):
    return a * (f(1) / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]))[:, None]


def np_rays(o, d, t, e1, e2, eps, transmit, reflect, ior, fault=()):
    """d_continue_ray (ugrt_dev.h) in numpy float32, operation for operation, on n hits at once: dict of the mirrored and
    the chosen ray [n, 6], k, dn, front and refract_ref.c's kind.  `fault` names single faults (see np_generate)."""
    with np.errstate(all="ignore"):
        P = o + t[:, None] * d
        nn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        nn = np_unit(nn)
        dn = np_dot(d, nn)
        if "dn denormal flushed" in fault:
            dn = np.where(np.abs(dn) < f(2.0 ** -126), dn * f(0), dn)
        back = dn > 0
        front = ~back if "front = dn < 0" not in fault else dn < 0
        nn = np.where(back[:, None], -nn, nn)
        dn = np.where(back, -dn, dn)
        mirror = np.concatenate([P + f(eps) * nn, d - (f(2) * dn)[:, None] * nn], 1)
        u = np_unit(d)
        c = -np_dot(u, nn)
        i = ior
        ok = i >= 0 if "ior >= 0" in fault else (i == i) | (i != i) if "ior unguarded" in fault else i > 0
        i = np.where(ok, i, f(1))
        eta = np.where(front, f(1) / i, i)
        k = f(1) - (eta * eta) * (f(1) - c * c)
        g = eta * c - np.sqrt(k)
        side = f(eps) if "+eps on the refracted origin" in fault else -f(eps)
        through = np.concatenate([P + side * nn, eta[:, None] * u + g[:, None] * nn], 1)
        total = k <= 0 if "k <= 0" in fault else k < 0
        cmp = lambda x, what: (x >= 0 if what + " >= 0" in fault else (x != 0) | (x != x) if what + " != 0" in fault else x > 0)
        tr, re = cmp(transmit, "transmit"), cmp(reflect, "reflect")
        if "reflect wins" in fault:
            tr = tr & ~re
        out = np.where((tr & ~total)[:, None], through, mirror)
        kind = np.where(tr, np.where(total, TOTAL, np.where(front, FRONT, BACK)), np.where(re, MIRROR, 0))
    return dict(mirror=mirror, out=out, k=k, dn=dn, front=front, kind=kind, c=c, eta=eta, nn=nn)


# ------------------------------------------------------------------------------------------------ the fixture

def critical_directions(ior, front, count=48):
    """[(dx, dz, k)] for the hit of d = (dx, 0, +-dz) on a triangle with the normal (0, 0, 1), refractive index `ior`,
    from the front (dz < 0) or from the back: the adjacent floats of dz 24 either side of the critical angle, for the
    first dx at which k is exactly 0, below 0 and above 0 somewhere among them; ordered by the distance from it.  Where
    no dx gives a zero (ior 1.5: eta * eta is 2.25, 1 - c * c is a multiple of 2^-24 near 4/9, and the two nearest, 7456540
    and 7456541 times 2^-24, give products 1 - 5.9e-8 and 1 + 7.5e-8, neither of which rounds to 1) the first dx serves."""
    eta = float(f(1) / f(ior)) if front else float(f(ior))
    first = None
    for dx in [0.5] + [j / 64.0 for j in range(17, 129)]:
        z = f(dx * np.sqrt(eta * eta - 1.0))
        zs = [z]
        lo = hi = z
        for _ in range(count // 2):
            lo, hi = np.nextafter(lo, f(0)), np.nextafter(hi, f(np.inf))
            zs += [lo, hi]
        zs = np.asarray(zs, f)
        n = len(zs)
        d = np.stack([np.full(n, dx, f), np.zeros(n, f), -zs if front else zs], 1)
        e1, e2 = np.tile(f([2, 0, 0]), (n, 1)), np.tile(f([0, 2, 0]), (n, 1))
        r = np_rays(np.zeros((n, 3), f), d, np.ones(n, f), e1, e2, EPS, np.full(n, 0.7, f), np.zeros(n, f), np.full(n, ior, f))
        assert (r["front"] == front).all()
        k = r["k"]
        assert (k < 0).any() and (k > 0).any()
        cand = [(dx, float(d[j, 2]), float(k[j])) for j in range(n)]
        if (k == 0).any():
            return cand
        first = first or cand
    return first


@functools.lru_cache(maxsize=None)
def synthetic():
    rng = np.random.default_rng(SEED)
    S = types.SimpleNamespace(W=W, H=H, N=N)
    S.cam_pos = CAM.copy()
    S.reflect = f([m[1] for m in MATERIALS])
    S.transmit = f([m[2] for m in MATERIALS])
    S.ior = f([m[3] for m in MATERIALS])
    # -- triangles: 0 is an ordinary mirror, F - 1 an ordinary triangle of the last material
    tris, mats, S.tri = [], [], {}

    def add(key, t9, m):
        S.tri.setdefault(key, []).append(len(tris))
        tris.append(np.asarray(t9, np.float64).reshape(3, 3))
        mats.append(m)

    def ordinary():
        while True:
            v = rng.uniform(-20.0, 20.0, 3) + rng.normal(size=(3, 3)) * np.exp(rng.uniform(np.log(0.1), np.log(10.0)))
            a, b = v[1] - v[0], v[2] - v[0]
            if np.linalg.norm(np.cross(a, b)) > 0.3 * np.linalg.norm(a) * np.linalg.norm(b):
                return v

    for _ in range(6):
        for m in range(M):
            add(("ord", m), ordinary(), m)
    for m in BAD_MATERIALS:
        for _ in range(4):
            add(("ord", m), ordinary(), m)
    for i, name in enumerate(AXIS):  # the normal is (0, 0, 1) exactly, or (0, 0, -1) in the other winding
        c, s = np.array([4.0 * i, -8.0, 2.0]), (2.0, 0.5)[i % 2]
        add(("axis", name, 1), [c, c + [s, 0, 0], c + [0, s, 0]], MAT[name])
        add(("axis", name, -1), [c, c + [0, s, 0], c + [s, 0, 0]], MAT[name])
    for i in range(6):
        m = MAT[("mirror", "glass 1.5", "both")[i % 3]]
        v = ordinary()
        add("two equal vertices", [v[0], v[0], v[2]] if i % 2 else [v[0], v[1], v[0]], m)
        add("three collinear vertices", [v[0], v[0] + [0.5, 0, 0], v[0] + [2.0, 0, 0]], m)  # (dyadic steps along one axis)
        add("cross product of denormals", rng.normal(size=(3, 3)) * 1e-20, m)
        add("cross product underflows to 0", rng.normal(size=(3, 3)) * 1e-25, m)
        add("cross product overflows", rng.normal(size=(3, 3)) * 1e20, m)
        add("squares of the normal overflow", rng.normal(size=(3, 3)) * 1e12, m)
        w = v.copy()
        w[rng.integers(0, 3), rng.integers(0, 3)] = np.nan
        add("vertex with a NaN", w, m)
        e, q = unit(rng.normal(size=3)), unit(rng.normal(size=3))
        add("sliver", [v[0], v[0] + 100.0 * e, v[0] + 50.0 * e + 1e-4 * q], m)
        v = ordinary()
        add(("winding", 1), v, MAT["glass 1.5"])
        add(("winding", -1), [v[0], v[2], v[1]], MAT["glass 1.5"])
    add(("ord", M - 1), ordinary(), M - 1)
    S.verts = np.ascontiguousarray(np.asarray(tris).reshape(-1), f)
    v = S.verts.reshape(-1, 3, 3)
    for k in S.tri["three collinear vertices"]:  # (collinear after the rounding too)
        v[k, 1], v[k, 2] = v[k, 0] + f([0.5, 0, 0]), v[k, 0] + f([2, 0, 0])
    S.F = F = len(tris)
    S.faces = np.arange(3 * F, dtype=np.int32)
    S.mat_idx = np.asarray(mats, np.int64).astype(np.int32)
    assert S.mat_idx[0] == MAT["mirror"] and S.mat_idx[F - 1] == M - 1
    # -- the larger arrays the device gets views of
    filler = np.full(MARGIN, MAT["both"], np.int32)
    S.big = dict(mat_idx=np.concatenate([filler, S.mat_idx, filler]),
                 faces=np.concatenate([np.tile(np.int32([0, 1, 2]), MARGIN), S.faces, np.tile(np.int32([0, 1, 2]), MARGIN)]),
                 reflect=np.concatenate([np.full(MARGIN, 0.5, f), S.reflect, np.full(MARGIN, 0.5, f)]),
                 transmit=np.concatenate([np.full(MARGIN, 0.5, f), S.transmit, np.full(MARGIN, 0.5, f)]),
                 ior=np.concatenate([np.full(MARGIN, 1.5, f), S.ior, np.full(MARGIN, 1.5, f)]))
    of = lambda key, n: rng.choice(S.tri[key], n)
    mat_tris = lambda names: np.concatenate([S.tri[("ord", MAT[n])] for n in names])

    # -- the ordinary pixel: a unit direction, t of 0.5 to 50, a triangle whose material sends a ray on
    t = rng.uniform(0.5, 50.0, N)
    d = unit(rng.normal(size=(N, 3)))
    ids = np.where(rng.integers(0, 4, N) > 0, rng.choice(mat_tris(SENDS_ON), N), rng.choice(mat_tris(SENDS_THROUGH), N))
    ids = ids.astype(np.int64)
    S.origin_scale = rng.choice([0.0, 1e3, 1e6], N)
    org = rng.uniform(-1.0, 1.0, (N, 3)) * S.origin_scale[:, None]
    active = np.ones(N, np.int64)
    classes = []

    def cls(name):
        def reg(fn):
            classes.append((name, fn))
            return fn
        return reg

    cls("ordinary")(lambda px: None)
    cls("ordinary 2")(lambda px: None)
    # 1. t
    for name, val in (("t smallest normal", float(np.finfo(f).tiny)), ("t denormal", 1e-40), ("t +0", 0.0), ("t -0", -0.0),
                      ("t -inf", -np.inf), ("t +inf", np.inf), ("t NaN", np.nan)):
        cls(name)(lambda px, val=val: t.__setitem__(px, val))

    @cls("t negative")
    def _(px):
        t[px] = -t[px]

    @cls("t +inf, a zero in d")
    def _(px):
        t[px] = np.inf
        d[px, np.arange(px.size) % 3] = np.where(np.arange(px.size) % 2, 0.0, -0.0)

    # 2. ids
    for name, val in (("id -1", -1), ("id -2", -2), ("id 0", 0), ("id F - 1", F - 1)):
        cls(name)(lambda px, val=val: ids.__setitem__(px, val))
    # 3. material indices
    for m in BAD_MATERIALS + (0, M - 1):
        cls("material index %d" % m)(lambda px, m=m: ids.__setitem__(px, of(("ord", m), px.size)))
    # 4. coefficients
    S.sweep = {}

    def sweep(name, names):
        def _(px):
            which = np.arange(px.size) % len(names)
            S.sweep[name] = (px, which, names)
            ids[px] = [of(("ord", MAT[names[w]]), 1)[0] for w in which]
        cls(name)(_)

    sweep("reflect sweep", ["reflect " + n for n, _ in SWEEP])
    sweep("transmit sweep", ["transmit " + n for n, _ in SWEEP])
    sweep("transmit sweep over a mirror", ["transmit %s over a mirror" % n for n, _ in SWEEP])
    sweep("reflect -0, negative, NaN under glass", ["reflect %s under glass" % n for n in ("-0", "negative", "NaN")])
    sweep("ior sweep", ["ior " + n for n, _ in IOR_SWEEP])
    for name, m in (("transmit and reflect", "both"), ("transmit only", "glass 1.5"), ("reflect only", "mirror"),
                    ("neither transmit nor reflect", "neither")):
        cls(name)(lambda px, m=m: ids.__setitem__(px, of(("ord", MAT[m]), px.size)))

    # 5. side and incidence
    def face_normals(idx):
        v = S.verts.reshape(-1, 3, 3)[idx].astype(np.float64)
        return unit(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))

    for name, sign in (("front", -1.0), ("back", 1.0)):
        def _(px, sign=sign):
            ids[px] = rng.choice(mat_tris(("glass 1.5", "glass 2", "glass 1/2", "mirror")), px.size)
            n = face_normals(ids[px])
            c = rng.uniform(0.1, 1.0, px.size)  # |cos| of the incidence
            side = unit(np.cross(n, rng.normal(size=(px.size, 3))))
            d[px] = sign * c[:, None] * n + np.sqrt(1 - c * c)[:, None] * side
        cls(name)(_)

    def axis_tri(px, names, winding=None):
        i = np.arange(px.size)
        w = np.where(i % 2, 1, -1) if winding is None else np.full(px.size, winding)
        m = [names[(j // 2) % len(names)] for j in i]
        ids[px] = [S.tri[("axis", m[j], int(w[j]))][0] for j in i]
        return w

    @cls("edge-on, d.n +0")
    def _(px):
        w = axis_tri(px, ("mirror", "glass 1.5", "glass 1/2"))
        i = np.arange(px.size)
        d[px] = unit(np.stack([rng.uniform(0.2, 1.0, px.size), rng.uniform(0.2, 1.0, px.size) * np.where(i % 3, 1, -1),
                               np.zeros(px.size)], 1))
        d[px, 2] = np.where(i % 4 < 2, 0.0, -0.0) * w  # (+0 + +-0 = +0 whatever the winding)

    @cls("edge-on, d.n -0")
    def _(px):
        w = axis_tri(px, ("mirror", "glass 1.5", "glass 1/2"))
        d[px] = unit(np.stack([-rng.uniform(0.2, 1.0, px.size), -rng.uniform(0.2, 1.0, px.size), np.zeros(px.size)], 1))
        d[px, 2] = -0.0 * w  # every product is -0: (0, 0, 1) with dz -0, (0, 0, -1) with dz +0

    @cls("normal incidence")
    def _(px):
        axis_tri(px, ("mirror", "glass 1.5", "glass 2", "glass 1/2"))
        i = np.arange(px.size)
        d[px] = 0.0
        d[px, 2] = np.where((i // 8) % 2, 1.0, -1.0) * np.choose(i % 3, [1.0, 0.5, 3.0])

    @cls("grazing")
    def _(px):
        axis_tri(px, ("mirror", "glass 1.5", "glass 1/2"), winding=1)
        i = np.arange(px.size)
        a = rng.uniform(0.0, 2 * np.pi, px.size)
        d[px] = np.stack([np.cos(a), np.sin(a), np.asarray(GRAZING)[(i // 6) % len(GRAZING)]], 1)

    # 6. the critical angle
    S.critical = {}
    for name, material, front in CRITICAL:
        def _(px, name=name, material=material, front=front):
            cand = critical_directions(MATERIALS[MAT[material]][3], front)
            S.critical[name] = (px, cand)
            ids[px] = S.tri[("axis", material, 1)][0]
            j = np.arange(px.size) % len(cand)
            d[px] = [(cand[q][0], 0.0, cand[q][1]) for q in j]
        cls("critical angle, " + name)(_)
    # 7. triangles
    for name in ODD_TRIANGLES:
        cls(name)(lambda px, name=name: ids.__setitem__(px, of(name, px.size)))

    @cls("one triangle in both windings")
    def _(px):
        i = np.arange(px.size)
        pair = (i // 2) % len(S.tri[("winding", 1)])
        ids[px] = np.where(i % 2, np.asarray(S.tri[("winding", -1)])[pair], np.asarray(S.tri[("winding", 1)])[pair])
        d[px] = d[px[(i // 2) * 2]]  # the two of a pair share the direction, t and the origin
        t[px] = t[px[(i // 2) * 2]]
        org[px] = org[px[(i // 2) * 2]]

    # 8. directions
    for length in LENGTHS:
        def _(px, length=length):
            d[px] *= length
            t[px] /= max(length, 1e-3)  # (the hit stays within reach)
            ids[px] = rng.choice(mat_tris(("mirror", "glass 1.5", "glass 1/2", "both")), px.size)
        cls("direction of length %g" % length)(_)
    # 9. active words
    for word in ACTIVE_WORDS:
        cls("active %s" % ("0x100" if word == 0x100 else "INT_MIN" if word == INT_MIN else word))(
            lambda px, word=word: active.__setitem__(px, word))

    S.names = [c[0] for c in classes]
    S.cls = deal(rng, S.names, 0, N, TAIL)
    for i, (_, fn) in enumerate(classes):
        fn(np.flatnonzero(S.cls == i))
    S.t = t.astype(f)
    S.dirs = np.ascontiguousarray(d.astype(f).reshape(-1))
    S.ids = ids.astype(np.int32)
    S.rays = np.ascontiguousarray(np.concatenate([org, d], 1).astype(f).reshape(-1))
    S.active = active.astype(np.int32)
    S.hit_t, S.hit_id = S.t, S.ids
    assert ((S.ids >= -2) & (S.ids < F)).all()
    assert np.isin(S.mat_idx, np.concatenate([np.arange(M), BAD_MATERIALS])).all()
    S.lights = {"the light": f([3.0, 4.0, 5.0]), "a light with infinite coordinates": f([np.inf, 4.0, -np.inf])}
    for a in (S.t, S.dirs, S.ids, S.rays, S.active, S.verts, S.faces, S.mat_idx, S.reflect, S.transmit, S.ior, S.cam_pos):
        a.setflags(write=False)
    return S


def px_of(S, name):
    return S.cls == S.names.index(name)


def class_of(S, p):
    return "pixel %d (row %d): %s" % (p, p // W, S.names[S.cls[p]])


def light_on_a_pixel(S, OC):
    """(the light, the pixel): o' of an ordinary live pixel of tile row 6 (in the frame, in band 3..6 and in band 6..8)."""
    rays, act = OC.occlusion_rays(S.rays, S.active, S.hit_t, S.hit_id, S.verts, S.faces, S.lights["the light"], EPS, 0, N, N)
    p = np.flatnonzero(px_of(S, "ordinary") & (act == 1) & in_band((6, 7)))[0]
    return rays.reshape(N, 6)[p, :3].copy(), p


def light_of(S, REFS, light):
    return light_on_a_pixel(S, REFS[1])[0] if light == "a light on a pixel's origin" else S.lights[light]


# ------------------------------------------------------------------------------------------------ the checkers

def want(O, REFS, RF, AO, S, call, rows=None, eps=EPS, light="the light", **over):
    """(rays, active, kind or None) of the checker of `call` on the fixture (or on `over` in an array's place); outside
    the band zeros."""
    REF, OC = REFS
    p0, n = band_of(rows)
    g = lambda k: over.get(k, getattr(S, k, None))
    prim = (g("cam_pos"), g("t"), g("dirs"), g("ids"))
    lev = (g("rays"), g("active"), g("hit_t"), g("hit_id"))
    geo = (S.verts, S.faces, eps, p0, n, N)
    if call == "reflect":
        return REF.reflect_rays(*prim, S.mat_idx, g("reflect"), *geo) + (None,)
    if call == "reflect_next":
        return REF.reflect_rays_next(*lev, S.mat_idx, g("reflect"), *geo) + (None,)
    if call == "refract":
        return RF.refract_rays(*prim, S.mat_idx, g("reflect"), g("transmit"), g("ior"), *geo)
    if call == "refract_next":
        return RF.refract_rays_next(*lev, S.mat_idx, g("reflect"), g("transmit"), g("ior"), *geo)
    if call == "occlusion":
        return OC.occlusion_rays(*lev, S.verts, S.faces, light_of(S, REFS, light), eps, p0, n, N) + (None,)
    if call == "ao":
        return AO.rays(*prim, *geo) + (None,)
    if call == "oracle":
        return O.reflect_rays(*prim, S.mat_idx, g("reflect"), *geo) + (None,)
    raise KeyError(call)


@pytest.fixture(scope="module")
def CHECK(O, REFS, RF, AO):
    """check(call, rows, eps, light) -> (rays, active, kind) of a checker on the fixture; computed once per argument set
    and shared, read-only."""
    S, memo = synthetic(), {}

    def check(call, rows=None, eps=EPS, light="the light", **over):
        if over:
            return want(O, REFS, RF, AO, S, call, rows, eps, light, **over)
        key = (call, rows, eps, light)
        if key not in memo:
            memo[key] = want(O, REFS, RF, AO, S, call, rows, eps, light)
            for a in memo[key]:
                if a is not None:
                    a.setflags(write=False)
        return memo[key]

    return check


def np_generate(S, call, eps=EPS, light=None, fault=(), t=None):
    """The generator `call` in numpy float32 on the whole frame, reading what a kernel reads: the larger arrays at the
    offset MARGIN.  (rays [N * 6], active [N], details).  `fault` is a set of single faults:
      "t >= 0", "t not <= 0", "t != 0"           in place of t > 0
      "active == 1", "active > 0", "active low byte"   in place of active != 0
      "id unguarded", "material below 0 unguarded", "material above M - 1 unguarded"
      "reflect >= 0", "reflect != 0", "transmit >= 0", "transmit != 0"   in place of > 0;   "reflect wins"
      "ior >= 0", "ior unguarded"                in place of ior > 0
      "front = dn < 0", "k <= 0", "+eps on the refracted origin", "dn denormal flushed"
    """
    B = S.big
    level, glass = call in LEVEL, call.startswith("refract")
    tt = S.t if t is None else t
    if level:
        r = S.rays.reshape(N, 6)
        o, d, a = r[:, :3], r[:, 3:], S.active
        live = (a == 1 if "active == 1" in fault else a > 0 if "active > 0" in fault else
                (a & 0xFF) != 0 if "active low byte" in fault else a != 0)
    else:
        o, d, live = np.broadcast_to(S.cam_pos, (N, 3)), S.dirs.reshape(N, 3), np.ones(N, bool)
    with np.errstate(all="ignore"):
        hit = (tt >= 0 if "t >= 0" in fault else ~(tt <= 0) if "t not <= 0" in fault else tt != 0 if "t != 0" in fault
               else tt > 0)
    ids = S.ids
    goes = live & hit & ((ids >= 0) | ("id unguarded" in fault))
    m = B["mat_idx"][MARGIN + ids]
    in_range = ((m >= 0) | ("material below 0 unguarded" in fault)) & ((m < M) | ("material above M - 1 unguarded" in fault))
    mm = MARGIN + np.clip(m, -MARGIN, M + MARGIN - 1)
    re, tr, ior = B["reflect"][mm], B["transmit"][mm], B["ior"][mm]
    if not glass:
        tr = np.zeros(N, f)
    if call in ("occlusion", "ao"):
        re, in_range = np.ones(N, f), np.ones(N, bool)
    v = S.verts.reshape(-1, 3)[B["faces"].reshape(-1, 3)[MARGIN + ids]]
    R = np_rays(o, d, tt, v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], eps, tr, re, ior, fault)
    goes = goes & in_range & (R["kind"] != 0)
    out = R["out"].copy()
    with np.errstate(all="ignore"):
        if call == "occlusion":
            out[:, 3:] = f(light)[None, :] - out[:, :3]
        if call == "ao":
            out[:, 3:] = R["nn"]
    out = np.where(goes[:, None], out, f(0))
    R["kind"] = np.where(goes, R["kind"], 0)
    return np.ascontiguousarray(out.reshape(-1)), goes.astype(np.int32), R


def ao_normals(S):
    """The unit normal per pixel turned against the primary direction, as np_rays forms it."""
    return np_generate(S, "ao")[2]["nn"]


def compare(S, got, wanted, rows, what, log=print):
    """The comparison rule of the module's docstring: (pixels on which the NaN rule was applied, NaN words whose bits
    differ).  got: (rays, active) with the sentinels outside the band."""
    inside = in_band(rows)
    g_act, w_act = np.asarray(got[1]), np.asarray(wanted[1])
    bad = np.flatnonzero((g_act != w_act) & inside)
    assert bad.size == 0, "%s: active differs from the checker on %d pixels, first: %s: %d, checker %d" % (
        what, bad.size, class_of(S, bad[0]), g_act[bad[0]], w_act[bad[0]])
    gf, wf = np.asarray(got[0], f).reshape(N, 6), np.asarray(wanted[0], f).reshape(N, 6)
    gb, wb = bits(gf).reshape(N, 6), bits(wf).reshape(N, 6)
    nan = np.isnan(wf)
    wrong = np.where(nan, ~np.isnan(gf), gb != wb)
    bad = np.flatnonzero(wrong.any(1) & inside)
    assert bad.size == 0, "%s: rays differ from the checker on %d pixels, first: %s: %s, checker %s" % (
        what, bad.size, class_of(S, bad[0]), gf[bad[0]], wf[bad[0]])
    assert (gf[~inside] == RAY).all() and (g_act[~inside] == ACT).all(), what + ": written outside the band"
    nan_px = int((nan.any(1) & inside).sum())
    payload = int((nan & (gb != wb) & inside[:, None]).sum())
    live = int((w_act[inside] != 0).sum())
    log("%-46s %5d active, NaN rule on %4d pixels, %5d NaN words of %5d differ in their bits" % (
        what, live, nan_px, payload, int((nan & inside[:, None]).sum())))
    odd = np.flatnonzero((nan & (gb != wb)).any(1) & inside)
    if odd.size:
        log("    first: %s: %s, checker %s" % (class_of(S, odd[0]), [hex(w) for w in gb[odd[0]]], [hex(w) for w in wb[odd[0]]]))
        log("    the NaN words: %s, the checker's %s" % tuple(
            sorted(hex(w) for w in np.unique(x[nan & inside[:, None]])) for x in (gb, wb)))
    assert 4 * nan_px < live, (what, nan_px, live)
    return nan_px, payload


def with_sentinels(rays, active, rows):
    inside = in_band(rows)
    return np.where(np.repeat(inside, 6), rays, RAY).astype(f), np.where(inside, active, ACT).astype(np.int32)


# ------------------------------------------------------------------------------------------------ CPU: the inputs

def test_every_class_lies_in_the_band_outside_it_and_in_the_tail_block():
    S = synthetic()
    band, tail = in_band(), in_band((0, 1)) & (np.arange(N) >= TAIL[0])
    assert TAIL == (1024, 1088) and N == 38 * PX_THREADS + 64
    print("%d classes, %d triangles, %d materials" % (len(S.names), S.F, M))
    for i, name in enumerate(S.names):
        px = S.cls == i
        blocks = np.unique(np.flatnonzero(px) // PX_THREADS)
        print("  %-44s %4d pixels, %3d in the band, %2d blocks" % (name, px.sum(), (px & band).sum(), blocks.size))
        assert (px & band).sum() >= 30 and (px & ~band).sum() >= 30 and (px & tail).any() and blocks.size >= 8, name
        assert len(np.unique(S.origin_scale[px])) == 3, name  # level origins at 0, 1e3 and 1e6
    # every value of a sweep, of the grazing offsets and of the critical candidates lies in the band and outside it
    for name, (px, which, names) in S.sweep.items():
        for w in range(len(names)):
            assert band[px[which == w]].any() and (~band[px[which == w]]).any(), (name, names[w])
    assert (S.cls >= 0).all()


def test_guard_and_edge_classes_are_what_they_say():
    S = synthetic()
    _, _, R = np_generate(S, "refract")
    dnb = bits(R["dn"])
    assert (dnb[px_of(S, "edge-on, d.n +0")] == 0).all() and (dnb[px_of(S, "edge-on, d.n -0")] == 0x80000000).all()
    px = px_of(S, "grazing")
    assert set(np.unique(R["dn"][px].astype(np.float64))) == {-abs(g) for g in GRAZING}  # exactly, turned against d
    assert set(np.unique(S.dirs.reshape(N, 3)[px, 2].astype(np.float64))) == set(GRAZING)
    px = px_of(S, "normal incidence")
    assert (R["c"][px] == 1).all() and (R["k"][px] == 1).all() and R["front"][px].any() and (~R["front"][px]).any()
    assert R["front"][px_of(S, "front")].all() and not R["front"][px_of(S, "back")].any()
    # +inf times a zero: NaN in one lane of P, infinities in the others
    rays = np_generate(S, "refract")[0].reshape(N, 6)
    px = px_of(S, "t +inf, a zero in d")
    assert (np.isnan(rays[px, :3]).sum(1) == 1).all() and (np.isinf(rays[px, :3]).sum(1) == 2).all()
    px = px_of(S, "t +inf")
    assert np.isinf(rays[px, :3]).all() and np.isfinite(rays[px, 3:]).all()
    # the odd triangles: NaN normals, infinite ones, and normals of zeros
    nn = ao_normals(S)
    for name, test in (("two equal vertices", np.isnan), ("three collinear vertices", np.isnan),
                       ("cross product underflows to 0", np.isnan), ("vertex with a NaN", np.isnan),
                       ("cross product overflows", np.isnan), ("cross product of denormals", lambda x: ~np.isfinite(x)),
                       ("squares of the normal overflow", lambda x: x == 0)):
        px = px_of(S, name)
        assert test(nn[px]).any(1).all(), name
    v = S.verts.reshape(-1, 3, 3)[S.tri["cross product of denormals"]]
    with np.errstate(all="ignore"):
        cr = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    assert (np.abs(cr[cr != 0]) < np.finfo(f).tiny).all() and (cr != 0).any()
    assert np.isfinite(nn[px_of(S, "sliver")]).all()
    # directions: the squares underflow to denormals and to 0, overflow at 1e20
    dd = S.dirs.reshape(N, 3)
    with np.errstate(all="ignore"):
        sq = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    assert (sq[px_of(S, "direction of length 1e-25")] == 0).all() and np.isinf(sq[px_of(S, "direction of length 1e+20")]).all()
    px = px_of(S, "direction of length 1e-20")
    assert ((sq[px] > 0) & (sq[px] < np.finfo(f).tiny)).all()
    assert np.isfinite(sq[px_of(S, "direction of length 1e+19")]).all()
    # an inactive pixel of a level form has everything else a ray needs
    px = px_of(S, "active 0")
    assert (np_generate(S, "ao")[1][px] == 1).all() and (np_generate(S, "refract")[1][px] == 1).all()
    assert not np_generate(S, "refract_next")[1][px].any()
    assert not np_generate(S, "occlusion", light=S.lights["the light"])[1][px].any()


def test_critical_angle_classes_hold_k_zero_and_its_neighbours(CHECK):
    S = synthetic()
    kind = CHECK("refract")[2]
    _, _, R = np_generate(S, "refract")
    zeros = 0
    for name, material, front in CRITICAL:
        px, cand = S.critical[name]
        k = R["k"][px]
        np.testing.assert_array_equal(k, f([cand[j % len(cand)][2] for j in range(px.size)]))
        has_zero = any(c[2] == 0 for c in cand)
        zeros += has_zero
        for where in (in_band()[px], ~in_band()[px]):
            assert (k[where] == 0).any() == has_zero and (k[where] < 0).any() and (k[where] > 0).any(), name
        print("%-18s k == 0 on %3d pixels, < 0 on %3d, > 0 on %3d; the values nearest 0: %s" % (
            name, (k == 0).sum(), (k < 0).sum(), (k > 0).sum(), sorted(set(k.tolist()), key=abs)[:5]))
        assert (R["front"][px] == front).all()
        assert (kind[px][k < 0] == TOTAL).all() and (kind[px][~(k < 0)] == (FRONT if front else BACK)).all(), name
    print("k == 0 exactly is reached on %d of the %d materials" % (zeros, len(CRITICAL)))
    assert zeros >= 3  # (critical_directions says why ior 1.5 has none)


def test_kinds_reach_all_four_values_and_every_class_has_its_kind(CHECK):
    S = synthetic()
    for call in ("refract", "refract_next"):
        kind = CHECK(call)[2]
        assert set(np.unique(kind)) == {0, MIRROR, FRONT, BACK, TOTAL}
        live = np.ones(N, bool) if call == "refract" else S.active != 0
        k = lambda name: set(np.unique(kind[px_of(S, name) & live]))
        assert k("reflect only") == {MIRROR} and k("transmit only") <= {FRONT, BACK, TOTAL} and k("transmit and reflect") <= {
            FRONT, BACK, TOTAL} and k("neither transmit nor reflect") == {0}
        for name in ("t +0", "t -0", "t negative", "t -inf", "t NaN", "id -1", "id -2") + tuple(
                "material index %d" % m for m in BAD_MATERIALS):
            assert k(name) == {0}, name
        for name in ("t smallest normal", "t denormal", "t +inf", "id 0", "id F - 1", "material index 0",
                     "material index %d" % (M - 1)) + ODD_TRIANGLES:
            assert 0 not in k(name), name
        assert k("front") <= {FRONT, TOTAL, MIRROR} and k("back") <= {BACK, TOTAL, MIRROR} and TOTAL in k("back")
        assert k("edge-on, d.n +0") == k("edge-on, d.n -0") == {MIRROR, FRONT, TOTAL}  # (glass 1/2 from the front: total)
        # the sweeps, value by value
        glass = {FRONT, BACK, TOTAL}
        expect = {"reflect sweep": lambda v: {MIRROR} if v > 0 else {0}, "transmit sweep": lambda v: glass if v > 0 else {0},
                  "transmit sweep over a mirror": lambda v: glass if v > 0 else {MIRROR},
                  "reflect -0, negative, NaN under glass": lambda v: glass, "ior sweep": lambda v: glass}
        for name, (px, which, names) in S.sweep.items():
            for w, mname in enumerate(names):
                m = MATERIALS[MAT[mname]]
                v = m[3] if name == "ior sweep" else m[2] if name.startswith("transmit") else m[1]
                p = px[which == w]
                p = p[live[p]]
                got = set(np.unique(kind[p]))
                assert got and got <= expect[name](v), (call, mname, got)
        if call == "refract_next":
            for word in ACTIVE_WORDS:
                name = "active %s" % ("0x100" if word == 0x100 else "INT_MIN" if word == INT_MIN else word)
                assert (0 in set(np.unique(kind[px_of(S, name)]))) == (word == 0), name


def test_numpy_restatement_equals_every_checker(CHECK):
    """np_generate without a fault gives the checkers' words: so what a fault changes in it, it changes against them."""
    S = synthetic()
    for call in CALLS:
        for eps in (EPS,) + OTHER_EPS:
            rays, act, _ = np_generate(S, call, eps, S.lights["the light"])
            w = CHECK(call, None, eps)
            compare(S, with_sentinels(rays, act, None), w, None, "numpy, %s eps %g" % (call, eps))


def test_nan_share_of_the_checkers_stays_below_a_quarter(CHECK):
    S = synthetic()
    for call in CALLS:
        for rows in ROWS:
            for eps in (EPS,) + (OTHER_EPS if rows is None else ()):
                for light in (("the light", "a light on a pixel's origin", "a light with infinite coordinates")
                              if call == "occlusion" else ("the light",)):
                    rays, act, _ = CHECK(call, rows, eps, light)
                    inside = in_band(rows)
                    nan = np.isnan(rays.reshape(N, 6)).any(1) & inside
                    live = int((act[inside] != 0).sum())
                    print("%-12s %-10s eps %-5g %-34s NaN on %4d of %5d active pixels" % (
                        call, rows, eps, light, nan.sum(), live))
                    assert live >= 300 and 4 * nan.sum() < live and not nan[act == 0].any()
                    assert not rays.reshape(N, 6)[act == 0].any()
                    assert not rays.reshape(N, 6)[~inside].any() and set(np.unique(act)) <= {0, 1}


FAULTS = [
    # (fault, call, classes whose words it must change)
    ("t >= 0", "reflect", ("t +0", "t -0")), ("t not <= 0", "refract", ("t NaN",)), ("t != 0", "ao", ("t negative", "t -inf")),
    ("t >= 0", "occlusion", ("t +0", "t -0")),
    ("active == 1", "reflect_next", ("active 2", "active -1", "active INT_MIN", "active 0x100")),
    ("active == 1", "occlusion", ("active 2", "active -1", "active INT_MIN", "active 0x100")),
    ("active > 0", "refract_next", ("active -1", "active INT_MIN")), ("active low byte", "refract_next", ("active 0x100",)),
    ("id unguarded", "reflect", ("id -1", "id -2")), ("id unguarded", "ao", ("id -1", "id -2")),
    ("id unguarded", "occlusion", ("id -1", "id -2")),
    ("material below 0 unguarded", "refract", ("material index -1", "material index -2")),
    ("material above M - 1 unguarded", "reflect_next", ("material index %d" % M, "material index %d" % (M + 1))),
    ("reflect >= 0", "reflect", ("reflect sweep",)), ("reflect != 0", "refract", ("reflect sweep",)),
    ("transmit >= 0", "refract", ("transmit sweep", "transmit sweep over a mirror")),
    ("transmit != 0", "refract_next", ("transmit sweep", "transmit sweep over a mirror")),
    ("reflect wins", "refract", ("transmit and reflect",)),
    ("ior >= 0", "refract", ("ior sweep",)), ("ior unguarded", "refract_next", ("ior sweep",)),
    ("front = dn < 0", "refract", ("edge-on, d.n +0", "edge-on, d.n -0")),
    ("k <= 0", "refract", tuple("critical angle, " + c[0] for c in CRITICAL if "1.5" not in c[0])),  # (1.5 has no k == 0)
    ("k <= 0", "refract_next", tuple("critical angle, " + c[0] for c in CRITICAL if "1.5" not in c[0])),
    ("+eps on the refracted origin", "refract", ("transmit only", "front", "back")),
    ("dn denormal flushed", "refract", ("grazing",)), ("dn denormal flushed", "ao", ("grazing",)),
]


@pytest.mark.parametrize("fault,call,names", FAULTS, ids=["%s in %s" % x[:2] for x in FAULTS])
def test_every_guard_and_branch_is_observable(CHECK, fault, call, names):
    """One guard or branch flipped in the numpy restatement changes a word of a pixel of each of its classes, in the
    band (3, 7) and outside it."""
    S = synthetic()
    a = np_generate(S, call, EPS, S.lights["the light"])
    b = np_generate(S, call, EPS, S.lights["the light"], fault={fault})
    differ = (bits(a[0]).reshape(N, 6) != bits(b[0]).reshape(N, 6)).any(1) | (a[1] != b[1])
    for name in names:
        px = px_of(S, name)
        print("%-34s in %-12s changes %3d of %3d pixels of %s" % (fault, call, (differ & px).sum(), px.sum(), name))
        assert (differ & px & in_band()).any() and (differ & px & ~in_band()).any(), name


def test_a_flushed_denormal_t_is_observable(CHECK):
    S = synthetic()
    px = px_of(S, "t denormal")
    for call in CALLS:
        act = np_generate(S, call, light=S.lights["the light"], t=np.where(px, f(0), S.t))[1]
        assert (CHECK(call)[1][px] == 1).sum() >= 60 and not act[px].any(), call


def same_words(S, a, b, what, px=None, nan_rule=False):
    """a and b, (rays, active) each, are equal word for word on the pixels px; with nan_rule a NaN on one side asks for
    a NaN of any payload on the other (two kernels of one device: the compiler is free to form -x, x * y and y * x
    differently in each, which shows in a NaN's sign and in nothing else).  Returns the number of pixels with a ray."""
    px = np.ones(N, bool) if px is None else px
    fa, fb = np.asarray(a[0], f).reshape(N, -1), np.asarray(b[0], f).reshape(N, -1)
    ra, rb = bits(fa).reshape(fa.shape), bits(fb).reshape(fb.shape)
    wrong = ra != rb
    if nan_rule:
        both = np.isnan(fa) & np.isnan(fb)
        print("%-56s %5d NaN words of %5d differ in their bits" % (
            what, (wrong & both & px[:, None]).sum(), (both & px[:, None]).sum()))
        odd = np.flatnonzero((wrong & both).any(1) & px)
        if odd.size:
            print("    first: %s: %s against %s" % (
                class_of(S, odd[0]), [hex(w) for w in ra[odd[0]]], [hex(w) for w in rb[odd[0]]]))
        wrong &= ~both
    bad = np.flatnonzero((wrong.any(1) | (np.asarray(a[1]) != np.asarray(b[1]))) & px)
    assert bad.size == 0, "%s: %d pixels differ, first: %s: %s against %s (%s against %s)" % (
        what, bad.size, class_of(S, bad[0]), fa[bad[0]], fb[bad[0]], [hex(w) for w in ra[bad[0]]], [hex(w) for w in rb[bad[0]]])
    return int(((np.asarray(a[1]) != 0) & px).sum())


def level_from_primary(S):
    """The level forms' arguments that restate the primary hit: rays = {cam, dir}, active all ones."""
    rays = np.concatenate([np.broadcast_to(S.cam_pos, (N, 3)), S.dirs.reshape(N, 3)], 1).astype(f).reshape(-1)
    return dict(rays=np.ascontiguousarray(rays), active=np.ones(N, np.int32), hit_t=S.t, hit_id=S.ids)


IDENTITIES = ["refract with transmit all zero = reflect", "refract_next with transmit all zero = reflect_next",
              "reflect_next of {cam, dir}, all live = reflect", "refract_next of {cam, dir}, all live = refract",
              "occlusion origin = reflect_next origin", "ao origin = reflect origin with reflect all 1"]


def identity_pairs(run, S, identity):
    """((rays, active), (rays, active), pixels or None, columns) of one identity from run(call, **arrays)."""
    zero = np.zeros(M, f)
    if identity == IDENTITIES[0]:
        return run("refract", transmit=zero), run("reflect"), None, 6
    if identity == IDENTITIES[1]:
        return run("refract_next", transmit=zero), run("reflect_next"), None, 6
    if identity == IDENTITIES[2]:
        return run("reflect_next", **level_from_primary(S)), run("reflect"), None, 6
    if identity == IDENTITIES[3]:
        return run("refract_next", **level_from_primary(S)), run("refract"), None, 6
    if identity == IDENTITIES[4]:
        a, b = run("occlusion"), run("reflect_next")
        return a, b, (np.asarray(a[1]) != 0) & (np.asarray(b[1]) != 0), 3
    a, b = run("ao"), run("reflect", reflect=np.ones(M, f))
    return a, b, (np.asarray(a[1]) != 0) & (np.asarray(b[1]) != 0), 3


def assert_identity(S, identity, pairs, nan_rule=False):
    a, b, px, cols = pairs
    cut = lambda r: (np.ascontiguousarray(np.asarray(r[0]).reshape(N, 6)[:, :cols]), r[1])
    live = same_words(S, cut(a), cut(b), identity, px, nan_rule)
    print("%-56s %5d pixels with a ray on both sides" % (identity, live))
    assert live > 1500, (identity, live)


@pytest.mark.parametrize("identity", IDENTITIES)
def test_checkers_agree_where_two_calls_are_equal(CHECK, identity):
    S = synthetic()
    assert_identity(S, identity, identity_pairs(lambda call, **over: CHECK(call, **over)[:2], S, identity))


def test_oracle_reflect_rays_equal_the_depth_checker(CHECK):
    S = synthetic()
    for eps in (EPS,) + OTHER_EPS:
        same_words(S, CHECK("oracle", None, eps)[:2], CHECK("reflect", None, eps)[:2], "orc_reflect_rays, eps %g" % eps)


def test_ao_direction_is_the_unit_normal_against_d(CHECK):
    S = synthetic()
    rays, act, _ = CHECK("ao")
    n, d = rays.reshape(N, 6)[:, 3:].astype(np.float64), S.dirs.reshape(N, 3).astype(np.float64)
    px = (act == 1) & ordinary_pixels(S)
    assert px.sum() > 2000 and np.abs(np.linalg.norm(n[px], axis=1) - 1).max() < 1e-6
    live = (act == 1) & np.isfinite(n).all(1) & np.isfinite(d).all(1)
    with np.errstate(all="ignore"):
        dn = (d[live] * n[live]).sum(1)
    assert (dn[np.isfinite(dn)] <= 0).all()
    # the occlusion ray ends on the light: o' + (L - o') is L to the rounding of one subtraction
    orays, oact, _ = CHECK("occlusion")
    o = orays.reshape(N, 6).astype(np.float64)
    px = (oact == 1) & ordinary_pixels(S)
    L = S.lights["the light"].astype(np.float64)
    assert px.sum() > 2000 and (np.abs(o[px, :3] + o[px, 3:] - L) <= np.spacing(np.abs(o[px]).max(1).astype(f))[:, None]).all()


def test_a_light_on_a_pixels_origin_gives_that_pixel_a_zero_direction(CHECK, REFS):
    S = synthetic()
    L, p = light_on_a_pixel(S, REFS[1])
    rays, act, _ = CHECK("occlusion", None, EPS, "a light on a pixel's origin")
    assert act[p] == 1 and (bits(rays.reshape(N, 6)[p, 3:]) == 0).all() and np.isfinite(L).all()
    assert in_band()[p] and in_band((6, 9))[p]
    rays, act, _ = CHECK("occlusion", None, EPS, "a light with infinite coordinates")
    r = rays.reshape(N, 6)[(act == 1) & ordinary_pixels(S)]
    assert np.isinf(r[:, 3]).all() and np.isfinite(r[:, 4]).all() and np.isinf(r[:, 5]).all()


# ------------------------------------------------------------------------------------------------ CPU: float64

ORDINARY = ("ordinary", "ordinary 2", "id 0", "id F - 1", "material index 0", "material index %d" % (M - 1),
            "transmit and reflect", "transmit only", "reflect only", "front", "back", "one triangle in both windings",
            "direction of length 0.001", "direction of length 1000", "active 2", "active -1", "active INT_MIN", "active 0x100",
            "reflect sweep", "transmit sweep", "transmit sweep over a mirror", "reflect -0, negative, NaN under glass")
# The largest deviation of the float32 checkers from the float64 restatement on the ordinary pixels, measured on the CPU:
# origins relative to |o| + t |d|, directions relative to the length of the float64 direction (|d| for the mirror rule, 1
# for Snell's).  Asserted at twice the measured value.
MEASURED_ORIGIN, MEASURED_DIRECTION = 1.211e-07, 1.398e-06  # (reflect and ao; refract and refract_next)
MIN_K, MIN_COS = 1.0 / 64, 1.0 / 64  # how far an ordinary pixel keeps from the critical angle (|k|) and from edge-on


def ordinary_pixels(S):
    return np.isin(S.cls, [S.names.index(n) for n in ORDINARY])


def f64_rays(S, call, eps, light):
    """The three rules in float64, written from DESIGN.md section 6 and 6.6: (rays [N, 6], sends a ray, well away from
    the critical angle and from edge-on)."""
    level = call in LEVEL
    r = S.rays.reshape(N, 6).astype(np.float64)
    o = r[:, :3] if level else np.broadcast_to(S.cam_pos.astype(np.float64), (N, 3))
    d, t = S.dirs.reshape(N, 3).astype(np.float64), S.t.astype(np.float64)
    ids = np.maximum(S.ids, 0)
    v = S.verts.reshape(-1, 3, 3)[ids].astype(np.float64)
    m = np.clip(S.mat_idx[ids], 0, M - 1)
    re, tr, ior = (x[m].astype(np.float64) for x in (S.reflect, S.transmit, S.ior))
    with np.errstate(all="ignore"):
        n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        dn = (d * n).sum(1)
        front = ~(dn > 0)
        n = np.where(front[:, None], n, -n)
        dn = -np.abs(dn)
        P = o + t[:, None] * d
        length = np.linalg.norm(d, axis=1)
        mirror = np.concatenate([P + eps * n, d - 2 * dn[:, None] * n], 1)
        u = d / length[:, None]
        c = -dn / length
        ior = np.where(ior > 0, ior, 1.0)
        eta = np.where(front, 1.0 / ior, ior)
        k = 1 - eta * eta * (1 - c * c)
        snell = np.concatenate([P - eps * n, eta[:, None] * u + (eta * c - np.sqrt(np.maximum(k, 0)))[:, None] * n], 1)
        glass = call.startswith("refract") & (tr > 0)
        out = np.where((glass & (k >= 0))[:, None], snell, mirror)
        if call == "occlusion":
            out[:, 3:] = np.asarray(light, np.float64) - out[:, :3]
        if call == "ao":
            out[:, 3:] = n
        sends = (t > 0) & (S.ids >= 0) & ((S.active != 0) | (not level))
        known = (S.mat_idx[ids] >= 0) & (S.mat_idx[ids] < M)
        if call in ("reflect", "reflect_next"):
            sends &= known & (re > 0)
        if call.startswith("refract"):
            sends &= known & ((tr > 0) | (re > 0))
        well = (c >= MIN_COS) & (~glass | (np.abs(k) >= MIN_K)) & np.isfinite(out).all(1)
    scale = np.linalg.norm(o, axis=1) + t * length
    return out, sends, well, dict(eta=eta, c=c, k=k, glass=glass, n=n, length=length, scale=scale)


def test_float64_restatement_bounds_the_checkers(CHECK):
    S = synthetic()
    worst_o = worst_d = 0.0
    ordinary = ordinary_pixels(S)
    for call in CALLS:
        rays, act, kind = CHECK(call)
        got = rays.reshape(N, 6).astype(np.float64)
        ref, sends, well, x = f64_rays(S, call, EPS, S.lights["the light"])
        np.testing.assert_array_equal(act[ordinary] != 0, sends[ordinary], err_msg=call)
        px = ordinary & sends & well
        assert px.sum() > 1500, (call, px.sum())
        if kind is not None:  # the float64 rule takes the branch the checker took
            np.testing.assert_array_equal(kind[px] == TOTAL, x["glass"][px] & (x["k"][px] < 0))
            np.testing.assert_array_equal(np.isin(kind[px], (FRONT, BACK)), x["glass"][px] & (x["k"][px] >= 0))
        eo = np.linalg.norm(got[px, :3] - ref[px, :3], axis=1) / x["scale"][px]
        if call == "occlusion":
            ed = np.linalg.norm(got[px, 3:] - ref[px, 3:], axis=1) / (x["scale"][px] + np.linalg.norm(S.lights["the light"]))
        else:
            ed = np.linalg.norm(got[px, 3:] - ref[px, 3:], axis=1) / np.linalg.norm(ref[px, 3:], axis=1)
        print("%-12s %5d pixels: origin %.3e, direction %.3e" % (call, px.sum(), eo.max(), ed.max()))
        worst_o, worst_d = max(worst_o, eo.max()), max(worst_d, ed.max())
        assert eo.max() <= 2 * MEASURED_ORIGIN and ed.max() <= 2 * MEASURED_DIRECTION, (call, eo.max(), ed.max())
        # on the same pixels: |reflected| = |d|, and Snell's ratio sin(out) = eta sin(in) with a unit direction.  Both
        # are 1-Lipschitz in the direction (n is a unit vector) and exact for the float64 ray, so the bound is the same.
        bound = 2 * MEASURED_DIRECTION
        if call in ("reflect", "reflect_next", "refract", "refract_next"):
            mirrored = px & ~(x["glass"] & (x["k"] >= 0))
            out_len = np.linalg.norm(got[:, 3:], axis=1)
            assert mirrored.sum() > 500 and (np.abs(out_len[mirrored] / x["length"][mirrored] - 1) <= bound).all()
        if call in ("refract", "refract_next"):
            thru = px & x["glass"] & (x["k"] >= 0)
            sin_out = np.linalg.norm(np.cross(got[thru, 3:], x["n"][thru]), axis=1)
            sin_in = np.sqrt(np.maximum(1 - x["c"][thru] ** 2, 0))
            assert thru.sum() > 500 and (np.abs(sin_out - x["eta"][thru] * sin_in) <= bound).all()
            assert (np.abs(np.linalg.norm(got[thru, 3:], axis=1) - 1) <= bound).all()
            assert ((got[thru, 3:] * x["n"][thru]).sum(1) < 0).all()  # into the far side
    print("measured: origin %.3e, direction %.3e" % (worst_o, worst_d))
    assert worst_o >= MEASURED_ORIGIN / 1.01 and worst_d >= MEASURED_DIRECTION / 1.01  # the constants are the measured ones


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Device:
    """One context per band and the fixture on the device: mat_idx, the triangle list, reflect, transmit and ior as views
    into the middle of larger tensors."""

    def __init__(self, ugrt, S):
        self.u, self.S, self.ctx = ugrt, S, {}
        for name, rows in BANDS.items():
            self.ctx[rows] = c = ugrt.Context(W, H, light_grid=RD.LG, uniform_dims=RD.UD, rows=rows)
            assert (c.p0, c.npix) == band_of(rows), name
        self.up = up = self.ctx[None].upload
        self.a = {k: up(np.array(getattr(S, k)).reshape(-1)) for k in ("cam_pos", "t", "dirs", "ids", "rays", "active", "verts")}
        self.a["hit_t"], self.a["hit_id"] = self.a["t"], self.a["ids"]
        self.big = {k: up(v) for k, v in S.big.items()}
        for k, n in (("mat_idx", S.F), ("faces", 3 * S.F), ("reflect", M), ("transmit", M), ("ior", M)):
            lo = MARGIN * (3 if k == "faces" else 1)
            self.a[k] = self.big[k][lo:lo + n]
            assert self.a[k].is_contiguous() and self.a[k].data_ptr() == self.big[k].data_ptr() + 4 * lo

    def coefficients(self, name, arr):
        """A coefficient list of the test's own (an identity's) as a view with the same margins."""
        big = np.concatenate([np.full(MARGIN, 0.5, f), np.asarray(arr, f), np.full(MARGIN, 0.5, f)])
        return self.up(big)[MARGIN:MARGIN + M]

    def run(self, call, rows=None, eps=EPS, light="the light", **over):
        """(rays, active) on the host; outside the band the sentinels."""
        c, t = self.ctx[rows], self.ctx[None].torch
        light = self.S.lights[light] if isinstance(light, str) else light
        a = dict(self.a)
        for k, v in over.items():
            a[k] = self.coefficients(k, v) if k in ("reflect", "transmit", "ior") else self.up(np.array(v).reshape(-1))
        rays = t.full((6 * N,), float(RAY), dtype=t.float32, device=c.device)
        act = t.full((N,), ACT, dtype=t.int32, device=c.device)
        prim = [a["cam_pos"], a["t"], a["dirs"], a["ids"]]
        lev = [a["rays"], a["active"], a["hit_t"], a["hit_id"]]
        geo = [a["verts"], a["faces"], eps, rays, act]
        if call == "reflect":
            c.reflect_rays(*prim, a["mat_idx"], a["reflect"], M, *geo)
        elif call == "reflect_next":
            c.reflect_rays_next(*lev, a["mat_idx"], a["reflect"], M, *geo)
        elif call == "refract":
            c.refract_rays(*prim, a["mat_idx"], a["reflect"], a["transmit"], a["ior"], M, *geo)
        elif call == "refract_next":
            c.refract_rays_next(*lev, a["mat_idx"], a["reflect"], a["transmit"], a["ior"], M, *geo)
        elif call == "occlusion":
            c.occlusion_rays(*lev, a["verts"], a["faces"], [float(x) for x in light], eps, rays, act)
        elif call == "ao":
            c.ao_rays(*prim, *geo)
        else:
            raise KeyError(call)
        c.synchronize()
        return rays.cpu().numpy(), act.cpu().numpy()


@pytest.fixture(scope="module")
def DEV(ugrt, torch):
    return Device(ugrt, synthetic())


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("call", CALLS)
def test_generators_equal_their_checkers(CHECK, DEV, REFS, call, rows):
    S = DEV.S
    what = "%s, %s" % (call, rows)
    compare(S, DEV.run(call, rows, EPS, S.lights["the light"]), CHECK(call, rows), rows, what)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("light", ["a light on a pixel's origin", "a light with infinite coordinates"])
def test_occlusion_rays_towards_odd_lights_equal_their_checker(CHECK, DEV, REFS, light, rows):
    S = DEV.S
    got = DEV.run("occlusion", rows, EPS, light_of(S, REFS, light))
    compare(S, got, CHECK("occlusion", rows, EPS, light), rows, "occlusion, %s, %s" % (light, rows))
    if light == "a light on a pixel's origin":
        p = light_on_a_pixel(S, REFS[1])[1]
        if in_band(rows)[p]:
            assert (bits(got[0]).reshape(N, 6)[p, 3:] == 0).all() and got[1][p] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("eps", OTHER_EPS)
@pytest.mark.parametrize("call", CALLS)
def test_generators_equal_their_checkers_at_other_eps(CHECK, DEV, call, eps):
    S = DEV.S
    compare(S, DEV.run(call, None, eps, S.lights["the light"]), CHECK(call, None, eps), None, "%s, eps %g" % (call, eps))


@pytest.mark.gpu
@pytest.mark.parametrize("identity", IDENTITIES)
def test_identities_hold_on_the_device(DEV, identity):
    S = DEV.S
    run = lambda call, **over: DEV.run(call, None, EPS, S.lights["the light"], **over)
    assert_identity(S, identity, identity_pairs(run, S, identity), nan_rule=True)


@pytest.mark.gpu
def test_null_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, CHECK, DEV, torch):
    S, c, a = DEV.S, DEV.ctx[None], DEV.a
    rays = torch.full((6 * N,), float(RAY), dtype=torch.float32, device=c.device)
    act = torch.full((N,), ACT, dtype=torch.int32, device=c.device)
    prim = [a["cam_pos"], a["t"], a["dirs"], a["ids"]]
    lev = [a["rays"], a["active"], a["hit_t"], a["hit_id"]]
    mats = [a["mat_idx"], a["reflect"]]
    glass = mats + [a["transmit"], a["ior"]]
    geo = [a["verts"], a["faces"], EPS, rays, act]
    cases = [(c.reflect_rays, prim + mats + [M] + geo, 5), (c.reflect_rays_next, lev + mats + [M] + geo, 1),
             (c.refract_rays, prim + glass + [M] + geo, 6), (c.refract_rays_next, lev + glass + [M] + geo, 7),
             (c.occlusion_rays, lev + geo[:2] + [[3.0, 4.0, 5.0]] + geo[2:], 9), (c.ao_rays, prim + geo, 7)]
    for fn, args, hole in cases:
        assert args[hole] is not None and not isinstance(args[hole], (int, float))
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*(args[:hole] + [None] + args[hole + 1:]))
        assert e.value.code == ugrt.UGRT_EINVAL and b"null" in ugrt.lib.ugrt_last_error(), fn.__name__
    c.synchronize()
    assert bool((rays == float(RAY)).all()) and bool((act == ACT).all())  # nothing was enqueued
    compare(S, DEV.run("refract_next", None, EPS), CHECK("refract_next"), None, "refract_next after the refusals")
