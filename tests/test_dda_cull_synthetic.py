"""The bounce walk's bundle cull (d_beam_box, d_cull_beam of csrc/ugrt_dda.h) on rays and triangles of its own: edge-on
hits, bundles that are one ray, fans with the aimed rays on the faces of their box, directions of every length.

Every other bounce test walks cornell, hall or crash, or a random soup: rays that pass the exact test on a triangle by
less than the cull's margin do not occur there, and the oracle visits every reference of a cell, so a cull that drops
what the exact test accepts goes unseen.  Here ugrt_trace_dda is called on buffers the test fills itself, over a soup
of 4 300 triangles (300 of them small and around the scene's middle: lists of more than 64 there) in a uniform grid of (8,8,8) built with ugrt_grid_build_uniform, image 256 x 128 = 32 768 ray slots,
every pixel active (a chunk of the ray list is then 64 consecutive pixels), inputs built with numpy in float64, rounded
once to float32, and seeded.  Each ray is built for a triangle k, from an origin inside the grid unless it is far:
   1 through an interior point of k      2 through a point of an edge of k      3 through a vertex of k
   4 kinds 2 and 3 with the direction moved by 1e-6 and by 1e-5 of itself
   5 kinds 1 to 3 from an origin 2 to 100 scene extents away (a large entry parameter: d_beam_box forms o + t_in d)
   0 (fan layout only) the other rays of a bundle: directions inside the box of the bundle's aimed rays
The origin is rounded to float32 first and the direction is formed from the rounded origin, so the ray misses its point
by the rounding of the direction alone.  Layouts, each with launches of its own:
   repeated  one ray fills its group of 64 consecutive pixels bit for bit: the bundle's box is the ray, and only the
             floors of orad and dr and the margins stand between the cull and the exact test
   fan       the 64 rays of a group start within a thousandth of an extent of each other; four of them, one per 16
             consecutive pixels, are aimed (kinds 2 to 4) at a triangle and two of its neighbours, the others lie
             inside the box of those four: an aimed ray is extreme in a direction component, so it lies on a face of
             the box of its 64, its 32 and its 16 rays
   mixed     the kinds dealt at random per pixel
Scales (direction length, scene extent, scene centre in extents along (1, -0.7, 0.4)): each value of each axis with the
others at their middle value, and two corners: see SCALES.

CPU tests (unmarked): conditions on the oracle, and on a numpy float32 restatement of d_beam_box and d_cull_beam, that
let the GPU tests fail.  The restatement cannot contract products to FMAs as the device code does; it only shows that
the inputs are sharp, and no GPU test compares against it.
GPU tests: ids equal and t bit-equal to O.trace_dda on O.grid_uniform with the cull forced (dda_cull_min 1,
dda_cull_work 1), at its default thresholds and off, each at 16, 32 and 64 rays per wave, dda_sort 0 and 1, dda_split 0
and 4, and the per-ray kernel; a counting context must report that the forced cull ran.

Oracle figures (the same soup at every scale: 4 300 triangles, 8 054 grid references, 508 of 512 cells used, mean
list 15.9, longest 96).  "hit" = the ray's expected id is its triangle k; rays counted once (repeated: 512 a scale).
  rays through an edge or a vertex, not moved, hit / not, per scale:  repeated 118-148 / 153-186,
      fan 391-564 / 740-927 (of 2 048 aimed rays a scale), mixed 6 095-6 679 / 8 055-8 683
  ... of them with k as the expected id, all scales: repeated 1 488, fan 4 824, mixed 69 439
  mixed, per kind, hit / rays at scale "middle": 1: 4 624 / 5 591, 2: 4 465 / 8 416, 3: 1 174 / 4 118,
      4: 3 271 / 9 795, 5: 1 332 / 4 848 (the other scales within 4 % of these; none of kind 5 at the origin scales)
  mixed, edge and vertex rays whose id changes when moved by 1e-6 / 1e-5: 5 134-5 432 / 5 274-5 540 of 14 561-14 912
  fan: aimed rays on a face of the box of their 64 / 32 / 16 rays: 76-77 % / 79-81 % / 86-89 %; largest angle to the
      group's mean direction, median 5.1-5.7 degrees (10.6 at the origin scales)
  restated cull, repeated layout, rays with a hit 409-439 a scale: hits dropped with the library's margins 0 at every
      scale; with K = 0 and bare boxes 46-95 a scale, 760 in all.  With the margins as they were before they followed
      the directions' length the restatement drops 1 (dir1e6-origin); on two million edge-aimed single-ray bundles
      with origins within 1e-3 of the coordinate origin and triangles of extent 100 it drops 48 of 130 000 hits at
      |d| = 1e3, 12 % at 1e4 and 1e6, and none with the margins as they are.
Measured on an MI355X: the 66 GPU tests of this file take 5 s together (0.2 s each; the first 0.45 s).
  The build before the margins followed the directions' length fails test_walk_equals_the_oracle[dir1e6-origin-repeated]
  (64 rays = one distinct ray, forced cull, dda_sort 1: a farther triangle than the oracle's) and [dir1e6-mixed] (1 ray,
  forced cull, 16 rays per wave); it passes the other 64.
  A build with K = 0, the boxes not widened (1.0001, + 1e-6, 7.63e-6) and d_cull_tlow's factor 1 fails all 66: in
  test_walk_equals_the_oracle under the forced cull at 16 rays per wave, repeated 1 728-4 224 rays (27-66 distinct
  rays) a scale, mixed 290-3 743, fan 3-41; test_the_forced_cull_runs 1-3 584.  Of the suite as it was
  before this file, 603 GPU tests, that build fails 3 for the bounce: test_bounce_kernels_on_synthetic_rays[cornell-ud3-4]
  by 3 rays of 32 768, test_display_paths_agree and test_display_paths_agree_at_depth_3 by 2 image bytes of 184 320
  each (and 5 of tests/test_shadow_synthetic.py for the shadow cull, as its docstring says).
"""
import functools
import types

import numpy as np
import pytest

W, H = 256, 128
N = W * H
GROUP = 64
NGROUPS = N // GROUP
DIMS = (8, 8, 8)
NSOUP, NCLUSTER = 4000, 300  # triangles all over the scene, and small ones around its middle
NTRI = NSOUP + NCLUSTER
CENTRE_DIR = np.array([1.0, -0.7, 0.4])
# name: (direction length, scene extent, scene centre in extents)
SCALES = {
    "middle": (1.0, 1.0, 0.0),
    "dir1e-3": (1e-3, 1.0, 0.0), "dir1e3": (1e3, 1.0, 0.0), "dir1e6": (1e6, 1.0, 0.0),
    "extent1e-2": (1.0, 1e-2, 0.0), "extent1e3": (1.0, 1e3, 0.0),
    "far": (1.0, 1.0, 1e3),
    "long-large-far": (1e6, 1e3, 1e3), "short-tiny": (1e-3, 1e-2, 0.0),
    "dir1e3-origin": (1e3, 1e3, 0.0), "dir1e6-origin": (1e6, 1e3, 0.0),
}
# Scales whose rays all start within 1e-6 extents of the coordinate origin (the middle of the scene, so inside the grid),
# at the small triangles around it (most in the eight cells that meet there, which the rays enter at t_in = 0).  The half width of the origin box is relative to |o'| but for a floor of 1e-6
# (d_beam_box: 7.63e-6 |o'| + 1e-6); everywhere else it happens to stand in for margins that are too small, because it
# is multiplied by |d x e|, which grows with the directions' length.  Here, with an extent of 1e3, it is 1e-9 of the
# distances and stands in for nothing: the margins are alone.
AT_ORIGIN = ("dir1e3-origin", "dir1e6-origin")
LAYOUTS = ("repeated", "fan", "mixed")
MOVES = (1e-6, 1e-5)
FAR_SHARE = 0.15
K_LIB = np.float32(6.0 / 65536.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------ inputs

@functools.lru_cache(maxsize=None)
def soup(O, scale):
    """The triangles of a scale and their uniform grid (the oracle's)."""
    dlen, E, centre = SCALES[scale]
    rng = np.random.default_rng(20261020)  # (the same soup at every scale, scaled and moved)
    c = np.concatenate([rng.uniform(-0.5, 0.5, (NSOUP, 3)), rng.normal(size=(NCLUSTER, 3)) * 0.05])
    size = np.concatenate([np.exp(rng.uniform(np.log(0.01), np.log(0.1), NSOUP)),
                           np.exp(rng.uniform(np.log(0.005), np.log(0.02), NCLUSTER))])
    tris = c[:, None, :] + rng.normal(size=(NTRI, 3, 3)) * (0.5 * size)[:, None, None]
    verts = np.ascontiguousarray((tris * E + CENTRE_DIR * centre * E).reshape(-1, 3), np.float32)
    faces = np.arange(3 * NTRI, dtype=np.int32).reshape(-1, 3)
    v = verts.reshape(-1, 3, 3).astype(np.float64)
    cen = v.mean(1)
    # the three nearest triangles of each (itself first), in the soup's own coordinates
    m = tris.mean(1)
    sq = (m * m).sum(1)
    near = np.argsort(sq[:, None] + sq[None, :] - 2.0 * m @ m.T, axis=1)[:, :3]
    bbmin, bbmax = verts.min(0), verts.max(0)
    ug = O.grid_uniform(faces, verts, bbmin, bbmax, DIMS)
    at_origin = scale in AT_ORIGIN
    pick = np.arange(NSOUP, NTRI) if at_origin else np.arange(NTRI)
    return types.SimpleNamespace(scale=scale, dlen=dlen, E=E, verts=verts, faces=faces, v=v, cen=cen, near=near,
                                 bbmin=bbmin, bbmax=bbmax, ug=ug, F=NTRI, at_origin=at_origin, pick=pick)


def aim(rng, S, k, target, move, origin):
    """Rays from `origin` ([n, 3], float64) through a point of triangle k[n]: target 1 interior, 2 edge, 3 vertex;
    move: 0, or the relative size of what is added to the direction.  -> origins and directions, float32."""
    n = len(k)
    b = 0.15 + 0.55 * rng.dirichlet([1, 1, 1], n)
    pair = rng.dirichlet([1, 1], n)
    zero = rng.integers(0, 3, n)
    others = np.array([[1, 2], [0, 2], [0, 1]])[zero]
    on_edge = np.zeros((n, 3))
    on_edge[np.arange(n), others[:, 0]], on_edge[np.arange(n), others[:, 1]] = pair[:, 0], pair[:, 1]
    b = np.where((target == 2)[:, None], on_edge, b)
    b = np.where((target == 3)[:, None], np.eye(3)[rng.integers(0, 3, n)], b)
    Q = (S.v[k] * b[:, :, None]).sum(1)
    o32 = origin.astype(np.float32)
    d = unit(Q - o32.astype(np.float64)) * S.dlen
    d = d * (1.0 + move[:, None] * rng.normal(size=(n, 3)))
    return o32, d.astype(np.float32), Q


def origins(rng, S, P, far, near=(0.03, 0.3)):
    """An origin per point P: `near` extents away and inside the grid, or (far) 2 to 100 extents away."""
    n = len(P)
    if S.at_origin:
        return rng.uniform(-1e-6, 1e-6, (n, 3)) * S.E
    u = unit(rng.normal(size=(n, 3)))
    r = np.exp(rng.uniform(np.log(near[0]), np.log(near[1]), n)) * S.E
    lo, hi = S.bbmin.astype(np.float64), S.bbmax.astype(np.float64)
    for _ in range(12):
        o = P - u * r[:, None]
        outside = ((o < lo) | (o > hi)).any(1)
        r = np.where(outside, 0.5 * r, r)
    rf = np.exp(rng.uniform(np.log(2.0), np.log(100.0), n)) * S.E
    return np.where(far[:, None], P - u * rf[:, None], P - u * r[:, None])


def deal(rng, n, share=(0.20, 0.30, 0.15, 0.35)):
    """target, move and far per ray: interior, edge, vertex, moved edge or vertex by `share`; 15 % far."""
    kind = rng.choice(np.array([1, 2, 3, 4]), n, p=share)
    target = np.where(kind == 4, rng.choice(np.array([2, 3]), n, p=[0.7, 0.3]), kind)
    move = np.where(kind == 4, rng.choice(np.asarray(MOVES), n), 0.0)
    far = rng.random(n) < FAR_SHARE
    return target, move, far


def kind_of(target, move, far):
    return np.where(far, 5, np.where(move > 0, 4, target))


@functools.lru_cache(maxsize=None)
def rays_of(O, scale, layout):
    """rays [N, 6] float32 with what each was built for: k (-1: none), target, move, far, kind."""
    S = soup(O, scale)
    rng = np.random.default_rng([20261021, sorted(SCALES).index(scale), LAYOUTS.index(layout)])
    if layout in ("repeated", "mixed"):
        n = NGROUPS if layout == "repeated" else N
        # (the repeated layout has 512 distinct rays: more of them on edges)
        target, move, far = deal(rng, n) if layout == "mixed" else deal(rng, n, (0.10, 0.45, 0.15, 0.30))
        k = rng.choice(S.pick, n)
        far &= not S.at_origin
        o32, d32, Q = aim(rng, S, k, target, move, origins(rng, S, S.cen[k], far))
        rep = GROUP if layout == "repeated" else 1
        rays = np.repeat(np.concatenate([o32, d32], 1), rep, axis=0)
        k, target, move, far = (np.repeat(a, rep) for a in (k, target, move, far))
        aimed = np.ones(N, bool)
    else:
        g = NGROUPS
        k0 = rng.choice(S.pick, g)
        gfar = (rng.random(g) < FAR_SHARE) & (not S.at_origin)
        og = origins(rng, S, S.cen[k0], gfar, near=(0.25, 0.6))
        o = og[:, None, :] + rng.uniform(-1e-3, 1e-3, (g, GROUP, 3)) * S.E
        # the aimed rays: one per 16 pixels, at k0, k0 and two of its neighbours
        slot = 16 * np.arange(4)[None, :] + rng.integers(0, 16, (g, 4))
        ks = np.stack([k0, k0, S.near[k0, 1], S.near[k0, 2]], 1)
        kind = rng.choice(np.array([2, 3, 4]), (g, 4), p=[0.45, 0.2, 0.35])
        tg = np.where(kind == 4, rng.choice(np.array([2, 3]), (g, 4), p=[0.7, 0.3]), kind)
        mv = np.where(kind == 4, rng.choice(np.asarray(MOVES), (g, 4)), 0.0)
        rows = np.arange(g)[:, None]
        ao32, ad32, _ = aim(rng, S, ks.reshape(-1), tg.reshape(-1), mv.reshape(-1), o[rows, slot].reshape(-1, 3))
        ad = ad32.reshape(g, 4, 3).astype(np.float64)
        lo, hi = ad.min(1), ad.max(1)
        wdt = hi - lo
        fill = (lo + 0.05 * wdt)[:, None, :] + rng.random((g, GROUP, 3)) * (0.9 * wdt)[:, None, :]
        rays = np.concatenate([o, fill], 2).astype(np.float32)
        rays[rows, slot] = np.concatenate([ao32, ad32], 1).reshape(g, 4, 6)
        rays = rays.reshape(N, 6)
        k = np.full((g, GROUP), -1)
        target, move = np.zeros((g, GROUP), int), np.zeros((g, GROUP))
        k[rows, slot], target[rows, slot], move[rows, slot] = ks, tg, mv
        aimed = (k >= 0).reshape(N)
        k, target, move = k.reshape(N), target.reshape(N), move.reshape(N)
        far = np.repeat(gfar, GROUP)
    kind = np.where(aimed, kind_of(target, move, far), 0)
    return types.SimpleNamespace(S=S, layout=layout, rays=np.ascontiguousarray(rays, np.float32), k=k, target=target,
                                 move=move, far=far, kind=kind, aimed=aimed)


ACTIVE = np.ones(N, np.int32)


def trace(O, S, rays):
    t, ids, cnt = O.trace_dda(S.ug, S.verts, S.faces, np.ascontiguousarray(rays, np.float32).reshape(-1), ACTIVE, 0, N, N)
    return t, ids, cnt


@functools.lru_cache(maxsize=None)
def want(O, scale, layout):
    R = rays_of(O, scale, layout)
    return trace(O, R.S, R.rays)


def sharp(R):
    """The rays aimed at an edge or a vertex, not moved."""
    return R.aimed & (R.target >= 2) & (R.move == 0)


# ------------------------------------------------------------------------------------------------ the cull, restated

def f32(x):
    return np.asarray(x, np.float32)


def cells_before_the_hit(ug, o, d, t_hit):
    """The walk of csrc/ugrt_dda.h (d_dda_clip, d_dda_axes, d_dda_step) in float32, over all rays at once: yields, per
    step, (which rays are in a cell they entered no later than their hit, the cell, its entry parameter)."""
    g, dims = ug["ug"], [int(x) for x in ug["dims"]]
    n = len(o)
    ar = np.arange(n)
    tenter, texit = np.zeros(n, np.float32), np.full(n, 3.0e38, np.float32)
    with np.errstate(all="ignore"):
        for k in range(3):
            lo, hi = g[k], f32(g[k] + g[3 + k] * np.float32(dims[k]))
            nz = d[:, k] != 0
            inv = np.float32(1.0) / d[:, k]
            t0, t1 = (lo - o[:, k]) * inv, (hi - o[:, k]) * inv
            t0, t1 = np.where(t0 > t1, t1, t0), np.where(t0 > t1, t0, t1)
            tenter = np.where(nz & (t0 > tenter), t0, tenter)
            texit = np.where(nz & (t1 < texit), t1, texit)
            texit = np.where(~nz & ((o[:, k] < lo) | (o[:, k] > hi)), np.float32(-1), texit)
        alive = tenter <= texit
        c = np.zeros((n, 3), np.int64)
        step = np.zeros((n, 3), np.int64)
        tmax, tdelta = np.full((n, 3), 3.0e38, np.float32), np.full((n, 3), 3.0e38, np.float32)
        for k in range(3):
            pe = o[:, k] + tenter * d[:, k]
            c[:, k] = np.clip(np.floor((pe - g[k]) * g[6 + k]), 0, dims[k] - 1).astype(np.int64)
            pos, neg = d[:, k] > 0, d[:, k] < 0
            step[:, k] = np.where(pos, 1, np.where(neg, -1, 0))
            wall = g[k] + (c[:, k] + pos).astype(np.float32) * g[3 + k]
            tmax[:, k] = np.where(pos | neg, (wall - o[:, k]) / d[:, k], np.float32(3.0e38))
            tdelta[:, k] = np.where(pos, g[3 + k] / d[:, k], np.where(neg, -g[3 + k] / d[:, k], np.float32(3.0e38)))
        tin = tenter.astype(np.float32)
        for _ in range(sum(dims) + 2):
            here = alive & (tin <= t_hit)
            if not here.any():
                break
            yield here, (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2], tin
            ax = np.where(tmax[:, 0] < tmax[:, 1], np.where(tmax[:, 0] < tmax[:, 2], 0, 2),
                          np.where(tmax[:, 1] < tmax[:, 2], 1, 2))
            tin = tmax[ar, ax]
            c[ar, ax] += step[ar, ax]
            alive &= ~((step[ar, ax] == 0) | (c[ar, ax] < 0) | (c[ar, ax] >= np.asarray(dims)[ax]))
            tmax[ar, ax] = tmax[ar, ax] + tdelta[ar, ax]


def beam_box_of_one_ray(o, d, tin, library):
    """d_beam_box for bundles of one ray each (lo == hi); library False: the boxes not widened, K = 0."""
    one = np.float32(1.0001)
    p = o + tin[:, None] * d
    oc, dc = np.float32(0.5) * (p + p), np.float32(0.5) * (d + d)
    s = np.maximum(np.float32(1.0), np.abs(d).max(1))
    if library:
        orad = np.float32(0.5) * (p - p) * one + np.float32(7.63e-6) * np.abs(p) + np.float32(1e-6)
        dr = np.float32(0.5) * (d - d) * one + np.float32(1e-6)  # (over s already)
        km = np.full_like(s, K_LIB)
    else:
        orad, dr, km = np.zeros_like(p), np.zeros_like(d), np.zeros_like(s)
    on = np.sqrt((orad * orad).sum(1, dtype=np.float32)) * one
    dc = dc * (np.float32(1.0) / s)[:, None]  # (the device takes v_rcp_f32, inside the halving)
    da = np.abs(dc) + dr
    dmax = np.sqrt((da * da).sum(1, dtype=np.float32)) * one * s
    reach = (tin * dmax + on) * np.float32(1.001)
    return types.SimpleNamespace(oc=oc, orad=orad, dc=dc, dr=dr, reach=reach, km=km)


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def cull_beam(v0, e1, e2, bx):
    """d_cull_beam, operation for operation, without FMA contraction: true = the cull drops the triangle."""
    tc = bx.oc - v0
    nA, nB, nD = cross(e2, tc), cross(tc, e1), cross(e2, e1)
    nC = nA + nB - nD
    a = np.abs(tc).max(1) + bx.reach
    b, c = np.abs(e1).max(1), np.abs(e2).max(1)
    tiny = np.float32(1e-25)
    mA, mB, mD = np.maximum(bx.km * a * c, tiny), np.maximum(bx.km * a * b, tiny), np.maximum(bx.km * b * c, tiny)
    Dm, Dr = dot(nD, bx.dc), dot(np.abs(nD), bx.dr)
    sane = (Dm + Dr < np.float32(1e15)) & (Dm - Dr > np.float32(-1e15))

    def origin_term(E):
        dc, dr, orad = bx.dc, bx.dr, bx.orad
        return (orad[:, 0] * (np.abs(dc[:, 1] * E[:, 2] - dc[:, 2] * E[:, 1]) + dr[:, 1] * np.abs(E[:, 2]) + dr[:, 2] * np.abs(E[:, 1])) +
                orad[:, 1] * (np.abs(dc[:, 2] * E[:, 0] - dc[:, 0] * E[:, 2]) + dr[:, 2] * np.abs(E[:, 0]) + dr[:, 0] * np.abs(E[:, 2])) +
                orad[:, 2] * (np.abs(dc[:, 0] * E[:, 1] - dc[:, 1] * E[:, 0]) + dr[:, 0] * np.abs(E[:, 1]) + dr[:, 1] * np.abs(E[:, 0])))

    one = np.float32(1.0001)
    Am, Ar = dot(nA, bx.dc), (dot(np.abs(nA), bx.dr) + origin_term(e2)) * one
    Bm, Br = dot(nB, bx.dc), (dot(np.abs(nB), bx.dr) + origin_term(e1)) * one
    Cm, Cr = dot(nC, bx.dc), (dot(np.abs(nC), bx.dr) + origin_term(e2 - e1)) * one
    mC = mA + mB + mD
    pos = (Dm - Dr > mD) & ((Am + Ar < -mA) | (Bm + Br < -mB) | (Cm - Cr > mC))
    neg = ~(Dm - Dr > mD) & (Dm + Dr < -mD) & ((Am - Ar > mA) | (Bm - Br > mB) | (Cm + Cr < -mC))
    return sane & (pos | neg)


def dropped_hits(O, scale, library):
    """Repeated layout, one ray per group: (rays with a hit, those whose hit triangle the restated cull drops in a cell
    of the walk that lists it and that the ray enters no later than the hit)."""
    R = rays_of(O, scale, "repeated")
    S = R.S
    t, ids, _ = want(O, scale, "repeated")
    sel = np.flatnonzero(ids[::GROUP] >= 0) * GROUP
    o, d, tri, th = R.rays[sel, :3], R.rays[sel, 3:], ids[sel].astype(np.int64), t[sel]
    v = S.verts.reshape(-1, 3, 3)
    v0, e1, e2 = v[tri, 0], v[tri, 1] - v[tri, 0], v[tri, 2] - v[tri, 0]
    listed = np.sort(S.ug["keys"].astype(np.int64) * S.F + S.ug["vals"].astype(np.int64))
    dropped = np.zeros(len(sel), bool)
    seen = np.zeros(len(sel), bool)
    with np.errstate(all="ignore"):
        for here, cell, tin in cells_before_the_hit(S.ug, o, d, th):
            here = here & np.isin(cell * S.F + tri, listed)
            seen |= here
            dropped |= here & cull_beam(v0, e1, e2, beam_box_of_one_ray(o, d, tin, library))
    assert seen.all()  # the restated walk meets the hit triangle's cell for every ray
    return len(sel), dropped


# ------------------------------------------------------------------------------------------------ CPU: the inputs

@pytest.mark.parametrize("scale", sorted(SCALES))
def test_inputs_can_fail(O, scale):
    """By the oracle: of the rays through an edge or a vertex of their triangle k, at least a quarter hit k and at least
    a quarter do not; the lists are tens of triangles long; the aimed rays of a fan lie on a face of their box."""
    S = soup(O, scale)
    span = S.ug["span"]
    print("%s: R %d, cells used %d of %d, mean list %.1f, longest %d" % (
        scale, S.ug["R"], (span > 0).sum(), span.size, span[span > 0].mean(), span.max()))
    assert span[span > 0].mean() >= 10 and (span >= 20).sum() >= 100
    for layout in LAYOUTS:
        R = rays_of(O, scale, layout)
        t, ids, cnt = want(O, scale, layout)
        step = GROUP if layout == "repeated" else 1  # (distinct rays)
        e = sharp(R)[::step]
        hit = (ids == R.k)[::step]
        line = ["%s %s:" % (scale, layout)]
        for kd in range(6):
            m = (R.kind == kd)[::step]
            line.append("kind %d %d/%d" % (kd, (hit & m).sum(), m.sum()))
        print(" ".join(line), "(hit k / rays); edge and vertex rays: hit %d, not %d; any hit %d" % (
            (hit & e).sum(), (~hit & e).sum(), (ids[::step] >= 0).sum()))
        assert (hit & e).sum() >= 0.25 * e.sum() and (~hit & e).sum() >= 0.25 * e.sum()
        assert np.isfinite(R.rays).all()
        if layout == "repeated":
            g = R.rays.reshape(NGROUPS, GROUP, 6)
            assert (bits(g) == bits(g[:, :1])).all()
        if layout == "fan":
            g = R.rays.reshape(NGROUPS, GROUP, 6)[:, :, 3:]
            aimed = R.aimed.reshape(NGROUPS, GROUP)
            assert (aimed.reshape(NGROUPS, 4, 16).sum(2) == 1).all()
            for width in (64, 32, 16):
                b = g.reshape(-1, width, 3)
                extreme = ((b == b.min(1, keepdims=True)) | (b == b.max(1, keepdims=True))).any(2).reshape(NGROUPS, GROUP)
                print("   aimed rays on a face of the box of their %d rays: %d of %d" % (width, (extreme & aimed).sum(), aimed.sum()))
                # (of four independent points, one is neither the least nor the greatest in any of three components with
                # probability 1/8; two of the four are aimed at one triangle, which makes it more: two thirds is asked for)
                assert 3 * (extreme & aimed).sum() >= 2 * aimed.sum()
            # a few degrees
            spread = np.degrees(np.arccos(np.clip((unit(g.astype(np.float64)) * unit(g.astype(np.float64).mean(1, keepdims=True))).sum(2), -1, 1)))
            print("   largest angle to the group's mean direction: median %.2f deg" % np.median(spread.max(1)))
            assert np.median(spread.max(1)) < 15.0


def test_a_thousand_edge_rays_end_on_their_triangle(O):
    """At least 1000 distinct rays through an edge or a vertex have their triangle k as the expected hit, per layout
    over the scales (repeated: 512 distinct rays per scale) and in the mixed layout at every scale."""
    for layout in LAYOUTS:
        total = 0
        for scale in sorted(SCALES):
            R = rays_of(O, scale, layout)
            step = GROUP if layout == "repeated" else 1
            n = ((want(O, scale, layout)[1] == R.k) & sharp(R))[::step].sum()
            total += n
            if layout == "mixed":
                assert n >= 1000, (scale, n)
        print("%s: %d edge and vertex rays end on their triangle" % (layout, total))
        assert total >= 1000


@pytest.mark.parametrize("scale", sorted(SCALES))
def test_moved_edge_rays_change_their_hits(O, scale):
    """The exact test decides the edge and vertex rays at the scale of the cull's margins: moving their directions by
    1e-6 and by 1e-5 of themselves changes the hit id of a counted share (the counts are in the docstring)."""
    R = rays_of(O, scale, "mixed")
    ids = want(O, scale, "mixed")[1]
    e = sharp(R)
    for rel in MOVES:
        rng = np.random.default_rng(7)
        rays = R.rays.astype(np.float64)
        rays[:, 3:] *= 1.0 + rel * rng.normal(size=(N, 3))
        moved = trace(O, R.S, rays.astype(np.float32))[1]
        changed = (moved != ids) & e
        print("%s: edge and vertex rays moved by %g: %d of %d ids change" % (scale, rel, changed.sum(), e.sum()))
        # a ray that lies on the edge to within the direction's rounding (6e-8) is put to either side of it by a move
        # 16 or 160 times that; it changes its id when it was a hit and lands outside, or the reverse: about half
        assert changed.sum() >= 0.2 * e.sum()


def test_restated_cull_is_sharp_on_the_repeated_layout(O):
    """The float32 restatement of d_beam_box and d_cull_beam on bundles of one ray: with the library's margins it drops
    no triangle that the oracle reports as the ray's hit; with K = 0 and the boxes not widened it drops at least 100."""
    lost = 0
    for scale in sorted(SCALES):
        n, lib = dropped_hits(O, scale, True)
        _, bare = dropped_hits(O, scale, False)
        print("%s: %d rays with a hit; the restated cull drops the hit of %d, of %d with K = 0 and bare boxes" % (
            scale, n, lib.sum(), bare.sum()))
        assert lib.sum() == 0, scale
        lost += bare.sum()
    assert lost >= 100


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


OPTIONS = ("dda_kernel", "dda_rays_per_wave", "dda_cull_min", "dda_cull_work", "dda_sort", "dda_split")
CULLS = {"forced": dict(dda_cull_min=1, dda_cull_work=1), "default": {}, "off": dict(dda_cull_min=1 << 30)}
# (dda_split 4 twice: the second launch cuts every group by the history the first one left)
SHAPES = [dict(dda_rays_per_wave=16), dict(dda_rays_per_wave=32), dict(dda_rays_per_wave=64), dict(dda_sort=0),
          dict(dda_sort=1), dict(dda_split=0), dict(dda_split=4), dict(dda_split=4), dict(dda_kernel=1)]


class Walk:
    """A context with the scale's soup uploaded and its uniform grid built."""

    def __init__(self, ugrt, S, flags=0):
        self.ctx = ctx = ugrt.Context(W, H, light_grid=(W // 8, H // 8), uniform_dims=DIMS, flags=flags)
        self.dv, self.df = ctx.upload(S.verts.reshape(-1)), ctx.upload(S.faces.reshape(-1))
        ctx.grid_build_uniform(self.df, self.dv, S.F, S.bbmin, S.bbmax)
        value, key, span, offset, gi = ctx.grid_arrays(ugrt.GRID_UNIFORM)
        assert gi.total_refs == S.ug["R"]
        for got, name in ((value, "vals"), (span, "span"), (offset, "offset")):
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), S.ug[name], err_msg=name)
        self.grid = ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3]
        self.active = ctx.upload(ACTIVE)

    def trace(self, torch, d_rays, **opts):
        ctx = self.ctx
        for k in OPTIONS:
            ctx.set_option(k, opts.get(k, -1))
        hit_t = torch.full((N,), 7.0, device=ctx.device)
        hit_id = torch.full((N,), 7, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda(self.grid[0], self.grid[1], self.grid[2], self.dv, self.df, d_rays, self.active, hit_t, hit_id)
        ctx.synchronize()
        return hit_t.cpu().numpy(), hit_id.cpu().numpy()


@pytest.fixture(scope="module")
def walk(ugrt, O, torch):
    made = {}

    def get(scale, counting=False):
        if (scale, counting) not in made:
            made[scale, counting] = Walk(ugrt, soup(O, scale), ugrt.FLAG_COUNT_WORK if counting else 0)
        return made[scale, counting]

    yield get
    made.clear()


def assert_hits_equal(got, w, R, what):
    t, ids = got
    bad = np.flatnonzero((ids != w[1]) | (bits(t) != bits(w[0])))
    assert bad.size == 0, "%s: %d of %d rays differ (kinds %s), first at pixel %d: id %d t %r, oracle id %d t %r" % (
        what, bad.size, N, np.bincount(R.kind[bad], minlength=6).tolist(), bad[0], ids[bad[0]], t[bad[0]], w[1][bad[0]],
        w[0][bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("scale", sorted(SCALES))
def test_walk_equals_the_oracle(ugrt, O, torch, walk, scale, layout):
    """Ids equal and t bit-equal under the forced cull, the default thresholds and no cull, at every launch shape."""
    R, w = rays_of(O, scale, layout), want(O, scale, layout)
    s = walk(scale)
    d_rays = s.ctx.upload(R.rays.reshape(-1))
    for cull, copts in CULLS.items():
        for shape in SHAPES:
            opts = dict(copts, **shape)
            assert_hits_equal(s.trace(torch, d_rays, **opts), w, R, "%s %s, cull %s, %r" % (scale, layout, cull, shape))
    for k in OPTIONS:
        s.ctx.set_option(k, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("scale", sorted(SCALES))
def test_the_forced_cull_runs(ugrt, O, torch, walk, scale, layout):
    """A counting context under the forced cull: the cull ran (batches, triangles), the results are the oracle's and so
    are the walk's work counts; with the cull off it did not run."""
    R, w = rays_of(O, scale, layout), want(O, scale, layout)
    s = walk(scale, counting=True)
    d_rays = s.ctx.upload(R.rays.reshape(-1))
    assert_hits_equal(s.trace(torch, d_rays, dda_kernel=0, **CULLS["forced"]), w, R, "counting, forced cull")
    st, work = s.ctx.stats_dda(), s.ctx.stats()
    print("%s %s: jobs %d, cull batches %d, triangles culled against a bundle %d" % (
        scale, layout, st["jobs"], st["cull_batches"], st["cull_tests"]))
    assert st["cull_batches"] > 0 and st["cull_tests"] > 0
    assert [int(work[3]), int(work[4]), int(work[5])] == w[2]
    s.trace(torch, d_rays, dda_kernel=0, **CULLS["off"])
    st = s.ctx.stats_dda()
    assert st["jobs"] > 0 and st["cull_batches"] == 0 and st["cull_tests"] == 0
    for k in OPTIONS:
        s.ctx.set_option(k, -1)
