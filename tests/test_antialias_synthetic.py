"""ugrt_aa_edges, ugrt_aa_gather and ugrt_aa_resolve on buffers of their own: every branch and edge.

tests/test_antialias.py compares the three calls with tests/aa_ref.c on the hall and crash frames and with the library's
own offset tables.  Frames hold no pair of neighbours whose cosine or plane distance meets its threshold to the ulp, no
NaN, no lone differing pixel in a corner, no tile that is not square, no offset at 0.5.  Here the calls run on inputs built
with numpy in float64, rounded once to float32, and seeded; the checker is the same tests/aa_ref.c, compared word for word
and byte for byte.  Every image is a multiple of the 8-pixel tile in both directions.

1. ugrt_aa_edges: g-buffers of 64 x 40 and 40 x 24 (a width that is no power of two), ten layouts each, whole image and a
   band (tile rows (1, 3) and (1, 2)) over a sentinel-filled d_edge.  The background is one plane of one material with one
   normal, a triangle id per pixel (neighbours are compared, and the answer is 0).  On it:
     special_*    a lone differing pixel -- a miss, another material, another normal, off the plane, a shadow flag -- at the
                  four corners, in the middle of the four borders, on the band's first and last row and on the rows just
                  outside it; the five reasons rotate over the twelve places from layout to layout.  Flagged: the pixel and
                  its neighbours inside the image, nothing else (each of the eight then sees one differing neighbour, in one
                  of the eight positions)
     lone_*       the same in the interior
     cos_*        neighbours (to the right, below, on either diagonal) whose stored normals, 10 to 15 degrees to either side
                  of the background's, have the float32 dot product (a0 b0 + a1 b1) + a2 b2 equal to normal_cos = 0.9f
                  (on), its predecessor (below), its successor (above); or on one side of it where both contracted forms
                  fma(a2, b2, fma(a0, b0, a1 b1)) and fma(a2, b2, fma(a1, b1, a0 b0)) lie on the other (fma_flags: the
                  spec does not flag, an FMA would; fma_clears: the reverse).  Found by walking one component through its
                  float neighbours.  The run (0.9f, +inf) shows them alone
     plane_*      the same for |np . (Pq - Pp)| against plane_tol = 0.25, P = cam + t dir with and without an FMA: p's normal
                  is 3 degrees off the plane's, q lies a quarter off the plane.  The run (-inf, 0.25) shows them alone
     t+0 t-0 tneg tnan   t of +0, -0, -3 and NaN with a valid id: a miss among hits
     tdenorm      t = 1.4e-45 with a valid id: above 0, a hit at the eye
     tinf         t = +inf with a valid id: a hit whose point is infinite
     id-1 id-2    a valid t with the id -1 and -2: a miss
     nan_normal nan_dir nan_point   a NaN normal component, a NaN direction component, and t = +inf with a zero direction
                  component (P is NaN): a NaN cosine or distance flags nothing, no pixel around them is flagged
     inf_normal inf_dir   infinite components: in the checker's hands
     same_id      a 3 x 3 block of one triangle id whose centre has another normal and depth: no edge
     mat_negative mat_huge   hit triangles whose mat_idx entry is -5, INT_MIN, INT_MAX or 2^20: only compared
     shadow_block*  a 3 x 3 block of is_shadowed words (ring, centre) = (1, 2), (2, -1), (-1, INT_MIN), (INT_MIN, 1) among
                  zeros: the centre is an edge by inequality and none by truth
     shadow_lone*  a lone word of 2, -1, INT_MIN
   Runs: (normal_cos, plane_tol) = (0.9f, +inf), (-inf, 0.25), (0.9f, 0.25), (1, 0), (2, -0), (-1, -1), (+inf, 0.25), each
   with is_shadowed and with the null pointer.  Every id with t > 0 lies inside the face list.
   Checker figures (test_edge_inputs_are_sharp): pixels on which a class occurs (the pixel or one of its neighbours holds
   it): cos_* 180 each, plane_* 144 each, special_* 304 each, lone_* 18 each, shadow_lone2 18, every other class 36;
   neighbour pairs, ordered: cos on 80, below 66, above 40, fma_clears 40, fma_flags 44; plane on 28, below 16, above 25,
   fma_clears 22, fma_flags 23.
2. ugrt_aa_gather: 3 029 triangles in the box [0, 8] x [0, 8] x [-4, 4], uniform grid (8, 8, 4), the eye at (4, 4, -3)
   inside the box looking along +z, image 64 x 40, whole and a band (tile rows (1, 3)) over sentinel-filled sums.  The depth
   gate passes 1.31 <= z < 3.6.
     stacks       twelve cells of the layer z in [0, 2], neighbours sharing faces, with lists of 1, 129, 7, 64, 8, 65 / 63, 9,
                  65, 8, 129, 64: n slats side by side, each half of its strip (rays pass the other half: a long list and no
                  hit), at depths that are a permutation of the list order, 0.02 from the cell's faces, so that the samples
                  of a pixel fall into two lists, or into a list and the gap between them
     duplicates   slat 1 of a list is slat 0 again, slat n - 1 is slat n / 2 again (in the list of 129: in another round of
                  64), with another material; and four pairs of equal triangles across a cell face, in both cells' lists.
                  The checker takes the lower id
     near, crossing   two triangles at z = -0.5 in front of stacks and soup, and one through the eye's plane: the closest
                  hit, which the gate rejects; the sample counts as 0 although a passing triangle lies behind it
     far          three triangles at z = 3.7 to 3.9 behind the far plane (what lies behind them is behind it too)
     materials    the slats of the list of 7 and an eighth of the soup carry mat_idx -1, num_materials, INT_MIN, INT_MAX:
                  the sample counts as 0 and starts no shadow walk
     white        one cell's slats and a triangle in front of the soup carry a material of kd = 4: pixels whose 32 samples are
                  all 255 in the three bytes (the packed sum r | g << 16 at its largest)
     soup         2 400 small triangles in z 2.05 .. 3.55; the first 600 have a vertex (even) or an edge
                  (odd) on the ray of a (pixel, sample) pair of the main table, within the rounding of the vertex
   Tables: the library's eight offsets (the main table); seeded tables of distinct rows per set for the tiles 1 x 1, 4 x 4,
   3 x 2, 2 x 3, 1 x 4, 4 x 1; and the odd table, S = 32: +-0.5, the float neighbours of +-0.5 on both sides, +-0.75,
   +-1e30, +-inf, NaN, -0 and +-1.4e-45 in x against a shifted cycle of them in y, used on every pixel, borders and corners
   included, with and without UGRT_FLAG_STRICT_TEXTURE.  Shadow light: null, inside the grid, far outside, on a vertex of
   a slat, and in the plane z = -0.5 of a near triangle, inside it (every shadow ray meets its occluder at t = 1 to the
   float) with its two float neighbours on either side; eps 1e-3, 0, -1e-3, +inf.  Edge words: ones, zeros, the band's last
   pixel, a checkerboard, and 2, -1, INT_MIN among zeros.  Launch shapes: any_rays_per_wave 1, 7, 31, 32, 64 x any_coop 1,
   8, 2^30 at S = 5 and 31, dda_blocks 1 and 7, arrays that are not the grid's.  The table 0, 4, 8, 12 bytes into an
   allocation, 2 to 1 024 floats (2 S set_w set_h is even: 0 or 2 floats behind the last float4, never 1 or 3;
   tests/test_indirect.py has all four for its table of 3 S floats).
   Checker figures (test_gather_scene_is_sharp; main table, every pixel flagged: 20 480 (pixel, sample) pairs, 36 % hit,
   64 % count as 0, 1 607 pixels mix the two): hits per list length 1: 165, 7: 293, 8: 603, 9: 303, 63: 313, 64: 366, 65:
   525, 129: 500; closest hit rejected by the gate: near 1 880 (861 with a passing triangle behind), crossing 1 470, far
   1 856; mat_idx -1: 121, 5: 130, INT_MIN: 130, INT_MAX: 123; hits on the lower id of equal triangles 1 090, of those
   across a face 617, none on a higher id; aimed pairs that hit their triangle 183, that do not 417; with 32 samples:
   pixels with two list lengths 66, with a list of 63 or more and a miss 640, all 255: 55.
3. ugrt_aa_resolve: 64 x 40, whole and band, every S in 1..32: sums k S + S / 2 - 1, k S + S / 2, k S + S / 2 + 1 and
   k S + (S - 1) / 2 for k in 0, 1, 2, 127, 128, 254, 255; 0; 255 S; 255 S + S / 2 and beyond (the byte wraps, and so
   does the checker's); 2^31; 2^32 - 1 and the sums that the + S / 2 carries past 2^32; count words 0, 1, 2 and
   2^32 - 1 in every pairing.  Bytes outside the band and of count-0 pixels are kept.

CPU tests (unmarked): the conditions above on the checker alone.  GPU tests: exact, no tolerance.
Measured on an MI355X: the 19 GPU tests of this file take 1.3 s together; the slowest are test_edges_equal_the_checker[64x40]
and test_gather_launch_shapes_change_no_word[31] with 0.26 s each (a run of the file with its imports and set-up: 4.6 s).

Sharpness.  Each of the following one-line changes, which keep every access inside its buffer, was built into a scratch
copy of the library (ugrt_aa.hip alone differs) and run once on the MI355X against tests/test_antialias.py (20 GPU tests)
and this file (19).  "new": the tests of this file that fail; "old": those of tests/test_antialias.py.
  cosine < normal_cos -> <=            new: test_edges_equal_the_checker[64x40], [40x24].  old: none
  > plane_tol -> >=                    new: test_edges_equal_the_checker[64x40].  old: test_edges_and_resolve_equal_the_checker
                                       [hall], [crash] (their run with plane_tol = 0, which distances of exactly 0 meet)
  !(fabsf(dist) <= plane_tol)          new: test_edges_equal_the_checker[64x40] (the NaN points, normals and directions).
                                       old: none
  the dx loop starts at 0              new: test_edges_equal_the_checker[64x40], [40x24].  old: 7 (edges, frames, bad arguments)
  is_shadowed compared as truth        new: test_edges_equal_the_checker[64x40] (the centres of the shadow blocks).  old: none
  set_w and set_h swapped in k(p)      new: all 15 test_gather_*.  old: none
  clamp fmaxf(fminf(x, 0.5f), -0.5f)   new: test_gather_odd_offsets[False], [True].  old: none
  the depth gate always passes         new: all 15 test_gather_*.  old: none
  the asmp + off < S guard dropped     new: test_gather_sample_counts_and_tiles[3], [5], [7], [31], test_gather_edge_flags,
                                       test_gather_launch_shapes_change_no_word[5], [31], test_gather_table_alignment.
                                       old: test_gather_equals_the_checker[hall-3], [crash-3], test_launch_shapes_change_no_word
  done = 4 in the float-by-float copy  new: test_gather_table_alignment (it launches the same samples in reverse order from an
                                       aligned table first, so that what stays in LDS is not the table).  old: none
  -ffp-contract=fast for ugrt_aa.hip   new: test_edges_equal_the_checker[64x40], [40x24], test_gather_sample_counts_and_tiles
                                       [8], [32], test_gather_shadow_lights_and_eps.  old: 19 of 20 (every ray direction)
The same changes made in a scratch copy of tests/aa_ref.c (those that have a counterpart there) move, against the checker
on this file's inputs: <= 356 edge words, >= 188, !(<=) 752, dx 3 912, truth 48; swapped tile 3 038 to 5 994 pixels a
sample count; the clamp 2 040 and 2 009 pixels of the odd table; the open gate 3 930 to 5 186 pixels a sample count.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import test_reflect_shadows as RS
from test_antialias import AA, _p, _f32, _i32, _u32, bits  # noqa: F401  (AA: fixture)

F32, F64 = np.float32, np.float64
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
INF, NAN = float("inf"), float("nan")
DENORM = float(np.float32(1e-45))
COS = float(np.float32(0.9))
TOL = 0.25
SENTINEL = -7

# ================================================================================================ 1. ugrt_aa_edges

E_SIZES = {"64x40": (64, 40, (1, 3)), "40x24": (40, 24, (1, 2))}  # width, height, the tile rows of the band context
E_LAYOUTS = 10
E_PITCH = 8
E_CAM = np.array([0.25, -0.5, 1.0], F32)
E_N0 = np.array([0.48, 0.6, 0.64])  # the background plane's normal (a unit vector in float32 too)
REASONS = ("miss", "material", "normal", "plane", "shadow")
# (normal_cos, plane_tol) of the runs; the first isolates the cosine (no plane test can fire), the second the plane
E_RUNS = ((COS, INF), (-INF, TOL), (COS, TOL), (1.0, 0.0), (2.0, -0.0), (-1.0, -1.0), (INF, TOL))
T_ODD = {"t+0": 0.0, "t-0": -0.0, "tdenorm": DENORM, "tneg": -3.0, "tnan": NAN, "tinf": INF}
ULP = ("on", "below", "above", "fma_clears", "fma_flags")
SHADOW_BLOCKS = ((1, 2), (2, -1), (-1, INT_MIN), (INT_MIN, 1))  # (ring, centre) of a 3 x 3 block on a background of 0
SHADOW_LONE = (2, -1, INT_MIN)
PAIR_STEPS = ((1, 0), (0, 1), (1, 1), (-1, 1))
# the classes of the interior sites, dealt in this order over the sites of the ten layouts of an image size
E_CLASSES = (["cos_" + u for u in ULP] * 8 + ["plane_" + u for u in ULP] * 8
             + [k for k in list(T_ODD) + ["id-1", "id-2", "nan_normal", "inf_normal", "nan_dir", "inf_dir", "nan_point", "same_id",
                                          "mat_negative", "mat_huge"] + ["shadow_block%d" % i for i in range(4)]
                + ["shadow_lone%d" % i for i in range(3)] + ["lone_" + r for r in REASONS] for _ in range(2)])


def _next(x, up):
    return np.nextafter(F32(x), F32(INF if up else -INF))


def _dot32(a, b):
    """The spec's order, every operation rounded to float32 (numpy does not contract)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _dot_fma(a, b, first):
    """A contracted evaluation: fma(a2, b2, fma(a_first, b_first, a_other * b_other)).  The products of floats are exact in
    float64 and the sums of like magnitude stay inside 53 bits, so one rounding to float32 per fma."""
    a, b = np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64)
    p = [a[..., k] * b[..., k] for k in range(3)]
    inner = (p[first] + p[1 - first].astype(F32).astype(F64)).astype(F32)
    return (inner.astype(F64) + p[2]).astype(F32)


def _ulp_class(u, fa, fb, c, below_means_flag):
    """The classes of a value u against the threshold c, with its two contracted evaluations: {class: mask}.  A value may
    be in two of them.  below_means_flag: the cosine (u < c flags); else the distance (u > c flags)."""
    c = F32(c)
    flag = (lambda v: v < c) if below_means_flag else (lambda v: v > c)
    return {"on": u == c, "below": u == _next(c, False), "above": u == _next(c, True),
            "fma_flags": ~flag(u) & flag(fa) & flag(fb), "fma_clears": flag(u) & ~flag(fa) & ~flag(fb)}


def _points32(cam, t, d):
    """cam + t * d as the spec forms it, and as an fma forms it."""
    cam, t, d = np.asarray(cam, F32), np.asarray(t, F32), np.asarray(d, F32)
    plain = cam + t[..., None] * d
    fused = (t.astype(F64)[..., None] * d.astype(F64) + cam.astype(F64)).astype(F32)
    return plain, fused


def _perp(rng):
    u = np.cross(E_N0, rng.normal(size=3))
    return u / np.linalg.norm(u)


def _cos_pair(rng, want):
    """Two stored normals, 10 to 15 degrees to either side of the background's, whose dot product is `want` against COS.
    Found by search: the last component of the second walks through its float neighbours."""
    j = np.arange(-60, 61)
    while True:
        u, alpha = _perp(rng), np.radians(rng.uniform(10.0, 15.0))
        beta = np.arccos(0.9) - alpha
        a = (np.cos(alpha) * E_N0 + np.sin(alpha) * u).astype(F32)
        b = np.repeat((np.cos(beta) * E_N0 - np.sin(beta) * u).astype(F32)[None], len(j), 0)
        b[:, 2] = (b[:, 2].view(np.int32) + j.astype(np.int32)).view(F32)
        A = np.repeat(a[None], len(j), 0)
        cls = _ulp_class(_dot32(A, b), _dot_fma(A, b, 0), _dot_fma(A, b, 1), COS, True)
        hit = np.flatnonzero(cls[want])
        if len(hit):
            return a, b[hit[rng.randint(len(hit))]]


def _plane_pair(rng, want, tp, dp, tq0, dq):
    """The normal of p (3 degrees off the background's) and the t of its neighbour q, about TOL off the plane, for which
    |np . (Pq - Pp)| is `want` against TOL.  The last component of the normal walks through its float neighbours."""
    j = np.arange(-300, 301)
    Pp, Ppf = _points32(E_CAM, F32(tp), dp)
    while True:
        u, sign = _perp(rng), rng.choice([-1.0, 1.0])
        a64 = np.cos(np.radians(3.0)) * E_N0 + np.sin(np.radians(3.0)) * u
        # q on its ray where a . (Pq - Pp) = +-TOL
        base = E_CAM.astype(F64) + F64(tq0) * dq.astype(F64) - Pp.astype(F64)
        tq = F32(F64(tq0) + (sign * TOL - a64 @ base) / (a64 @ dq.astype(F64)))
        if not tq > 0:
            continue
        Pq, Pqf = _points32(E_CAM, tq, dq)
        A = np.repeat(a64.astype(F32)[None], len(j), 0)
        A[:, 2] = (A[:, 2].view(np.int32) + j.astype(np.int32)).view(F32)
        diff, diff_f = np.repeat((Pq - Pp)[None], len(j), 0), np.repeat((Pqf - Ppf)[None], len(j), 0)
        cls = _ulp_class(np.abs(_dot32(A, diff)), np.abs(_dot_fma(A, diff_f, 0)), np.abs(_dot_fma(A, diff_f, 1)), TOL, False)
        hit = np.flatnonzero(cls[want])
        if len(hit):
            return A[hit[rng.randint(len(hit))]], tq


def _special_positions(W, H, rows):
    """Where a lone pixel shows an indexing mistake: the corners, the middle of each border, and the band's first and last
    row and the rows just outside them."""
    r0, r1 = rows[0] * 8, rows[1] * 8 - 1
    xm, ym = 8 * (W // 16) + 4, 8 * (H // 16) + 4  # (on the columns and rows of the sites: fewer sites give way)
    cols = [12, 28, 44, 52] if W >= 64 else [12, 20, 28, 12]
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (xm, 0), (xm, H - 1), (0, ym), (W - 1, ym),
            (cols[0], r0 - 1), (cols[1], r0), (cols[2], r1), (cols[3], r1 + 1)]


@functools.lru_cache(maxsize=None)
def edge_inputs(size):
    """The ten layouts of an image size: g-buffers over one plane of one material, with the cases on it.  -> a list of
    namespaces (normal, t, dir, id, mat_idx, shadowed, sites); sites: (class, x, y, pixels).  Computed once and shared:
    nobody writes to it."""
    W, H, rows = E_SIZES[size]
    N = W * H
    rng = np.random.RandomState(611 + W)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    d64 = np.stack([((xs + 0.5) / W - 0.5) * 1.2, ((ys + 0.5) / H - 0.5) * 0.8, -np.ones((H, W))], -1).reshape(N, 3)
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    dirs = d64.astype(F32)
    t_plane = ((-4.0 - E_N0 @ E_CAM.astype(F64)) / (dirs.astype(F64) @ E_N0)).astype(F32)
    assert (t_plane > 1).all() and (t_plane < 100).all()
    special = _special_positions(W, H, rows)
    centres = [(x, y) for y in range(4, H - 3, E_PITCH) for x in range(4, W - 3, E_PITCH)
               if all(abs(x - sx) > 4 or abs(y - sy) > 4 for sx, sy in special)]
    deal = 0
    layouts = []
    for layout in range(E_LAYOUTS):
        g = types.SimpleNamespace(W=W, H=H, N=N, rows=rows, normal=np.repeat(E_N0.astype(F32)[None], N, 0), t=t_plane.copy(),
                                  dir=dirs.copy(), id=np.arange(N, dtype=np.int32), mat_idx=np.zeros(N + 8, np.int32),
                                  shadowed=np.zeros(N, np.int32), sites=[], cam=E_CAM)
        # ids N .. N + 7: triangles of other materials, in range, negative and huge
        g.mat_idx[N:] = [1, 2, -5, INT_MIN, INT_MAX, 1 << 20, 0, 0]

        def lone(p, reason):
            if reason == "miss":
                g.id[p], g.t[p] = -2, -1.0
            elif reason == "material":
                g.id[p] = N
            elif reason == "normal":
                g.normal[p] = [0.96, 0.0, 0.28]  # cosine 0.64
            elif reason == "plane":
                g.t[p] *= F32(1.5)
            else:
                g.shadowed[p] = 1

        for i, (x, y) in enumerate(special):
            reason = REASONS[(i + layout) % 5]
            lone(y * W + x, reason)
            g.sites.append(("special_" + reason, x, y, (y * W + x,)))
        for x, y in centres:
            cls = E_CLASSES[deal % len(E_CLASSES)]
            deal += 1
            p = y * W + x
            sx, sy = PAIR_STEPS[deal % 4]
            q = (y + sy) * W + x + sx
            pixels = (p,)
            if cls.startswith("cos_"):
                g.normal[p], g.normal[q] = _cos_pair(rng, cls[4:])
                pixels = (p, q)
            elif cls.startswith("plane_"):
                g.normal[p], g.t[q] = _plane_pair(rng, cls[6:], g.t[p], g.dir[p], g.t[q], g.dir[q])
                pixels = (p, q)
            elif cls in T_ODD:
                g.t[p] = T_ODD[cls]
            elif cls in ("id-1", "id-2"):
                g.id[p] = int(cls[2:])
            elif cls == "nan_normal":
                g.normal[p, deal % 3] = NAN
            elif cls == "inf_normal":
                g.normal[p, deal % 3] = INF if deal % 2 else -INF
            elif cls == "nan_dir":
                g.dir[p, deal % 3] = NAN
            elif cls == "inf_dir":
                g.dir[p, deal % 3] = INF if deal % 2 else -INF
            elif cls == "nan_point":  # t = +inf times a zero direction component
                g.t[p], g.dir[p, deal % 3] = INF, 0.0
            elif cls == "same_id":  # a 3 x 3 block of one triangle id; its centre has another normal and lies off the plane
                for dy in (-1, 0, 1):
                    g.id[p + dy * W - 1:p + dy * W + 2] = p
                g.normal[p], g.t[p] = [0.0, -0.6, 0.8], g.t[p] * F32(0.7)
            elif cls == "mat_negative":
                g.id[p] = N + 2 + deal % 2
            elif cls == "mat_huge":
                g.id[p] = N + 4 + deal % 2
            elif cls.startswith("shadow_block"):
                ring, centre = SHADOW_BLOCKS[int(cls[-1])]
                for dy in (-1, 0, 1):
                    g.shadowed[p + dy * W - 1:p + dy * W + 2] = ring
                g.shadowed[p] = centre
            elif cls.startswith("shadow_lone"):
                g.shadowed[p] = SHADOW_LONE[int(cls[-1])]
            else:
                lone(p, cls[5:])
            g.sites.append((cls, x, y, pixels))
        assert ((g.id < N + 8) & ((g.id >= 0) | (g.id == -1) | (g.id == -2))).all()  # mat_idx[id] is read where t > 0
        g.pr = dict(normal=g.normal.reshape(-1), t=g.t, dir=g.dir.reshape(-1), id=g.id)
        layouts.append(g)
    return layouts


def cpu_edge(AA, g, run, with_shadows, p0=0, n=None, fill=0):
    return AA.edges(g.pr, g.cam, g.mat_idx, g.shadowed if with_shadows else None, run[0], run[1], g.W, g.H, p0,
                    g.N if n is None else n, fill)


def _around(g, x, y, r):
    """The pixels of the image at Chebyshev distance <= r of (x, y)."""
    return [yy * g.W + xx for yy in range(max(0, y - r), min(g.H, y + r + 1)) for xx in range(max(0, x - r), min(g.W, x + r + 1))]


def _pair_values(g, p, q):
    """What the spec computes for the ordered pair (p, q): cosine, |dist|, and their contracted evaluations."""
    Pp, Ppf = _points32(g.cam, g.t[p], g.dir[p])
    Pq, Pqf = _points32(g.cam, g.t[q], g.dir[q])
    a, b = g.normal[p], g.normal[q]
    return (_dot32(a, b), _dot_fma(a, b, 0), _dot_fma(a, b, 1),
            np.abs(_dot32(a, Pq - Pp)), np.abs(_dot_fma(a, Pqf - Ppf, 0)), np.abs(_dot_fma(a, Pqf - Ppf, 1)))


def test_edge_inputs_are_sharp(AA):
    """CPU, the checker alone: every class occurs on at least 16 pixels (a pixel counts where it or one of its neighbours
    holds the class), every ulp class on at least 8 neighbour pairs, a lone pixel flags exactly itself and its neighbours
    inside the image, and the classes behave as section 6.11 says."""
    pixels, pairs = {}, {}
    for size in E_SIZES:
        for g in edge_inputs(size):
            both = cpu_edge(AA, g, (COS, TOL), True)
            cos_run, plane_run = cpu_edge(AA, g, E_RUNS[0], False), cpu_edge(AA, g, E_RUNS[1], False)
            assert set(np.unique(both)) == {0, 1} and 0.02 < both.mean() < 0.6
            for cls, x, y, px in g.sites:
                zone = _around(g, x, y, 1)
                pixels[cls] = pixels.get(cls, 0) + len(zone)
                p = px[0]
                if cls.startswith("special_") or cls.startswith("lone_"):
                    # exactly the pixel and its in-image neighbours
                    assert both[zone].all(), (size, cls, x, y)
                    assert not both[sorted(set(_around(g, x, y, 2)) - set(zone))].any(), (size, cls, x, y)
                    reason = cls.split("_")[1]
                    bare = cpu_edge(AA, g, (COS, TOL), False)
                    assert bare[zone].all() == (reason != "shadow")
                    assert cos_run[zone].all() == (reason in ("miss", "material", "normal"))
                    if reason != "normal":  # (the other normal also moves the plane through the pixel)
                        assert plane_run[zone].all() == (reason in ("miss", "material", "plane"))
                elif cls.startswith("cos_") or cls.startswith("plane_"):
                    q = px[1]
                    for a, b in ((p, q), (q, p)):
                        u, fa, fb, d, da, db = _pair_values(g, a, b)
                        for name, c in (("cos_", _ulp_class(u, fa, fb, COS, True)), ("plane_", _ulp_class(d, da, db, TOL, False))):
                            for k, v in c.items():
                                pairs[name + k] = pairs.get(name + k, 0) + int(v)
                    u, fa, fb, d, da, db = _pair_values(g, p, q)
                    if cls.startswith("cos_"):  # p is flagged in the cosine's run exactly where the float32 cosine is below COS
                        assert _ulp_class(u, fa, fb, COS, True)[cls[4:]]
                        assert cos_run[p] == int(u < F32(COS)) == int(cls[4:] in ("below", "fma_clears")), (size, cls, x, y)
                        if cls.startswith("cos_fma"):
                            assert (fa < F32(COS)) == (fb < F32(COS)) != (u < F32(COS))
                    else:
                        assert _ulp_class(d, da, db, TOL, False)[cls[6:]]
                        assert plane_run[p] == int(d > F32(TOL)) == int(cls[6:] in ("above", "fma_clears")), (size, cls, x, y)
                        if cls.startswith("plane_fma"):
                            assert (da > F32(TOL)) == (db > F32(TOL)) != (d > F32(TOL))
                elif cls in T_ODD or cls in ("id-1", "id-2"):
                    # a miss among hits; the smallest denormal is above 0, a hit at the eye, which only the plane test sees,
                    # and t = +inf a hit whose point is infinite: a NaN distance
                    if cls == "tdenorm":
                        assert not cos_run[zone].any() and plane_run[zone].all()
                    elif cls != "tinf":
                        assert both[zone].all() and cos_run[zone].all()
                elif cls in ("nan_normal", "nan_dir", "nan_point"):
                    assert not both[zone].any(), (size, cls, x, y)  # a NaN cosine or distance flags nothing
                elif cls == "same_id":
                    assert not both[p] and not both[zone].any()
                elif cls.startswith("mat_"):
                    assert both[zone].all() and cos_run[zone].all()
                elif cls.startswith("shadow_block"):
                    assert both[zone].all() and not cpu_edge(AA, g, (COS, TOL), False)[zone].any()
                    # compared as truth values the centre would equal its ring
                    truth = cpu_edge(AA, types.SimpleNamespace(**{**vars(g), "shadowed": (g.shadowed != 0).astype(np.int32)}),
                                     (COS, TOL), True)
                    assert truth[p] == 0 and both[p] == 1
                elif cls.startswith("shadow_lone"):
                    assert both[zone].all()
            # the thresholds that nothing or everything passes
            hit = (g.t > 0) & (g.id >= 0)
            assert cpu_edge(AA, g, (INF, TOL), False).sum() > 0.9 * hit.sum()
            never = cpu_edge(AA, g, (-INF, INF), False)
            assert never.sum() < both.sum()
    print("pixels per class", sorted(pixels.items()))
    print("neighbour pairs per ulp class", sorted(pairs.items()))
    assert set(pixels) >= set(E_CLASSES) | {"special_" + r for r in REASONS}
    assert min(pixels.values()) >= 16, pixels
    assert set(pairs) >= {k + u for k in ("cos_", "plane_") for u in ULP} and min(pairs.values()) >= 8, pairs


# ================================================================================================ 2. ugrt_aa_gather

G_W, G_H, G_ROWS = 64, 40, (1, 3)
G_N = G_W * G_H
G_P0, G_NB = G_ROWS[0] * 8 * G_W, (G_ROWS[1] - G_ROWS[0]) * 8 * G_W
# The eye stands inside the grid's box [0, 8] x [0, 8] x [-4, 4] and looks along +z.  The depth gate passes the hits with
# 2 far near / (far + near) <= depth < far, that is -3 + 4.31 = 1.31 <= z < 3.6.
G_EYE = dict(eye=(4.0, 4.0, -3.0), look=(4.0, 4.0, 1.0), up=(0.0, 1.0, 0.0), near=3.2, far=6.6)
G_Z = (1.31, 3.6)
# cell (i, j) of the layer k = 2 (z in [0, 2]): the length of its list.  Neighbours in a row share a cell face.
G_STACKS = {(1, 3): 1, (2, 3): 129, (3, 3): 7, (4, 3): 64, (5, 3): 8, (6, 3): 65,
            (1, 4): 63, (2, 4): 9, (3, 4): 65, (4, 4): 8, (5, 4): 129, (6, 4): 64}
G_WHITE_CELL = (4, 3)
G_STRADDLE = ((3, 2), (5, 2), (3, 5), (5, 5))  # (x of the cell face, row j): two equal triangles across the face
G_K = 5  # materials; the last is the white one
G_ODD_MATS = (-1, G_K, INT_MIN, INT_MAX)
G_NSOUP, G_NAIMED = 2400, 600
G_LIGHT = np.array([2.0, 7.0, -2.0], F32)  # the shading light
G_SHADOW_IN, G_SHADOW_FAR = np.array([3.3, 4.6, 0.2], F32), np.array([60.0, -45.0, -80.0], F32)
G_T1 = np.array([4.9, 4.5, -0.5], F32)  # inside the second near triangle, in its plane to the float
G_EPS = (1e-3, 0.0, -1e-3, INF)
G_S = (1, 2, 3, 5, 7, 8, 31, 32)
G_TILES = ((1, 1), (4, 4), (3, 2), (2, 3), (1, 4), (4, 1))
ODD_OFFSETS = [0.5, -0.5, _next(0.5, True), _next(0.5, False), _next(-0.5, True), _next(-0.5, False), 0.75, -0.75, 1e30, -1e30,
               INF, -INF, NAN, -0.0, DENORM, -DENORM]


def directions(AA, cam, strict, fcol, frow):
    fcol, frow = _f32(fcol), _f32(frow)
    d = np.zeros(3 * len(fcol), F32)
    AA.lib.aa_directions(_p(_f32(cam.cc)), _p(_f32(cam.tex)), C.c_int(G_W), C.c_int(G_H), C.c_int(1 if strict else 0),
                         C.c_int(len(fcol)), _p(fcol), _p(frow), _p(d))
    return d.reshape(-1, 3)


def clamp_offsets(table):
    """The spec's clamp: outside [-0.5, 0.5] is clamped, a NaN counts as -0.5."""
    t = np.where(np.isnan(table), F32(-0.5), table)
    return np.clip(t, F32(-0.5), F32(0.5)).astype(F32)


def main_table(ugrt):
    return ugrt.scenes.aa_offsets(8).reshape(1, 8, 2)


def random_table(S, tile, seed=0):
    """Distinct rows per set, seeded."""
    return np.random.RandomState(1000 * seed + 100 * S + 10 * tile[0] + tile[1]).uniform(-0.5, 0.5, (tile[0] * tile[1], S, 2)) \
        .astype(F32)


def odd_table():
    """S = 32, one set: the odd values in x against a shifted cycle of them in y, and ordinary entries between them."""
    rng = np.random.RandomState(77)
    t = rng.uniform(-0.5, 0.5, (1, 32, 2)).astype(F32)
    odd = np.array(ODD_OFFSETS, F32)
    t[0, :16, 0] = odd
    t[0, 8:24, 1] = np.roll(odd, 5)
    return t


_GS = {}


def gscene(O, ugrt, AA):
    """The synthetic scene, its grid, the eye and the state of the context.  Computed once and shared: nobody writes to it."""
    if _GS:
        return _GS["g"]
    rng = np.random.RandomState(20261021)
    cam = O.cam_from(G_EYE, 45.0, float(F32(G_W) / F32(G_H)))
    eye = cam.cc[:3].astype(F64)
    tris, mats, kind = [], [], {}

    def add(v, m, k):
        kind.setdefault(k, []).append(len(tris))
        tris.append(np.asarray(v, F64))
        mats.append(m)
        return len(tris) - 1

    add([(0, 0, -4), (0.01, 0, -4), (0, 0.01, -4)], 0, "anchor")
    stacks, dup_of = {}, {}
    for (i, j), n in G_STACKS.items():
        # n slats along x, side by side in y, each at a depth of its own (the list is in ascending id, the depths are not)
        order = rng.permutation(n)
        first = len(tris)
        dups = {} if n < 2 else ({1: 0} if n < 4 else {1: 0, n - 1: n // 2})
        for m in range(n):
            src = dups.get(m, m)
            y0, y1 = j + 0.02 + 0.96 * src / n, j + 0.02 + 0.96 * (src + 1) / n
            z = 1.4 + 0.5 * order[src] / n
            v = [(i + 0.02, y0, z), (i + 0.98, y0, z), (i + 0.02, y1, z)] if src % 2 == 0 else \
                [(i + 0.98, y1, z), (i + 0.02, y1, z), (i + 0.98, y0, z)]
            if (i, j) == G_WHITE_CELL:
                mat = G_K - 1
            elif n == 7:
                mat = (G_ODD_MATS + (0, 1, 2))[m]
            else:
                mat = int(rng.randint(0, 4))
            if m in dups:
                mat = (mats[first + src] + 1) % 4 if 0 <= mats[first + src] < 4 else 0
                dup_of[first + m] = first + src
            add(v, mat, "stack%d" % n)
        stacks[(i, j)] = (first, n)
    for xb, j in G_STRADDLE:
        v = [(xb - 0.3, j + 0.2, 1.5), (xb + 0.3, j + 0.2, 1.5), (xb - 0.1, j + 0.8, 1.5)]
        a = add(v, 0, "straddle")
        dup_of[add(v, 1, "straddle")] = a
    # in front of the gate's near distance, each with stacks or soup behind it; one crosses the eye's plane
    add([(2.5, 3.2, -0.5), (3.6, 3.2, -0.5), (2.5, 3.9, -0.5)], 0, "near")
    add([(4.6, 4.3, -0.5), (5.5, 4.3, -0.5), (4.6, 4.9, -0.5)], 1, "near")
    add([(4.25, 4.05, -3.5), (4.5, 4.2, -2.0), (4.35, 3.9, -2.0)], 2, "crossing")
    # the white material, in front of the soup: pixels whose samples are all 255 in the three bytes
    add([(1.0, 5.0, 2.02), (3.0, 5.0, 2.02), (1.0, 5.9, 2.02)], G_K - 1, "white")
    # behind the far plane, the closest hit where the soup has a gap
    add([(1.0, 1.5, 3.8), (7.0, 1.5, 3.8), (1.0, 3.0, 3.8)], 0, "far")
    add([(1.0, 1.5, 3.9), (7.0, 1.5, 3.9), (1.0, 3.0, 3.9)], 1, "far")
    add([(7.0, 6.5, 3.7), (1.0, 6.5, 3.7), (7.0, 5.0, 3.7)], 2, "far")
    # the soup of the layer k = 3; its first G_NAIMED triangles have a vertex or an edge on a ray of the main table
    table = main_table(ugrt)
    aim_p = rng.randint(0, G_N, G_NAIMED)
    aim_s = rng.randint(0, 8, G_NAIMED)
    aim_d = directions(AA, cam, False, (aim_p % G_W) + table[0, aim_s, 0], (aim_p // G_W) + table[0, aim_s, 1]).astype(F64)
    aimed = []
    for s in range(G_NSOUP):
        size = np.exp(rng.uniform(np.log(0.06), np.log(0.25)))
        off = rng.normal(size=(3, 3)) * 0.5 * size
        off[:, 2] *= 0.3
        if s < G_NAIMED:
            zc = rng.uniform(2.4, 3.3)
            P = eye + (zc - eye[2]) / aim_d[s, 2] * aim_d[s]
            if s % 2 == 0:
                v = np.array([P, P + off[1], P + off[2]])  # a vertex on the ray
            else:
                v = np.array([P + off[0], P - rng.uniform(0.3, 3.0) * off[0], P + off[2]])  # an edge through the ray
        else:
            v = rng.uniform([0.3, 1.0, 2.4], [7.7, 7.0, 3.3]) + off
        v[:, 2] = np.clip(v[:, 2], 2.05, 3.55)
        v[:, :2] = np.clip(v[:, :2], 0.02, 7.98)  # (inside the anchors' box)
        mat = int(rng.randint(0, 4)) if rng.rand() > 0.125 else int(rng.choice(G_ODD_MATS))
        t = add(v, mat, "soup")
        if s < G_NAIMED:
            aimed.append((int(aim_p[s]), int(aim_s[s]), t))
    add([(8, 8, 4), (7.99, 8, 4), (8, 7.99, 4)], 0, "anchor")
    verts = np.asarray(tris, F64).reshape(-1, 3).astype(F32)
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    mat_list = np.concatenate([rng.uniform(0.1, 0.9, (G_K - 1, 6)), [[0.2, 0.2, 0.2, 4.0, 4.0, 4.0]]]).astype(F32)
    grid = O.grid_uniform(faces, verts, verts.min(0), verts.max(0), RS.SYN_DIMS)
    g = types.SimpleNamespace(verts=verts, faces=faces, mat_idx=np.asarray(mats, np.int32), mat_list=mat_list, grid=grid, cam=cam,
                              kind={k: np.asarray(v) for k, v in kind.items()}, stacks=stacks, dup_of=dup_of, aimed=aimed,
                              sums={}, F=len(faces))
    _GS["g"] = g
    return g


def gsums(AA, g, edge, S, tile, table, shadow_light=None, eps=1e-3, strict=False, p0=0, n=G_N, fill=0, detail=False):
    key = (_i32(edge).tobytes(), S, tile, bits(table).tobytes(),
           None if shadow_light is None else bits(shadow_light).tobytes(), bits(F32(eps)).tobytes(), strict, p0, n, fill)
    if detail or key not in g.sums:
        out = AA.gather(g.grid, g.verts, g.faces, g.cam, strict, G_W, G_H, edge, S, tile, table, g.mat_idx, g.mat_list, g.cam.cc,
                        G_LIGHT, shadow_light, eps, p0, n, fill, detail)
        if detail:
            return out
        g.sums[key] = out
    return g.sums[key]


ONES = np.ones(G_N, np.int32)


def edge_forms():
    rng = np.random.RandomState(3)
    last = np.zeros(G_N, np.int32)
    last[G_P0 + G_NB - 1] = 1
    xs, ys = np.meshgrid(np.arange(G_W), np.arange(G_H))
    return (("ones", ONES), ("zeros", np.zeros(G_N, np.int32)), ("last", last),
            ("checkerboard", ((xs + ys) % 2).astype(np.int32).reshape(-1)),
            ("values", rng.choice(np.array([0, 2, -1, INT_MIN], np.int64), G_N).astype(np.int32)))


def t1_lights():
    """The light in the plane of a triangle, and its float neighbours to either side of the plane."""
    z = G_T1[2].view(np.int32)
    return [np.array([G_T1[0], G_T1[1], (z + k).astype(np.int32).view(F32)], F32) for k in (2, 1, 0, -1, -2)]  # (z < 0)


def test_gather_scene_is_sharp(ugrt, O, AA):
    """CPU, the checker alone: the list lengths, and every input class in at least 64 (pixel, sample) pairs of the main
    table (S = 8, every pixel flagged)."""
    g = gscene(O, ugrt, AA)
    dims = RS.SYN_DIMS
    assert 3000 <= g.F <= 4000
    for (i, j), (first, n) in g.stacks.items():
        cell = (i * dims[1] + j) * dims[2] + 2
        assert int(g.grid["span"][cell]) == n
        off = int(g.grid["offset"][cell])
        np.testing.assert_array_equal(g.grid["vals"][off:off + n], np.arange(first, first + n))
    table = main_table(ugrt)
    S = 8
    sums, (ht, hid) = gsums(AA, g, ONES, S, (1, 1), table, detail=True)
    # every ray again, against every triangle
    p = np.arange(G_N)
    rays = np.zeros((S, G_N, 6), F32)
    for s in range(S):
        rays[s, :, :3] = g.cam.cc[:3]
        rays[s, :, 3:] = directions(AA, g.cam, False, (p % G_W) + table[0, s, 0], (p // G_W) + table[0, s, 1])
    M = S * G_N
    bt, bid = O.brute_nearest(g.verts, g.faces, rays.reshape(-1), np.ones(M, np.int32), 0, M, M)
    bt, bid = bt.reshape(S, G_N), bid.reshape(S, G_N)
    z = g.cam.cc[2] + bt * rays[:, :, 5]
    passes = (bid >= 0) & (z >= G_Z[0] + 1e-3) & (z < G_Z[1] - 1e-3)
    rejected = (bid >= 0) & ((z < G_Z[0] - 1e-3) | (z > G_Z[1] + 1e-3))
    assert (hid[passes] >= 0).all() and (bits(ht[passes]) == bits(bt[passes])).all() and (hid[rejected] == -2).all()
    counts = {}
    for n in set(G_STACKS.values()):
        counts["list%d" % n] = int(np.isin(hid, g.kind["stack%d" % n]).sum())
    for k in ("near", "far", "crossing"):
        counts["gate_" + k] = int((np.isin(bid, g.kind[k]) & (hid == -2)).sum())
    # behind a rejected near triangle: the closest of the others passes the gate
    others = np.ones(g.F, bool)
    others[np.concatenate([g.kind["near"], g.kind["crossing"]])] = False
    sel = np.isin(bid, g.kind["near"])
    t2, id2 = O.brute_nearest(g.verts, g.faces[others], rays.reshape(-1), sel.reshape(-1).astype(np.int32), 0, M, M)
    z2 = g.cam.cc[2] + t2.reshape(S, G_N) * rays[:, :, 5]
    counts["passing_behind_near"] = int((sel & (id2.reshape(S, G_N) >= 0) & (z2 > G_Z[0]) & (z2 < G_Z[1])).sum())
    hit = hid >= 0
    for m in G_ODD_MATS:
        counts["mat%d" % m] = int((hit & (g.mat_idx[np.maximum(hid, 0)] == m)).sum())
    lows = np.array(sorted(set(g.dup_of.values())))
    counts["duplicate_lower_id"] = int(np.isin(hid, lows).sum())
    assert not np.isin(hid, np.array(sorted(g.dup_of))).any()  # of two equal triangles the checker takes the lower id
    counts["duplicate_across_a_face"] = int(np.isin(hid, g.kind["straddle"]).sum())
    ap, as_, at = (np.array(x) for x in zip(*g.aimed))
    counts["aimed_hit"] = int((hid[as_, ap] == at).sum())
    counts["aimed_not_hit"] = int((hid[as_, ap] != at).sum())
    # within a pixel: lists of different lengths and misses
    s32, (_, hid32) = gsums(AA, g, ONES, 32, (1, 1), random_table(32, (1, 1)), detail=True)
    length = np.zeros(g.F + 2, np.int32)
    for (i, j), (first, n) in g.stacks.items():
        length[first:first + n] = n
    L = length[hid32]
    mixed = [(L == n).any(0) for n in sorted(set(G_STACKS.values()))]
    counts["pixels_with_two_list_lengths"] = int((np.sum(mixed, 0) >= 2).sum())
    counts["pixels_with_a_long_list_and_a_miss"] = int(((L >= 63).any(0) & (hid32 == -2).any(0)).sum())
    counts["pixels_all_255"] = int((s32.reshape(G_N, 4)[:, :3] == 255 * 32).all(1).sum())
    share_hit, share_miss = float(hit.mean()), float((hid == -2).mean())
    counts["pixels_mixing_hit_and_miss"] = int((hit.any(0) & ~hit.all(0)).sum())
    print("gather classes", sorted(counts.items()), "hit share", share_hit, "miss share", share_miss)
    low = {k: v for k, v in counts.items() if v < (16 if k.startswith("pixels") else 64)}
    assert not low, low
    assert share_hit >= 0.25 and share_miss >= 0.1 and counts["pixels_mixing_hit_and_miss"] >= 64


def test_gather_tables_are_sharp(ugrt, O, AA):
    """CPU: a non-square tile and its transpose give different words on many pixels; clamped, NaN and exact +-0.5 offsets
    change words on border pixels; the light in a triangle's plane is neither of its neighbours."""
    g = gscene(O, ugrt, AA)
    for tile in G_TILES:
        if tile[0] == tile[1]:
            continue
        table = random_table(8, tile)
        a = gsums(AA, g, ONES, 8, tile, table).reshape(G_N, 4)
        b = gsums(AA, g, ONES, 8, tile[::-1], table).reshape(G_N, 4)
        assert int((a != b).any(1).sum()) > G_N // 8, tile
    odd = odd_table()
    xs, ys = np.meshgrid(np.arange(G_W), np.arange(G_H))
    border = ((xs == 0) | (xs == G_W - 1) | (ys == 0) | (ys == G_H - 1)).reshape(-1)
    kinds = {"clamped": np.abs(odd) > 0.5, "nan": np.isnan(odd), "half": np.abs(odd) == 0.5}
    for strict in (False, True):
        full = gsums(AA, g, ONES, 32, (1, 1), odd, strict=strict).reshape(G_N, 4)
        assert (full[:, 3] == 1).all()
        np.testing.assert_array_equal(full.reshape(-1), gsums(AA, g, ONES, 32, (1, 1), clamp_offsets(odd), strict=strict))
        for name, mask in kinds.items():
            assert mask.sum() >= 2
            zeroed = np.where(mask, F32(0), odd)
            w = gsums(AA, g, ONES, 32, (1, 1), zeroed, strict=strict).reshape(G_N, 4)
            assert int(((w != full).any(1) & border).sum()) >= 16, (name, strict)
    words = [gsums(AA, g, ONES, 8, (1, 1), main_table(ugrt), L).reshape(G_N, 4) for L in t1_lights()[1:4]]
    assert int((words[0] != words[1]).any(1).sum()) >= 64 and int((words[1] != words[2]).any(1).sum()) >= 64
    # eps moves the shadow ray's origin: each value gives words of its own
    e = [gsums(AA, g, ONES, 8, (1, 1), main_table(ugrt), G_SHADOW_IN, eps) for eps in G_EPS]
    for i in range(4):
        for j in range(i):
            assert (e[i] != e[j]).any(), (G_EPS[i], G_EPS[j])


# ================================================================================================ 3. ugrt_aa_resolve

R_W, R_H, R_ROWS = 64, 40, (1, 3)
R_COUNTS = (0, 1, 2, 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def resolve_inputs(S):
    """[4N] words: the sums of every rounding boundary k S + S / 2 - 1 and k S + S / 2 for a few k, 0, 255 S, 255 S + S / 2
    and beyond, 2^32 - 1, dealt over the three bytes, in every pairing with the count words 0, 1, 2 and 2^32 - 1."""
    N = R_W * R_H
    ks = (0, 1, 2, 127, 128, 254, 255)
    values = [0, 255 * S, 255 * S + S // 2, 255 * S + S // 2 + 1, 256 * S, 256 * S + S // 2, 300 * S + 7, 2 ** 31, 2 ** 32 - S,
              2 ** 32 - 1 - S // 2, 2 ** 32 - 1]
    for k in ks:
        values += [k * S + S // 2 - 1, k * S + S // 2, k * S + S // 2 + 1, k * S + (S - 1) // 2, k * S]
    values = np.array([v % 2 ** 32 for v in values], np.uint64).astype(np.uint32)
    rng = np.random.RandomState(7 + S)
    sums = np.zeros((N, 4), np.uint32)
    m = len(values)
    i = np.arange(N)
    sums[:, 0] = values[i % m]
    sums[:, 1] = values[(i // m + i) % m]
    sums[:, 2] = values[rng.randint(0, m, N)]
    sums[:, 3] = np.array(R_COUNTS, np.uint32)[(i // (m * m // 8 + 1) + i // 3) % 4]
    img = rng.randint(0, 256, 3 * N).astype(np.uint8)
    return sums.reshape(-1), img


def test_resolve_inputs_are_sharp(AA):
    """CPU: on the checker the boundaries round as (sum + S / 2) / S says, count words other than 0 write, sums above
    255 S wrap in the byte, and every pairing of a class of sums with a count word occurs."""
    N = R_W * R_H
    for S in range(1, 33):
        sums, img = resolve_inputs(S)
        w = sums.reshape(N, 4).astype(np.uint64)
        out = AA.resolve(img, sums, S, 0, N).reshape(N, 3)
        keep = w[:, 3] == 0
        for c in R_COUNTS:
            assert int((w[:, 3] == c).sum()) > N // 8
        np.testing.assert_array_equal(out[keep], img.reshape(N, 3)[keep])
        want = (((w[:, :3] + S // 2) % 2 ** 32) // S % 256).astype(np.uint8)
        np.testing.assert_array_equal(out[~keep], want[~keep])
        for c in R_COUNTS[1:]:
            sel = w[:, 3] == c
            v = w[sel, :3]
            assert ((v % S == (S // 2 - 1) % S) & (v < 256 * S)).sum() >= 16 and (v % S == S // 2).sum() >= 16
            assert (v == 0).sum() >= 4 and (v == 255 * S).sum() >= 4 and (v > 255 * S + S // 2).sum() >= 16
            assert (v == 2 ** 32 - 1).sum() >= 4
        # rounding half up: k S + S / 2 gives k + 1 (even S: the exact half), one less gives k
        sel = ~keep
        v = w[sel, 0]
        if S % 2 == 0:
            up, down = (v % S == S // 2) & (v < 255 * S), (v % S == S // 2 - 1) & (v < 255 * S)
            np.testing.assert_array_equal(out[sel, 0][up], (v[up] // S + 1).astype(np.uint8))
            np.testing.assert_array_equal(out[sel, 0][down], (v[down] // S).astype(np.uint8))
        band = AA.resolve(img, sums, S, 8 * R_W * R_ROWS[0], 8 * R_W * (R_ROWS[1] - R_ROWS[0]))
        assert (band[:24 * R_W * R_ROWS[0]] == img[:24 * R_W * R_ROWS[0]]).all()
        assert (band[24 * R_W * R_ROWS[1]:] == img[24 * R_W * R_ROWS[1]:]).all() and (band != img).sum() > N // 4


# ================================================================================================ GPU

@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(E_SIZES))
def test_edges_equal_the_checker(ugrt, AA, torch, size):
    """Ten layouts, seven (normal_cos, plane_tol), with the shadow flags and with the null pointer, on the whole image and
    on a band whose neighbours' rows decide flags inside it: the checker's words, pixels outside the band untouched."""
    W, H, rows = E_SIZES[size]
    N = W * H
    flagged = 0
    for rows_ in (None, rows):
        ctx = ugrt.Context(W, H, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS, rows=rows_)
        p0, n = ctx.p0, ctx.npix
        assert (p0, n) == ((0, N) if rows_ is None else (rows[0] * 8 * W, (rows[1] - rows[0]) * 8 * W))
        for li, g in enumerate(edge_inputs(size)):
            d = [ctx.upload(a) for a in (g.pr["normal"], g.t, g.pr["dir"], g.id, g.cam, g.mat_idx, g.shadowed)]
            for run in E_RUNS:
                for with_shadows in (True, False):
                    edge = torch.full((N,), SENTINEL, dtype=torch.int32, device=ctx.device)
                    ctx.aa_edges(*d[:6], d[6] if with_shadows else None, run[0], run[1], edge)
                    ctx.synchronize()
                    want = cpu_edge(AA, g, run, with_shadows, p0, n, fill=SENTINEL)
                    np.testing.assert_array_equal(edge.cpu().numpy(), want,
                                                  err_msg="%s layout %d cos %g tol %g shadows %s rows %s"
                                                  % (size, li, run[0], run[1], with_shadows, rows_))
                    flagged += int((want == 1).sum())
    assert flagged > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("half", [0, 1])
def test_resolve_equals_the_checker(ugrt, AA, torch, half):
    """Every S (half 0: 1..16, half 1: 17..32), whole image and band: the checker's bytes."""
    N = R_W * R_H
    for rows in (None, R_ROWS):
        ctx = ugrt.Context(R_W, R_H, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS, rows=rows)
        p0, n = ctx.p0, ctx.npix
        for S in range(1 + 16 * half, 17 + 16 * half):
            sums, img = resolve_inputs(S)
            d_img = ctx.upload(img)
            ctx.aa_resolve(d_img, ctx.upload(sums.view(np.int32)), S)
            ctx.synchronize()
            want = AA.resolve(img, sums, S, p0, n)
            np.testing.assert_array_equal(d_img.cpu().numpy(), want, err_msg="S %d rows %s" % (S, rows))
            assert (want[:3 * p0] == img[:3 * p0]).all() and (want[3 * (p0 + n):] == img[3 * (p0 + n):]).all()


def _gcontext(ugrt, g, rows=None, flags=0):
    ctx = ugrt.Context(G_W, G_H, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS, rows=rows, flags=flags)
    dv, df = ctx.upload(g.verts.reshape(-1)), ctx.upload(g.faces.reshape(-1))
    ctx.grid_build_uniform(df, dv, g.F, g.verts.min(0), g.verts.max(0))
    np.testing.assert_array_equal(ctx.grid_arrays(ugrt.GRID_UNIFORM)[2].cpu().numpy().view(np.uint32), g.grid["span"])
    ctx.upload_camera(g.cam.cc)
    ctx.set_light_position(G_LIGHT)
    assert (ctx.p0, ctx.npix) == ((0, G_N) if rows is None else (G_P0, G_NB))
    return types.SimpleNamespace(ctx=ctx, dv=dv, df=df, grid=ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3], mat_idx=ctx.upload(g.mat_idx),
                                 mat_list=ctx.upload(g.mat_list.reshape(-1)), strict=bool(flags))


def _ggather(torch, d, g, edge, S, tile, table, light, eps=1e-3, dv=None, df=None):
    sums = torch.full((4 * G_N,), SENTINEL, dtype=torch.int32, device=d.ctx.device)
    d.ctx.aa_gather(d.grid[0], d.grid[1], d.grid[2], d.dv if dv is None else dv, d.df if df is None else df, g.cam.cc,
                    d.ctx.upload(edge), S, tile[0], tile[1], table, d.mat_idx, d.mat_list, G_K, light, eps, sums)
    d.ctx.synchronize()
    return _words(sums)


def _check(torch, AA, g, contexts, edge, S, tile, table, light, eps=1e-3, msg=""):
    """The whole image and the band against the checker; the band's other words keep the sentinel."""
    for d in contexts:
        want = gsums(AA, g, edge, S, tile, table, light, eps, d.strict)
        got = _ggather(torch, d, g, edge, S, tile, d.ctx.upload(table.reshape(-1)), light, eps)
        p0, n = d.ctx.p0, d.ctx.npix
        assert (got[:4 * p0] == 0xFFFFFFF9).all() and (got[4 * (p0 + n):] == 0xFFFFFFF9).all(), msg
        np.testing.assert_array_equal(got[4 * p0:4 * (p0 + n)], want[4 * p0:4 * (p0 + n)],
                                      err_msg="%s S %d tile %s eps %g rows %s" % (msg, S, tile, eps, n != G_N))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("S", G_S)
def test_gather_sample_counts_and_tiles(ugrt, O, AA, torch, S):
    """Every tile, square or not, with a table of distinct rows per set, the shadow light inside the grid, every pixel
    flagged, whole image and band."""
    g = gscene(O, ugrt, AA)
    contexts = (_gcontext(ugrt, g), _gcontext(ugrt, g, G_ROWS))
    lit = 0
    for tile in G_TILES:
        want = _check(torch, AA, g, contexts, ONES, S, tile, random_table(S, tile), G_SHADOW_IN, msg="tiles")
        lit += int((want.reshape(G_N, 4)[:, :3].sum(1) > 0).sum())
    assert lit > G_N


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True])
def test_gather_odd_offsets(ugrt, O, AA, torch, strict):
    """+-0.5 and their float neighbours, +-0.75, +-1e30, +-inf, NaN, -0 and denormals, on every pixel, the borders and the
    corners included, with and without UGRT_FLAG_STRICT_TEXTURE; and the table that holds the clamped values instead."""
    g = gscene(O, ugrt, AA)
    flags = ugrt.FLAG_STRICT_TEXTURE if strict else 0
    contexts = (_gcontext(ugrt, g, flags=flags), _gcontext(ugrt, g, G_ROWS, flags=flags))
    odd = odd_table()
    for light in (None, G_SHADOW_IN):
        _check(torch, AA, g, contexts, ONES, 32, (1, 1), odd, light, msg="odd offsets")
        _check(torch, AA, g, contexts, ONES, 32, (1, 1), clamp_offsets(odd), light, msg="clamped offsets")
    _check(torch, AA, g, contexts, edge_forms()[4][1], 16, (2, 1), odd.reshape(2, 16, 2), G_SHADOW_IN, msg="odd offsets, two sets")


@pytest.mark.gpu
def test_gather_shadow_lights_and_eps(ugrt, O, AA, torch):
    """No light, a light inside the grid, far outside it, on a vertex of a hit triangle, in the plane of a triangle (its
    occluder at t = 1 to the float) and at the floats to either side; eps 1e-3, 0, -1e-3 and +inf."""
    g = gscene(O, ugrt, AA)
    contexts = (_gcontext(ugrt, g), _gcontext(ugrt, g, G_ROWS))
    vertex = g.verts[g.faces[g.stacks[(2, 3)][0] + 5, 0]].copy()
    table = random_table(8, (2, 3))
    for eps in G_EPS:
        for name, light in (("none", None), ("inside", G_SHADOW_IN), ("far", G_SHADOW_FAR), ("vertex", vertex)):
            _check(torch, AA, g, contexts, ONES, 8, (2, 3), table, light, eps, msg="light " + name)
        for k, light in enumerate(t1_lights()):
            _check(torch, AA, g, contexts, ONES, 8, (1, 1), main_table(ugrt), light, eps, msg="light in a plane %+d" % (k - 2))


@pytest.mark.gpu
def test_gather_edge_flags(ugrt, O, AA, torch):
    """All ones, all zeros, the band's last pixel only, a checkerboard, and the values 2, -1 and INT_MIN among zeros: a
    pixel is flagged where its word is not 0."""
    g = gscene(O, ugrt, AA)
    contexts = (_gcontext(ugrt, g), _gcontext(ugrt, g, G_ROWS))
    for name, edge in edge_forms():
        for S, tile in ((5, (3, 2)), (32, (1, 1))):
            want = _check(torch, AA, g, contexts, edge, S, tile, random_table(S, tile), G_SHADOW_IN, msg="flags " + name)
            np.testing.assert_array_equal(want.reshape(G_N, 4)[:, 3], (edge != 0).astype(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 31])
def test_gather_launch_shapes_change_no_word(ugrt, O, AA, torch, S):
    """any_rays_per_wave below S (one pixel a wave, more lanes walking than asked for), at values that leave idle lanes
    behind the last pixel, any_coop at 1, 8 and 2^30, dda_blocks 1 and 7, and arrays that are not the ones the grid was
    built from (no triangle records)."""
    g = gscene(O, ugrt, AA)
    d = _gcontext(ugrt, g)
    tile = (3, 2)
    table = random_table(S, tile)
    d_table = d.ctx.upload(table.reshape(-1))
    want = gsums(AA, g, ONES, S, tile, table, G_SHADOW_IN)
    for rpw in (1, 7, 31, 32, 64):
        for coop in (1, 8, 1 << 30):
            d.ctx.set_option("any_rays_per_wave", rpw)
            d.ctx.set_option("any_coop", coop)
            np.testing.assert_array_equal(_ggather(torch, d, g, ONES, S, tile, d_table, G_SHADOW_IN), want,
                                          err_msg="rays per wave %d, coop %d" % (rpw, coop))
    d.ctx.set_option("any_rays_per_wave", -1)
    d.ctx.set_option("any_coop", -1)
    for blocks in (1, 7):
        d.ctx.set_option("dda_blocks", blocks)
        np.testing.assert_array_equal(_ggather(torch, d, g, ONES, S, tile, d_table, G_SHADOW_IN), want,
                                      err_msg="blocks %d" % blocks)
    d.ctx.set_option("dda_blocks", -1)
    got = _ggather(torch, d, g, ONES, S, tile, d_table, G_SHADOW_IN, dv=d.dv.clone(), df=d.df.clone())
    np.testing.assert_array_equal(got, want, err_msg="no records")


@pytest.mark.gpu
def test_gather_table_alignment(ugrt, O, AA, torch):
    """The table 0, 4, 8 and 12 bytes into an allocation: float4 by float4 where it is 16-byte aligned, float by float
    elsewhere.  Its 2 S set_w set_h floats leave 0 or 2 behind the last float4 (an even count leaves neither 1 nor 3)."""
    g = gscene(O, ugrt, AA)
    d = _gcontext(ugrt, g)
    for S, tile, rest in ((1, (1, 1), 2), (2, (1, 1), 0), (3, (1, 1), 2), (7, (1, 1), 2), (5, (3, 2), 0), (31, (2, 3), 0),
                          (32, (4, 4), 0)):
        table = random_table(S, tile, seed=1)
        count = table.size
        assert count % 4 == rest
        want = gsums(AA, g, ONES, S, tile, table, G_SHADOW_IN)
        for shift in (0, 1, 2, 3):
            room = torch.full((count + 8,), float("nan"), dtype=torch.float32, device=d.ctx.device)
            base = (-room.data_ptr() // 4) % 4  # floats up to the next 16-byte boundary
            d_table = room[base + shift:base + shift + count]
            d_table.copy_(d.ctx.upload(table.reshape(-1)))
            assert d_table.data_ptr() % 16 == 4 * shift
            # first the same samples in the reverse order from an aligned table: what a launch finds in LDS is not its table
            turned = d.ctx.upload(np.ascontiguousarray(table[:, ::-1]).reshape(-1))
            np.testing.assert_array_equal(_ggather(torch, d, g, ONES, S, tile, turned, G_SHADOW_IN), want)
            np.testing.assert_array_equal(_ggather(torch, d, g, ONES, S, tile, d_table, G_SHADOW_IN), want,
                                          err_msg="S %d tile %s, %d bytes into the allocation" % (S, tile, 4 * shift))
