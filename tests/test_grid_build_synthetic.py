"""The three grid builds (ugrt_grid_build_perspective, _spherical, _uniform of csrc/ugrt_build.hip), their shared tail
(scan, k_fill_parts, k_fill, sort, k_bounds, the span scan, k_wide_rank, k_merge_narrow, k_merge_wide), the slab stage and
ugrt_grid_merge_shards on triangles made for them: vertices where the last bit decides the cell, and lists of triangles
that cross each branch of the tail on purpose.

Every other test feeds the builds cornell, hall, crash or a seeded soup, where no vertex lies on a cell boundary and the
tail's thresholds are met by luck or not at all.  Here every case is built with numpy in float64, rounded once to
float32, and seeded; the expected arrays are O.grid_perspective / O.grid_spherical / O.grid_uniform (which have no wide
list: every reference goes through one fill and one stable sort).

Boundary families
  uniform  a box (0.1 .. 0.9)^3 handed to the build, smaller than the geometry (-0.5 .. 1.5), dims (7,1,5), (12,10,3),
           (16,8,4).  Vertex coordinates are drawn from: lo + i * cs in float32 as O.uniform_setup gives lo and cs, one
           ulp below and above; bbmin and bbmax; values outside the box; PAIRS, adjacent floats that the oracle bins into
           different cells, found by bisection between two cells (flip_pairs).  Triangles wholly in an interior cell-face
           plane.  Triangles whose box is one cell, and the grid less one layer, twice: from wall to wall in float32
           (the far wall one ulp inside), where (wall - lo) * inv may round to either side of the integer, so that such
           a box is 1 to 18 cells by the oracle; and between the floats that decide (the first float the oracle bins
           into a cell, and the float below the next cell's first), where each box is one cell and each layer triangle
           prod(dims) / dims[k] * (dims[k] - 1) cells exactly.
  persp    the camera of tests/test_primary_cull_synthetic.py (its pixel_rays: a pixel's ray passes through the pixel's
           corner, so the pixels of column and row 0 mod 8 give the rays through tile corners and tile edges), 120 x 72,
           15 x 9 tiles (no powers of two, so that the products round); vertices on those rays at distances 1 .. 100,
           PAIRS around them along x and y, vertices on the eye plane (through the eye, across the viewing direction),
           the eye itself, vertices behind it, triangles that straddle the plane, 20 of them built to cover the screen;
           the full frame and the band rows=(2, 5), tile rows 2 .. 4.
  sph      the light of tests/test_shadow_synthetic.py (L = (3,4,5), looking along (1,0,0): every cell row occurs),
           light grids (2,2), (32,16), (256,256), (4096,2), (2,4096) (the ABI takes 2 .. 4096 per axis: the smallest
           grid, and the largest extent of either axis, not (4096,4096), whose 16.8 M cells are beyond a quick test): vertices on +-right, +-up, +-forward of L at the
           dyadic distances 0.5, 2, 8, 32, on the seam (the line of sight, where the angle to the view matrix's forward
           axis reaches pi and the column jumps from the first to the last) and PAIRS across it, at the poles and PAIRS
           around them, PAIRS where a column or a row changes anywhere on the sphere (the angle expressions land on an
           integer between the two), one vertex at L bit for bit.
Tail cases (TAIL; the same patterns for each grid from pools of triangles that the oracle classifies: n one cell, b many
cells, w the whole grid = wide, z no cell = off the band): fill parts that span 1024, 1025 and 1027 triangles behind
wide or off-band triangles; one triangle that fills whole parts; R = 1, 256, 257, 512; R = 0 with W > 0; a grid no
triangle touches; W = 1, 63, 64, 65 from the head of a wave, wide triangles in the last, padded wave (F = 300), spread over
waves and workgroups, W = 1024, 1025, 4096, 4097; a cell with a narrow run of 1024 and 1025 beside wide triangles; uniform
grids of 1, 2, 255, 256, 257, 65 535, 65 536 and 65 538 cells (65 537 is prime and no product of three dims up to 1024;
65 538 = 198 x 331 needs the same 17 sort bits); 40 triangles that each cover 63 x 64 x 16 cells of a (64,64,16) grid,
2 580 520 references with the one-cell triangles between them (the grid-stride fill in both forms).
Every case is built in the waiting form, again as the second build of the same inputs under async_build 1 and, uniform
and spherical, inside ugrt_grid_build_batch_begin / _end.  (That second build is asynchronous where the library allows
it: one slab, and at most 3000 wide triangles in the build before.  The slab cases, W4096 and W4097 build again in the
waiting form, and the context exposes nothing that says which form ran.)  A context builds the tail cases one after
the other, large then small, W > 0 then W = 0 and back.  Shards: set_face_window + ugrt_grid_merge_shards at 1, 2 and 16
parts, each window built in the waiting form and again under async_build 1.

CPU tests (unmarked): what the oracle says about the inputs, so that the GPU tests can fail: the PAIRS are one ulp
apart and lie in different cells, every tail case meets its branch condition (computed from the oracle's sizes and
scan), the slab cases have zMax == zMin, negative depths, depths on slab edges; the uniform family's triangles are hit
where the brute force says (O.trace_dda == O.brute_nearest, oc_trace_any == oc_brute_any around the hit).
GPU tests: key, value, span, offset, total_refs, num_cells and cells_used equal to the oracle's; with slabs also zMin,
zMax and projCoordZ.

Oracle figures (the CPU tests print them; run with -s)
  uniform  dims      F      R       cells used   PAIRS  vertex coordinates on a wall  vertices outside the grid
           (7,1,5)   2 433  7 872   35 of 35     120    4 053                         3 049
           (12,10,3) 2 761  18 705  360 of 360   180    4 654                         1 794
           (16,8,4)  2 797  21 235  512 of 512   180    4 647                         1 679
           in-plane triangles in the layer above / below their wall: 36 / 84, 180 / 84, 240 / 60
           the 120 boxes from wall to wall that are one cell by the oracle: 14, 26, 46 (the others 2 to 18 cells); the
           layer triangles from wall to wall: 35 30 35 28 of 35, 360 330 324 324 360 240 of 360, 480 480 448 448 384 384
           of 512 (two of four, two of six are the whole grid, so wide); between the deciding floats all 120 boxes are one
           cell and the layer triangles 30 30 28 28, 330 330 324 324 240 240, 480 480 448 448 384 384
  persp    full frame: F 5 086, R 31 246, 135 of 135 cells, 1 030 PAIRS, 34 wide triangles (all 20 built to straddle the
           eye plane among them), 64 triangles with a depth that is no finite number; rows=(2, 5): R 10 716, 45 cells,
           42 wide, 3 024 triangles off the band, 298 cut by its first row and 352 by its last
  sph      light grid  F      R          cells used        PAIRS (seam, poles)  rows / columns met  wide
           (2,2)       1 487  2 177      4 of 4            263 (3, 240)         2 / 2               14
           (32,16)     2 801  34 012     512 of 512        701 (40, 320)        16 / 32             12
           (256,256)   3 224  710 036    65 536 of 65 536  842 (80, 320)        256 / 256           2
           (4096,2)    2 756  1 242 979  8 188 of 8 192    686 (44, 320)        2 / 1 902           0
           (2,4096)    2 435  1 427 598  8 192 of 8 192    579 (40, 240)        1 901 / 2           3
           (with two columns the column is the same on either side of the seam: its PAIRS there are the rows')
  sort     cells 1, 2, 255, 256, 257, 65 535, 65 536, 65 538: F 763 or 761, R 763 to 2 503, sort bits 1, 1, 8, 8, 9, 16,
           16, 17; the one-cell grid has no wide triangle (full > 1), the two-cell grid 29
  stride   20 triangles: 1 290 260 narrow references in 5 041 parts (more than 4 096); 40: 2 580 520 in 10 081 (more
           than 8 192)
  walk     rays at the uniform families' triangles, 8 564 / 11 822 / 12 392 of them (1 136 / 2 460 / 2 896 at in-plane
           triangles): O.trace_dda differs from O.brute_nearest for 2 / 1 / 1, each with its hit on a cell face;
           oc_trace_any from oc_brute_any for none of ALL rays with t_max one float below or at the hit, and one float
           above it for 3 of 8 232 / 4 of 9 728 / 5 of 9 881, all of them among the 30 sampled rays whose nearest triangle
           lies in a cell-face plane: there the sample's size keeps the share under the cap, not the inputs.  (Of ALL rays with such a nearest triangle about one in ten differs there: the cell is
           entered at the hit's own parameter.  That is how the walk is specified, not a fault of the builder.)
tests/golden/ref_kernels_buildsyn.npz (tests/golden/make_ref_kernels.py) records what the reference's own count, slab and
fill kernels compute on the perspective family (full frame) and on the spherical family at (32,16), slabs 1 and 3.  The
oracle equals them on every triangle of the perspective family, eye plane included, and on the spherical family's but
for the 606 of 2 801 triangles with a vertex whose angle is acos(0/0) (at L, on +-up, on +-right), which the host build
of those kernels converts otherwise than a GPU does (pinned()).
Measured on an MI355X: the 132 GPU tests of this file take 3.8 s together (the slowest 0.2 s).
No comparison failed on the library as it was: nothing in csrc/ugrt_build.hip or oracle/ugrt_oracle.c changed.
Builds of the library that change arithmetic alone in csrc/ugrt_build.hip (no address, no index range), the GPU tests of
this file that fail on each (of 132), and of the suite as it was before this file (696 GPU tests):
  (p - lo) / cs for (p - lo) * inv in d_ucell            2: test_uniform_boundary_family[(7,1,5)], [(12,10,3)]; suite 0
  x * (nbx / 2) + nbx / 2 for ((x + 1) / 2) * nbx in k_count_persp (and y)
                                                         15: test_perspective_boundary_family (both), test_slabs[*-p],
                                                         test_tail_case[p|pband - W1024, W1025, no_wide], the two
                                                         perspective contexts of test_one_context_... and of
                                                         test_the_screen_grid_puts_its_merge_off_...; suite 1
                                                         (test_primary_cull_synthetic::test_frame_equals_the_oracle[band])
  angle * (n / max) for (angle / max) * n in d_effective_x/y, for the build alone
                                                         7: test_spherical_boundary_family at every grid but (2,2),
                                                         test_slabs[*-s]; suite 4 (test_light_grid_sweep, crash at
                                                         (4096,256) and (4096,2))
  gymax <= gy_lo for gymax < gy_lo in the band test      37 (every perspective test); suite 154: a blunt change, row 0
                                                         of a full frame goes missing
  truncation for ugrt_floor2i in a count kernel, `full > 0` for `full > 1` in d_split_wide: no test here or in the suite
  fails, and none can: the cell is clamped to 0 from below right after, where floor and truncation part only below 0;
  and a one-cell grid whose triangles are all wide gives the same arrays, element for element.  ((x + 1) * (nbx / 2) is
  likewise the same float as ((x + 1) / 2) * nbx: halving is exact.)
"""
import functools
import types

import numpy as np
import pytest

import test_primary_cull_synthetic as PC
import test_shadow_synthetic as SS

PI_F = float(np.float32(np.pi))
FILL_LDS = 1024          # csrc/ugrt_build.hip: a fill part's run of the scan is searched in LDS up to this length
MERGE_LDS = 1024         # ... the wide list (k_merge_narrow) and a cell's narrow run (k_merge_wide) likewise
PART = 256               # references per fill part (BUILD_THREADS)
FILL_MAX_BLOCKS, FILL_MAX_BLOCKS_COUNTING = 8192, 4096
WIDE_RANK_MAX = 4096     # above: the wide ids go through the radix sort, and the screen grid's merge is not put off
PW, PH = 120, 72         # the perspective cases' image: 15 x 9 tiles (no powers of two: the products round)
BAND = (2, 5)


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def bits_for(C):
    b = 1
    while b < 32 and (1 << b) < C:
        b += 1
    return b


# ------------------------------------------------------------------------------------------------ cases and the oracle

def case(kind, tris, **cfg):
    """kind: "u" uniform (dims, bbmin, bbmax), "p" perspective (rows), "s" spherical (lg); slabs, window."""
    verts = f32(np.asarray(tris, np.float64).reshape(-1, 3))
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    c = types.SimpleNamespace(kind=kind, verts=verts, faces=faces, F=len(faces), rows=None, slabs=1, window=None,
                              dims=None, bbmin=None, bbmax=None, lg=None, img=(PW, PH))
    c.__dict__.update(cfg)
    return c


@functools.lru_cache(maxsize=None)
def camera(O, img=(PW, PH)):
    """(camera, eye, each pixel's direction) of the perspective cases."""
    return PC.pixel_rays(O, img[0], img[1], False)


@functools.lru_cache(maxsize=None)
def light(O):
    return O.cam_from(SS.LIGHT, SS.FOVY, 2.0)


def oracle(O, c, window="case", slabs=None):
    window = c.window if window == "case" else window
    slabs = c.slabs if slabs is None else slabs
    if c.kind == "u":
        return O.grid_uniform(c.faces, c.verts, c.bbmin, c.bbmax, c.dims, window=window)
    if c.kind == "p":
        return O.grid_perspective(camera(O, c.img)[0].cc, c.faces, c.verts, c.img[0] // 8, c.img[1] // 8, c.rows, slabs=slabs)
    return O.grid_spherical(light(O).cc, c.faces, c.verts, c.lg[0], c.lg[1], slabs=slabs, window=window)


def active_cells(c):
    """The cells a wide triangle covers (d_split_wide's `full`); with z-slabs no triangle is wide."""
    if c.kind == "u":
        return int(np.prod(c.dims))
    if c.kind == "p":
        lo, hi = c.rows if c.rows is not None else (0, c.img[1] // 8)
        return (c.img[0] // 8) * (hi - lo)
    return c.lg[0] * c.lg[1]


def tail_stats(c, g):
    """What the tail of the build sees, from the oracle's sizes: the wide triangles leave the scan."""
    sizes = g["sizes"].astype(np.int64)
    full = active_cells(c)
    wide = (sizes == full) & (full > 1) & (c.slabs == 1)
    narrow = np.where(wide, 0, sizes)
    scan = np.cumsum(narrow)
    Rn, W = int(scan[-1]), int(wide.sum())
    nparts = (Rn + PART - 1) // PART
    first = np.searchsorted(scan, np.minimum(np.arange(nparts + 1) * PART, max(Rn - 1, 0)), side="right")
    nrun = first[1:] - first[:-1] + 1 if Rn else np.zeros(0, np.int64)
    longest = 0
    if Rn:
        # the longest run of narrow references in one cell: the cells' spans less the wide triangles of an active cell
        sp = g["span"].astype(np.int64)
        longest = int((sp - np.where(sp > 0, W, 0)).max()) if W else int(sp.max())
    wave = np.flatnonzero(wide) // 64
    return types.SimpleNamespace(F=c.F, full=full, W=W, Rn=Rn, R=int(g["R"]), nparts=nparts, nrun=nrun,
                                 nrun_max=int(nrun.max()) if nrun.size else 0, whole_parts=int((nrun == 1).sum()),
                                 longest=longest, wide=wide, waves=np.unique(wave), bits=bits_for(len(g["span"])),
                                 cells=len(g["span"]), used=int(g["used"]))


# ------------------------------------------------------------------------------------------------ PAIRS: adjacent floats

def to_ord(x):
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


def from_ord(o):
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(np.float32)


def flip_pairs(cell_of, A, B, axis):
    """A, B: float32 points [n, 3] that differ in coordinate `axis` alone.  Where cell_of (points -> an integer each) tells
    them apart: (Pa, Pb), equal to A but for that coordinate, one ulp apart in it, cell_of(Pa) == cell_of(A) != cell_of(Pb)."""
    A, B = f32(A), f32(B)
    ca = cell_of(A)
    keep = cell_of(B) != ca
    A, B, ca = A[keep], B[keep], ca[keep]
    lo, hi = to_ord(A[:, axis]), to_ord(B[:, axis])
    while (np.abs(hi - lo) > 1).any():
        mid = (lo + hi) // 2
        M = A.copy()
        M[:, axis] = from_ord(mid)
        same = cell_of(M) == ca
        open_ = np.abs(hi - lo) > 1
        lo, hi = np.where(same & open_, mid, lo), np.where(~same & open_, mid, hi)
    Pa, Pb = A.copy(), A.copy()
    Pa[:, axis], Pb[:, axis] = from_ord(lo), from_ord(hi)
    return Pa, Pb


def points_as_triangles(P):
    return np.repeat(np.asarray(P, np.float64)[:, None, :], 3, axis=1)


def cell_fn(O, kind, **cfg):
    """points [n, 3] -> the oracle's cell of each (a triangle of three equal vertices has one reference, or none)."""
    def cell_of(P):
        c = case(kind, points_as_triangles(P), **cfg)
        g = oracle(O, c)
        if kind == "u":
            out = np.full(c.F, -1, np.int64)
            out[g["vals"]] = g["keys"]
            return out
        r = g["rng"].reshape(-1, 4).astype(np.int64)
        return r[:, 0] * 100000 + r[:, 2]
    return cell_of


def around(rng, P, spread, n_each=1):
    """Triangles with P[i] as their first vertex and two more within `spread[i]` of it."""
    P = np.asarray(P, np.float64)
    spread = np.broadcast_to(np.asarray(spread, np.float64), (len(P),))
    P = np.repeat(P, n_each, axis=0)
    s = np.repeat(spread, n_each)[:, None, None]
    other = P[:, None, :] + rng.uniform(-1, 1, (len(P), 2, 3)) * s
    return np.concatenate([P[:, None, :], other], 1)


def pair_triangles(rng, Pa, Pb, spread):
    """Per pair: a triangle at Pa, one at Pb with the same two other vertices, and one that holds both."""
    ta = around(rng, Pa, spread)
    tb = ta.copy()
    tb[:, 0] = Pb
    tc = ta.copy()
    tc[:, 1] = Pb
    return np.concatenate([ta, tb, tc])


# ------------------------------------------------------------------------------------------------ the boundary families

UDIMS = ((7, 1, 5), (12, 10, 3), (16, 8, 4))
UBOX = (np.full(3, 0.1, np.float32), np.full(3, 0.9, np.float32))


@functools.lru_cache(maxsize=None)
def uniform_family(O, dims):
    rng = np.random.default_rng([20261101, dims[0], dims[1], dims[2]])
    bbmin, bbmax = UBOX
    cfg = dict(dims=dims, bbmin=bbmin, bbmax=bbmax)
    ug = O.uniform_setup(bbmin, bbmax, dims)
    lo, cs = ug[0:3], ug[3:6]
    # lo + i * cs in float32, the product and the sum rounded as the float32 they are
    walls = [f32(lo[k] + f32(np.arange(dims[k] + 1)) * cs[k]) for k in range(3)]
    for k in range(3):
        assert walls[k].dtype == np.float32
    sharp = []  # per axis: the walls, one ulp either side, the caller's box, values outside it
    for k in range(3):
        w = walls[k]
        sharp.append(np.concatenate([w, np.nextafter(w, np.float32(-9)), np.nextafter(w, np.float32(9)),
                                     [bbmin[k], bbmax[k], -0.5, 0.0, 1.0, 1.5]]).astype(np.float32))
    # (a) triangles about a cell: each coordinate of each vertex a sharp value near that cell, or anywhere near it
    n = 1500
    base = np.stack([rng.integers(0, dims[k], n) for k in range(3)], 1)
    tri = np.zeros((n, 3, 3))
    for k in range(3):
        w = walls[k].astype(np.float64)
        idx = np.clip(base[:, k, None] + rng.integers(0, 2, (n, 3)), 0, dims[k])
        ulp = rng.integers(-1, 2, (n, 3))
        on = np.where(ulp < 0, np.nextafter(walls[k][idx], np.float32(-9)),
                      np.where(ulp > 0, np.nextafter(walls[k][idx], np.float32(9)), walls[k][idx])).astype(np.float64)
        free = w[base[:, k], None] + rng.uniform(-0.7, 1.7, (n, 3)) * cs[k]
        tri[:, :, k] = np.where(rng.random((n, 3)) < 0.5, on, free)
    # (b) triangles wholly in an interior cell-face plane
    planes, plane_axis, plane_wall = [], [], []
    for k in range(3):
        for i in range(1, dims[k]):
            m = 12
            t = rng.uniform(0.05, 0.95, (m, 1, 3)) + rng.uniform(-0.12, 0.12, (m, 3, 3))
            t[:, :, k] = walls[k][i]
            planes.append(t)
            plane_axis += [k] * m
            plane_wall += [i] * m
    planes = np.concatenate(planes)
    # (c) boxes that are one cell from face to face, and the grid less one layer
    m = m_boxes = 120
    cell = np.stack([rng.integers(0, dims[k], m) for k in range(3)], 1)
    lo_c = np.stack([walls[k][cell[:, k]] for k in range(3)], 1).astype(np.float64)
    hi_c = np.stack([np.nextafter(walls[k][cell[:, k] + 1], np.float32(-9)) for k in range(3)], 1).astype(np.float64)
    one_cell = np.stack([lo_c, hi_c, lo_c], 1)
    layers = []
    for k in range(3):
        if dims[k] < 2:
            continue
        for side in (0, 1):
            a = np.array([walls[j][0] for j in range(3)], np.float64)
            b = np.array([np.nextafter(walls[j][dims[j]], np.float32(-9)) for j in range(3)], np.float64)
            if side == 0:
                a[k] = walls[k][1]
            else:
                b[k] = np.nextafter(walls[k][dims[k] - 1], np.float32(-9))
            layers.append(np.stack([a, b, 0.5 * (a + b)]))
    layers = np.asarray(layers)
    # (c') the same from the floats that decide: cell i of an axis begins at the first float the oracle bins into it
    # (flip_pairs between the middles of cells i - 1 and i; (wall - lo) * inv may round to either side of i, so a wall
    # itself need not be that float) and ends one float below the next cell's first.  The grid's outer faces clamp.
    cell_of = cell_fn(O, "u", **cfg)
    first, last = [], []  # per axis: the first and the last float of each cell
    for k in range(3):
        mid = np.tile(0.5 * (bbmin + bbmax).astype(np.float64), (max(dims[k] - 1, 0), 1))
        A, B = mid.copy(), mid.copy()
        A[:, k] = walls[k][:-2].astype(np.float64) + 0.5 * cs[k]
        B[:, k] = walls[k][1:-1].astype(np.float64) + 0.5 * cs[k]
        Pa, Pb = (flip_pairs(cell_of, A, B, k) if dims[k] > 1 else (f32(A), f32(B)))
        assert len(Pa) == dims[k] - 1
        first.append(np.concatenate([walls[k][:1], Pb[:, k]]).astype(np.float64))
        last.append(np.concatenate([Pa[:, k], np.nextafter(walls[k][-1:], np.float32(-9))]).astype(np.float64))
    lo_x = np.stack([first[k][cell[:, k]] for k in range(3)], 1)
    hi_x = np.stack([last[k][cell[:, k]] for k in range(3)], 1)
    one_cell_exact = np.stack([lo_x, hi_x, lo_x], 1)
    layers_exact, layer_sizes = [], []
    for k in range(3):
        if dims[k] < 2:
            continue
        for side in (0, 1):
            a, b = np.array([first[j][0] for j in range(3)]), np.array([last[j][-1] for j in range(3)])
            if side == 0:
                a[k] = first[k][1]
            else:
                b[k] = last[k][dims[k] - 2]
            layers_exact.append(np.stack([a, b, 0.5 * (a + b)]))
            layer_sizes.append(int(np.prod(dims)) // dims[k] * (dims[k] - 1))
    layers_exact = np.asarray(layers_exact)
    # (d) PAIRS: between the middles of neighbouring cells, along each axis
    pairs = []
    npairs = 0
    for k in range(3):
        if dims[k] < 2:
            continue
        m = 60
        A = rng.uniform(0.12, 0.88, (m, 3))
        i = rng.integers(0, dims[k] - 1, m)
        A[:, k] = walls[k][i] + 0.5 * cs[k]
        B = A.copy()
        B[:, k] = A[:, k] + cs[k]
        Pa, Pb = flip_pairs(cell_of, A, B, k)
        npairs += len(Pa)
        pairs.append(pair_triangles(rng, Pa, Pb, 0.3 * float(cs.min())))
    # (e) the caller's box, and far outside it
    corners = np.array([[bbmin, bbmax, 0.5 * (bbmin + bbmax)], [bbmin, bbmin, bbmin], [bbmax, bbmax, bbmax],
                        [[-0.5, -0.5, -0.5], [1.5, 0.2, 0.3], [0.3, 1.5, 0.2]], [[-40.0, 0.5, 0.5], [0.5, 0.5, 90.0], [0.5, 0.5, 0.5]]],
                       np.float64)
    soup = rng.uniform(-0.5, 1.5, (200, 1, 3)) + rng.normal(size=(200, 3, 3)) * 0.08
    parts = [tri, planes, one_cell, layers] + pairs + [corners, soup, one_cell_exact, layers_exact]
    c = case("u", np.concatenate(parts), **cfg)
    c.wall_boxes = np.arange(n + len(planes), n + len(planes) + m_boxes)
    c.wall_layers = np.arange(c.wall_boxes[-1] + 1, c.wall_boxes[-1] + 1 + len(layers))
    c.exact_boxes = np.arange(c.F - len(layers_exact) - m_boxes, c.F - len(layers_exact))
    c.exact_layers, c.layer_sizes = np.arange(c.F - len(layers_exact), c.F), np.asarray(layer_sizes)
    c.plane_axis, c.plane_wall = np.asarray(plane_axis), np.asarray(plane_wall)
    c.walls, c.ug, c.npairs = walls, ug, npairs
    c.n_free, c.n_planes = n, len(planes)
    c.plane_faces = np.arange(n, n + len(planes))
    first_pair = sum(len(x) for x in (tri, planes, one_cell, layers))
    c.pair_faces = np.zeros(c.F, bool)
    c.pair_faces[first_pair:first_pair + sum(len(x) for x in pairs)] = True
    return c


def across_and_wide(rng, eye, dirs, n):
    """Triangles across the eye plane that cover the screen: a vertex beyond one corner of the screen, one behind the eye
    on the line through the opposite corner (it projects beyond that corner), one in front."""
    dc = unit(dirs.mean(0))
    out0, out1 = unit(dirs[0] + 0.5 * (dirs[0] - dc)), unit(dirs[-1] + 0.5 * (dirs[-1] - dc))
    return np.stack([eye + rng.uniform(1, 30, (n, 1)) * out0, eye - rng.uniform(1, 30, (n, 1)) * out1,
                     eye + rng.uniform(1, 30, (n, 1)) * dc], 1)


def eye_frame(O):
    cam, eye, dirs = camera(O)
    fwd = unit(PC.LOOK)
    right = unit(np.cross([0.0, 1.0, 0.0], fwd))
    return eye, fwd, right, np.cross(fwd, right)


@functools.lru_cache(maxsize=None)
def persp_family(O, rows):
    rng = np.random.default_rng(20261102)
    cam, eye, dirs = camera(O)
    eye, fwd, right, up = eye_frame(O)
    col, row = np.meshgrid(np.arange(PW), np.arange(PH), indexing="xy")
    corner = ((col % 8 == 0) & (row % 8 == 0)).reshape(-1)
    edge = ((col % 8 == 0) ^ (row % 8 == 0)).reshape(-1)
    p = np.concatenate([np.flatnonzero(corner), rng.choice(np.flatnonzero(edge), 400, replace=False)])
    t = np.exp(rng.uniform(np.log(1.0), np.log(100.0), p.size))
    on_ray = eye + t[:, None] * dirs[p]
    pix = float(np.median(np.linalg.norm(dirs[1:] - dirs[:-1], axis=1)))
    spread = 3.0 * pix * t
    cell_of = cell_fn(O, "p", rows=None)
    pairs, npairs = [], 0
    for axis in (0, 1):
        step = np.zeros(3)
        step[axis] = 1.0
        A = f32(on_ray - 4.0 * (pix * t)[:, None] * step)
        B = A.copy()
        B[:, axis] = f32(on_ray + 4.0 * (pix * t)[:, None] * step)[:, axis]
        Pa, Pb = flip_pairs(cell_of, A, B, axis)
        npairs += len(Pa)
        pairs.append(pair_triangles(rng, Pa, Pb, 2.0 * pix * np.linalg.norm(Pa - eye, axis=1)))
    # the eye plane: on it (to float32's rounding of the plane's points, and the eye bit for bit), behind it, across it
    m = 60
    on_plane = eye + rng.uniform(-5, 5, (m, 1)) * right + rng.uniform(-5, 5, (m, 1)) * up
    front = eye + rng.uniform(1, 30, (m, 1)) * unit(fwd + rng.uniform(-0.4, 0.4, (m, 3)))
    behind = eye - rng.uniform(0.01, 30, (m, 1)) * unit(fwd + rng.uniform(-0.8, 0.8, (m, 3)))
    eye32 = cam.worldori[:3].astype(np.float64)
    plane_tris = np.concatenate([
        np.stack([on_plane, front, np.roll(front, 1, 0)], 1), np.stack([on_plane, np.roll(on_plane, 1, 0), front], 1),
        points_as_triangles(on_plane[:10]), np.stack([np.broadcast_to(eye32, (m, 3)), front, np.roll(front, 1, 0)], 1),
        points_as_triangles(eye32[None, :]), np.stack([behind, np.roll(behind, 1, 0), np.roll(behind, 2, 0)], 1),
        np.stack([front, behind, np.roll(front, 1, 0)], 1), np.stack([behind, np.roll(behind, 1, 0), front], 1)])
    ns = 20
    plane_tris = np.concatenate([plane_tris, across_and_wide(rng, eye, dirs, ns)])
    straddle = np.arange(len(plane_tris) - ns, len(plane_tris))
    parts = [around(rng, on_ray, spread, 2), points_as_triangles(on_ray)] + pairs
    first_plane = sum(len(x) for x in parts)
    c = case("p", np.concatenate(parts + [plane_tris]), rows=rows)
    c.npairs, c.straddle, c.n_on_ray = npairs, first_plane + straddle, len(on_ray)
    c.plane_faces = np.arange(first_plane, first_plane + len(plane_tris))
    return c


SPH_GRIDS = ((2, 2), (32, 16), (256, 256), (4096, 2), (2, 4096))


@functools.lru_cache(maxsize=None)
def sph_family(O, lg):
    rng = np.random.default_rng([20261103, lg[0], lg[1]])
    L = SS.L
    cfg = dict(lg=lg)
    cell_of = cell_fn(O, "s", **cfg)
    axes = np.array([[0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
    on_axis = (L + axes[:, None, :] * np.asarray(SS.AXIS_STEPS)[None, :, None]).reshape(-1, 3)  # exact in float32
    assert (f32(on_axis).astype(np.float64) == on_axis).all()
    pairs, npairs = [], 0

    def add_pairs(A, B, axis):
        nonlocal npairs
        Pa, Pb = flip_pairs(cell_of, A, B, axis)
        npairs += len(Pa)
        pairs.append(pair_triangles(rng, Pa, Pb, 0.02 * np.linalg.norm(Pa - L, axis=1)))
        return len(Pa)

    # the seam, where the angle to the forward axis reaches pi and the column jumps from the first to the last: on the
    # line of sight (both ways along it are taken: one of them is the seam), across it along z and along y
    r = np.repeat(np.asarray(SS.AXIS_STEPS), 10)
    seam = L + np.stack([r * np.tile([1.0, -1.0], r.size // 2), rng.uniform(-0.5, 0.5, r.size) * r, np.zeros(r.size)], 1)
    n_seam = 0
    for axis in (2, 1):
        d = np.zeros(3)
        d[axis] = 1.0
        n_seam += add_pairs(seam - 0.05 * r[:, None] * d, seam + 0.05 * r[:, None] * d, axis)
    # the poles (+-up = +-y, where the column's projection vanishes; +-right = +-z, where the row's does)
    n_pole = 0
    for a in axes[:4]:
        P = L + a * r[:, None]
        for axis in range(3):
            if a[axis] != 0:
                continue
            d = np.zeros(3)
            d[axis] = 1.0
            n_pole += add_pairs(P - 0.03 * r[:, None] * d, P + 0.03 * r[:, None] * d, axis)
    # anywhere on the sphere: a column or a row changes between two points a few cells apart
    m = 150
    P = L + unit(rng.normal(size=(m, 3))) * np.exp(rng.uniform(np.log(0.5), np.log(50.0), m))[:, None]
    for axis in range(3):
        d = np.zeros(3)
        d[axis] = 1.0
        add_pairs(P, P + np.linalg.norm(P - L, axis=1)[:, None] * 0.3 * d, axis)
    at_light = np.stack([f32(L).astype(np.float64), L + [2.0, 0.5, 0.0], L + [2.0, 0.0, 0.5]])[None]
    shells = L + unit(rng.normal(size=(600, 1, 3))) * np.exp(rng.uniform(np.log(0.5), np.log(50.0), 600))[:, None, None]
    shells = shells * np.ones((1, 3, 1)) + rng.normal(size=(600, 3, 3)) * 0.03 * np.linalg.norm(shells - L, axis=2, keepdims=True)
    parts = [around(rng, on_axis, 0.05 * np.repeat(np.asarray(SS.AXIS_STEPS)[None, :], 6, 0).reshape(-1), 3),
             points_as_triangles(on_axis), at_light, points_as_triangles(f32(L)[None, :])] + pairs + [shells]
    c = case("s", np.concatenate(parts), **cfg)
    c.npairs, c.n_seam, c.n_pole = npairs, n_seam, n_pole
    return c


# ------------------------------------------------------------------------------------------------ the tail's cases

TAIL_UDIMS = (4, 3, 5)
TAIL_LG = (4, 2)


def ucell_centre(dims, ijk):
    """The middle of a cell of the tail cases' uniform grid: box (0,0,0) .. dims, so a cell is one unit (and the pad)."""
    return np.asarray(ijk, np.float64) + 0.5


def ubox(dims, lo, hi):
    """A triangle whose cell range is lo .. hi per axis."""
    a, b = ucell_centre(dims, lo), ucell_centre(dims, hi)
    return np.stack([a, b, a])


@functools.lru_cache(maxsize=None)
def pools(O, kind, cfgkey):
    """Triangles the oracle classifies for a grid: n = one cell, b = several but not all, w = all active cells (wide),
    z = none (off the band), B = the b with the most references."""
    cfg = dict(cfgkey)
    rng = np.random.default_rng([20261104, "ups".index(kind)])
    if kind == "u":
        dims = cfg["dims"]
        cells = np.stack([rng.integers(0, dims[k], 400) for k in range(3)], 1)
        one = np.stack([ubox(dims, c, c) for c in cells]) + rng.uniform(-0.2, 0.2, (400, 3, 3))
        lo = np.stack([rng.integers(0, dims[k], 200) for k in range(3)], 1)
        hi = np.minimum(lo + rng.integers(0, 3, (200, 3)), np.asarray(dims) - 1)
        some = np.stack([ubox(dims, a, b) for a, b in zip(lo, hi)])
        full = np.stack([ubox(dims, (0, 0, 0), np.asarray(dims) - 1)] * 4) + rng.uniform(-0.2, 0.2, (4, 3, 3))
        most = [ubox(dims, (1 if k == 0 else 0, 1 if k == 1 else 0, 1 if k == 2 else 0), np.asarray(dims) - 1)
                for k in range(3) if dims[k] > 1]
        cand = np.concatenate([one, some, full] + ([np.stack(most)] if most else []))
    elif kind == "p":
        iw, ih = cfg.get("img", (PW, PH))
        cam, eye, dirs = camera(O, (iw, ih))
        eye, fwd, right, up = eye_frame(O)
        tx, ty = rng.integers(0, iw // 8, 600), rng.integers(0, ih // 8, 600)
        p = (ty * 8 + 4) * iw + tx * 8 + 4
        t = rng.uniform(2, 50, 600)
        one = (eye + t[:, None] * dirs[p])[:, None, :] + rng.normal(size=(600, 3, 3)) * (1e-3 * t)[:, None, None]
        q = rng.integers(0, iw * ih, (300, 3))
        q[:40] = [0, iw * ih - 1, iw * (ih - 2)]  # (nearly the whole screen)
        q[:40] += rng.integers(0, iw // 2, (40, 3)) * [1, -1, 1]
        some = eye + rng.uniform(5, 20, (300, 3, 1)) * dirs[q]
        front = eye + rng.uniform(1, 30, (60, 1)) * unit(fwd + rng.uniform(-0.4, 0.4, (60, 3)))
        behind = eye - rng.uniform(1, 30, (60, 1)) * unit(fwd + rng.uniform(-0.4, 0.4, (60, 3)))
        across = np.stack([front, behind, np.roll(front, 1, 0)], 1)
        cand = np.concatenate([one, some, across, across_and_wide(rng, eye, dirs, 12)])
    else:
        L = SS.L
        d = unit(rng.normal(size=(600, 3)))
        r = rng.uniform(1, 20, 600)
        one = (L + d * r[:, None])[:, None, :] + rng.normal(size=(600, 3, 3)) * (1e-3 * r)[:, None, None]
        some = L + unit(rng.normal(size=(600, 3, 3))) * rng.uniform(1, 20, (600, 1, 1))
        # column 0 holds a vertex only where the angle to the forward axis is pi exactly: on the line of sight, at dyadic
        # distances (either way along it: the axis is the view matrix's, which looks down its negative z)
        back = some[:300].copy()
        back[:, 0] = L + np.array([1.0, 0.0, 0.0]) * rng.choice(np.asarray(SS.AXIS_STEPS), (300, 1)) * rng.choice([-1.0, 1.0], (300, 1))
        cand = np.concatenate([one, some, back])
    c = case(kind, cand, **cfg)
    sizes = oracle(O, c)["sizes"].astype(np.int64)
    full = active_cells(c)
    tri = c.verts.reshape(-1, 3, 3).astype(np.float64)
    P = {"n": tri[sizes == 1], "b": tri[(sizes > 1) & (sizes < full)], "w": tri[(sizes == full) & (full > 1)],
         "z": tri[sizes == 0]}
    bs = sizes[(sizes > 1) & (sizes < full)]
    P["B"] = P["b"][np.argsort(-bs, kind="stable")[:1]] if len(bs) else P["b"]
    if full == 1:
        P["w"] = tri[:0]
    return P


def compose(O, kind, letters, **cfg):
    """The case whose triangle i is the next of pool letters[i] (c: always the first one-cell triangle)."""
    # (the pools' key: numpy arrays do not hash, a box goes in as a tuple)
    key = {k: tuple(float(x) for x in v) if k in ("bbmin", "bbmax") else v for k, v in cfg.items()}
    P = pools(O, kind, tuple(sorted(key.items())))
    nxt = dict.fromkeys("nbwzB", 0)
    tris = []
    for ch in letters:
        pool = P["n" if ch == "c" else ch]
        assert len(pool), "no triangle of class %r for %s %r" % (ch, kind, cfg)
        tris.append(pool[0 if ch == "c" else nxt[ch] % len(pool)])
        if ch != "c":
            nxt[ch] += 1
    return case(kind, np.asarray(tris), **cfg)


def spread(seed, F, W, narrow="n"):
    rng = np.random.default_rng([20261105, seed])
    s = np.array([narrow] * F)
    s[rng.choice(F, W, replace=False)] = "w"
    return "".join(s)


# name -> (letters, what tail_stats must say).  (F = 300 leaves 44 triangles in the last, padded wave: waves 0 .. 4.)
TAIL = {
    "parts1024": ("n" + "w" * 1022 + "n", dict(nrun_max=FILL_LDS, W=1022)),
    "parts1025": ("n" + "w" * 1023 + "n", dict(nrun_max=FILL_LDS + 1, W=1023)),
    "parts1027": ("n" + "w" * 1025 + "n", dict(nrun_max=FILL_LDS + 3, W=1025)),
    "one_fills_parts": ("nnn" + "B" + "nnn", dict()),
    "R1": ("n", dict(Rn=1, W=0, F=1)),
    "R256": ("n" * 256, dict(Rn=256, W=0)),
    "R257": ("n" * 257, dict(Rn=257, W=0)),
    "R512_W2": ("w" + "n" * 512 + "w", dict(Rn=512, W=2)),
    "all_wide": ("w" * 5, dict(Rn=0, W=5)),
    "W1": ("w" + "n" * 299, dict(W=1, waves=[0])),
    "W63": ("w" * 63 + "n" * 237, dict(W=63, waves=[0])),
    "W64": ("w" * 64 + "n" * 236, dict(W=64, waves=[0])),
    "W65": ("w" * 65 + "n" * 235, dict(W=65, waves=[0, 1])),
    "W_padded_wave": ("n" * 290 + "w" * 10, dict(W=10, waves=[4])),
    "W_spread": (spread(1, 3000, 200), dict(W=200)),
    "W1024": (spread(2, 1524, 1024, "b"), dict(W=MERGE_LDS)),
    "W1025": (spread(3, 1525, 1025, "b"), dict(W=MERGE_LDS + 1)),
    "W4096": (spread(4, 4596, 4096), dict(W=WIDE_RANK_MAX)),
    "W4097": (spread(5, 4597, 4097), dict(W=WIDE_RANK_MAX + 1)),
    "run1024": ("w" + "c" * 1024 + "ww", dict(W=3, longest=MERGE_LDS)),
    "run1025": ("c" * 1025 + "www", dict(W=3, longest=MERGE_LDS + 1)),
    "no_wide": ("b" * 100 + "n" * 100, dict(W=0)),
}
# the perspective band only: triangles off the band have no references, as a wide triangle has none in the scan
TAIL_BAND = {
    "off1024": ("n" + "z" * 1022 + "n", dict(nrun_max=FILL_LDS, W=0)),
    "off1025": ("n" + "z" * 1023 + "n", dict(nrun_max=FILL_LDS + 1, W=0)),
    "off_and_wide": ("n" + "z" * 700 + "w" * 700 + "n" * 2, dict(nrun_max=1403, W=700)),
    "untouched": ("z" * 10, dict(Rn=0, W=0, R=0, used=0)),
}
TAIL_GRIDS = {"u": dict(dims=TAIL_UDIMS, bbmin=(0.0, 0.0, 0.0), bbmax=tuple(float(x) for x in TAIL_UDIMS)),
              "p": dict(rows=None), "pband": dict(rows=BAND), "s": dict(lg=TAIL_LG)}
# "one_fills_parts" needs a triangle of several hundred references that is not wide: larger grids
ONE_FILLS = {"u": dict(dims=(16, 16, 8), bbmin=(0.0, 0.0, 0.0), bbmax=(16.0, 16.0, 8.0)), "p": dict(rows=None, img=(520, 264)),
             "pband": dict(rows=(8, 24), img=(520, 264)), "s": dict(lg=(64, 32))}
TAIL_CASES = [(g, name) for g in TAIL_GRIDS for name in TAIL] + [("pband", name) for name in TAIL_BAND]


@functools.lru_cache(maxsize=None)
def tail_case(O, grid, name):
    letters, expect = TAIL[name] if name in TAIL else TAIL_BAND[name]
    cfg = dict(ONE_FILLS[grid] if name == "one_fills_parts" else TAIL_GRIDS[grid])
    if "bbmin" in cfg:
        cfg["bbmin"], cfg["bbmax"] = f32(cfg["bbmin"]), f32(cfg["bbmax"])
    c = compose(O, grid[0], letters, **cfg)
    c.expect = expect
    return c


def ucfg(dims):
    return dict(dims=tuple(dims), bbmin=f32([0, 0, 0]), bbmax=f32(dims))


# uniform grids by cell count: one, two and three radix passes, bits_for at its edges
SORT_DIMS = {1: (1, 1, 1), 2: (1, 2, 1), 255: (15, 1, 17), 256: (16, 16, 1), 257: (1, 257, 1), 65535: (255, 257, 1),
             65536: (64, 64, 16), 65538: (198, 1, 331)}
SORT_BITS = {1: 1, 2: 1, 255: 8, 256: 8, 257: 9, 65535: 16, 65536: 16, 65538: 17}


@functools.lru_cache(maxsize=None)
def sort_case(O, cells):
    dims = SORT_DIMS[cells]
    rng = np.random.default_rng([20261106, cells])
    c = np.stack([rng.integers(0, dims[k], 700) for k in range(3)], 1)
    one = np.stack([ubox(dims, x, x) for x in c]) + rng.uniform(-0.3, 0.3, (700, 3, 3))
    hi = np.minimum(c[:60] + rng.integers(0, 6, (60, 3)), np.asarray(dims) - 1)
    some = np.stack([ubox(dims, a, b) for a, b in zip(c[:60], hi)])
    last = ubox(dims, np.asarray(dims) - 1, np.asarray(dims) - 1)[None]
    whole = ubox(dims, (0, 0, 0), np.asarray(dims) - 1)[None]
    tris = np.concatenate([one[:350], whole, some, one[350:], last, whole] if cells <= 257 else [one[:350], some, one[350:], last])
    return case("u", tris, **ucfg(dims))


STRIDE_DIMS = (64, 64, 16)


@functools.lru_cache(maxsize=None)
def stride_case(O, ntri):
    """ntri triangles that each cover all but the first x layer of a (64,64,16) grid, with one-cell triangles between."""
    rng = np.random.default_rng(20261107)
    big = ubox(STRIDE_DIMS, (1, 0, 0), np.asarray(STRIDE_DIMS) - 1)
    c = np.stack([rng.integers(0, STRIDE_DIMS[k], ntri) for k in range(3)], 1)
    one = np.stack([ubox(STRIDE_DIMS, x, x) for x in c])
    tris = np.stack([big[None].repeat(ntri, 0), one], 1).reshape(-1, 3, 3)
    return case("u", tris, **ucfg(STRIDE_DIMS))


# -- z-slabs (perspective and spherical): the family itself, and the corners of the slab stage
SLABS = (2, 3, 64)
SLAB_CASES = ("family", "equal", "single", "negative", "edges")


@functools.lru_cache(maxsize=None)
def slab_case(O, kind, name, slabs):
    fam = persp_family(O, None) if kind == "p" else sph_family(O, (32, 16))
    cfg = dict(rows=None) if kind == "p" else dict(lg=(32, 16))
    tri = fam.verts.reshape(-1, 3, 3).astype(np.float64)
    z = oracle(O, fam, slabs=slabs)["zmin"]
    if name == "family":
        t = tri
    elif name == "equal":  # one triangle fifty times: zMax == zMin, the slab is 0/0
        t = tri[np.flatnonzero(z > 0)[:1]].repeat(50, 0)
    elif name == "single":
        t = tri[np.flatnonzero(z > 0)[:1]]
    elif name == "negative":
        if kind == "p":
            neg = np.flatnonzero(z < 0)
            assert neg.size >= 10
            t = np.concatenate([tri[neg[:40]], tri[np.flatnonzero(z > 0)[:40]]])
        else:  # a radius is never negative; the only depth that is no positive number is the vertex at the light's: 0
            t = np.concatenate([tri[np.flatnonzero(z == 0)], tri[np.flatnonzero(z > 0)[:40]]])
    else:
        t = slab_edges(O, kind, slabs)
    return case(kind, t, slabs=slabs, **cfg)


def slab_edges(O, kind, slabs):
    """Depths that are exactly zMin + k (zMax - zMin) / slabs.  Spherical: the depth is the least of the radii, and points
    on +forward at the distances 1, 2 .. slabs + 1 are exact.  Perspective: a triangle between the nearest and the
    farthest whose depth is moved, float by float, to where its slab changes (flip_pairs on the oracle's slab list)."""
    if kind == "s":
        r = np.arange(1, slabs + 2, dtype=np.float64)
        P = SS.L + np.stack([r, np.zeros_like(r), np.zeros_like(r)], 1)
        return np.stack([P, P + [1.0, 0.25, 0.0], P + [1.0, 0.0, 0.25]], 1)
    cam, eye, dirs = camera(O)
    d = dirs[(PH // 2) * PW + PW // 2]
    near, far = eye + 1.5 * d, eye + 60.0 * d
    ends = np.stack([points_as_triangles(near[None])[0], points_as_triangles(far[None])[0]])

    def slab_of(P):
        out = np.zeros(len(P), np.int64)
        for i, q in enumerate(P):  # (each point with the two ends: the range is theirs)
            c = case("p", np.concatenate([ends, points_as_triangles(q[None].astype(np.float64))]), rows=None, slabs=slabs)
            out[i] = oracle(O, c)["zlist"][2]
        return out

    ts = np.array([1.6, 2.0, 3.0, 5.0, 10.0])
    A = f32(eye + ts[:, None] * d)
    B = A.copy()
    B[:, 2] = f32(eye + (ts * 1.5)[:, None] * d)[:, 2]
    Pa, Pb = flip_pairs(slab_of, A, B, 2)
    mids = np.concatenate([Pa, Pb]).astype(np.float64)
    return np.concatenate([ends, points_as_triangles(mids)])


# -- shards
def windows_of(F, nparts, wide_run=None):
    """Unequal windows; at 16 parts the first, the last and two in the middle are empty; one edge inside `wide_run`."""
    if nparts == 1:
        return [(0, F)]
    cut = (wide_run[0] + wide_run[1]) // 2 if wide_run else F // 5
    if nparts == 2:
        return [(0, cut), (cut, F)]
    rng = np.random.default_rng(20261108)
    inner = np.sort(np.concatenate([[cut], rng.choice(np.arange(1, F), 10, replace=False)]))
    edges = np.concatenate([[0, 0], inner[:5], [inner[5]] * 3, inner[6:], [F, F]])
    assert len(edges) == 17
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


SHARD_LETTERS = "n" * 150 + "b" * 150 + "w" * 100 + "n" * 100 + "b" * 100
SHARD_WIDE_RUN = (300, 400)


@functools.lru_cache(maxsize=None)
def shard_case(O, grid):
    cfg = dict(TAIL_GRIDS[grid])
    if grid == "u":
        cfg["bbmin"], cfg["bbmax"] = f32(cfg["bbmin"]), f32(cfg["bbmax"])
    return compose(O, grid, SHARD_LETTERS, **cfg)


# ------------------------------------------------------------------------------------------------ CPU: the inputs

@pytest.mark.parametrize("dims", UDIMS)
def test_uniform_boundary_inputs_can_fail(O, dims):
    """The family's PAIRS are one ulp apart and lie in different cells; vertices lie on every wall bit for bit, on the
    caller's box and outside the grid; an in-plane triangle lies in one layer of cells across its plane; the boxes and
    layer triangles between the deciding floats are one cell and the grid less one layer exactly, those from wall to wall
    are so only in part (counted)."""
    c = uniform_family(O, dims)
    g = oracle(O, c)
    v = c.verts.reshape(-1, 3)
    on_wall = sum(int(np.isin(bits(v[:, k]), bits(c.walls[k])).sum()) for k in range(3))
    outside = int(((v < [w[0] for w in c.walls]) | (v > [w[-1] for w in c.walls])).any(1).sum())
    print("uniform %r: F %d, R %d, cells used %d of %d, PAIRS %d, vertex coordinates on a wall %d, vertices outside the grid %d" % (
        dims, c.F, g["R"], g["used"], len(g["span"]), c.npairs, on_wall, outside))
    assert c.npairs >= 50 and on_wall >= 1000 and outside >= 100
    for k in range(3):  # every wall holds a vertex coordinate, and so does the float on either side
        for w in (c.walls[k], np.nextafter(c.walls[k], np.float32(-9)), np.nextafter(c.walls[k], np.float32(9))):
            assert np.isin(bits(w[1:-1]), bits(v[:, k])).all()
    assert np.isin(bits(UBOX[0]), bits(v)).all() and np.isin(bits(UBOX[1]), bits(v)).all()
    # a triangle in an interior cell-face plane lies in ONE layer of cells across that plane: the one above wall i where
    # (wall - lo) * inv rounds to i, the one below where it rounds to the float under i
    sizes = g["sizes"]
    tri = v.reshape(-1, 3, 3)[c.plane_faces]
    flat = [(bits(tri[:, 0, k]) == bits(tri[:, 1, k])) & (bits(tri[:, 0, k]) == bits(tri[:, 2, k])) for k in range(3)]
    assert np.any(flat, axis=0).all() and c.n_planes >= 12
    key = cell_fn(O, "u", dims=dims, bbmin=c.bbmin, bbmax=c.bbmax)(tri.reshape(-1, 3))
    idx = np.stack([key // (dims[1] * dims[2]), key // dims[2] % dims[1], key % dims[2]], 1).reshape(-1, 3, 3)
    layer = np.take_along_axis(idx, c.plane_axis[:, None, None].repeat(3, 1), 2)[:, :, 0]  # [triangle, vertex]
    upper = (layer == c.plane_wall[:, None]).all(1)
    lower = (layer == c.plane_wall[:, None] - 1).all(1)
    print("   in-plane triangles: %d, in the layer above their wall %d, below it %d" % (len(tri), upper.sum(), lower.sum()))
    assert (upper | lower).all() and upper.sum() >= 12
    assert 3 <= np.unique(sizes).size and (sizes == active_cells(c)).sum() >= 1  # (the far corners: a wide triangle)
    # boxes of one cell and the grid less one layer: between the deciding floats exactly that, from wall to wall in part
    full = active_cells(c)
    print("   boxes between the deciding floats: %d of %d one cell; layer triangles %r, expected %r" % (
        (sizes[c.exact_boxes] == 1).sum(), c.exact_boxes.size, sizes[c.exact_layers].tolist(), c.layer_sizes.tolist()))
    print("   boxes from wall to wall: sizes %r; layer triangles %r of %d" % (
        dict(zip(*[x.tolist() for x in np.unique(sizes[c.wall_boxes], return_counts=True)])), sizes[c.wall_layers].tolist(), full))
    assert (sizes[c.exact_boxes] == 1).all() and c.exact_boxes.size == 120
    assert (sizes[c.exact_layers] == c.layer_sizes).all() and (c.layer_sizes < full).all() and c.layer_sizes.size >= 4
    assert (sizes[c.wall_boxes] == 1).sum() >= 10 and (sizes[c.wall_boxes] > 1).sum() >= 10
    assert np.isin(sizes[c.wall_layers], np.concatenate([c.layer_sizes, [full]])).sum() >= 2


@pytest.mark.parametrize("rows", [None, BAND])
def test_perspective_boundary_inputs_can_fail(O, rows):
    c = persp_family(O, rows)
    g = oracle(O, c)
    sizes = g["sizes"].astype(np.int64)
    full = active_cells(c)
    st = tail_stats(c, g)
    z = oracle(O, c, slabs=2)["zmin"]
    print("perspective rows %r: F %d, R %d, cells used %d of %d, PAIRS %d, wide %d, off the band %d, non-finite depths %d, "
          "straddling triangles that are wide %d of %d" % (rows, c.F, g["R"], g["used"], len(g["span"]), c.npairs, st.W,
                                                        (sizes == 0).sum(), (~np.isfinite(z)).sum(),
                                                        (sizes[c.straddle] == full).sum(), c.straddle.size))
    assert c.npairs >= 300 and c.n_on_ray >= 500  # (every tile corner of the frame and 400 points of tile edges)
    assert (sizes[c.straddle] == full).all() and c.straddle.size == 20  # across the eye plane and over the screen: wide
    assert (z < 0).sum() >= 10
    # finite inputs, non-finite intermediates: a triangle with the eye itself as a vertex (the divisor is 0) has no finite depth
    at_eye = (c.verts.reshape(-1, 3, 3).view(np.uint32) == bits(camera(O)[0].worldori[:3])).all(2).any(1)
    assert at_eye.sum() >= 61 and (~np.isfinite(z[at_eye])).all() and np.isfinite(c.verts).all()
    if rows is not None:
        # (the oracle clamps the stored range to the band: the cut ones are counted on the full frame's ranges)
        rf = oracle(O, persp_family(O, None))["rng"].reshape(-1, 4)
        cut_first = (rf[:, 2] < rows[0]) & (rf[:, 3] >= rows[0]) & (rf[:, 3] < rows[1])
        cut_last = (rf[:, 2] < rows[1]) & (rf[:, 3] >= rows[1]) & (rf[:, 2] >= rows[0])
        print("   cut by the band's first row %d, by its last %d" % (cut_first.sum(), cut_last.sum()))
        assert (sizes == 0).sum() >= 100 and cut_first.sum() >= 10 and cut_last.sum() >= 10


@pytest.mark.parametrize("lg", SPH_GRIDS)
def test_spherical_boundary_inputs_can_fail(O, lg):
    c = sph_family(O, lg)
    g = oracle(O, c)
    r = g["rng"].reshape(-1, 4)
    print("spherical %r: F %d, R %d, cells used %d of %d, PAIRS %d (seam %d, poles %d), rows %d, columns %d, wide %d" % (
        lg, c.F, g["R"], g["used"], len(g["span"]), c.npairs, c.n_seam, c.n_pole, np.unique(r[:, 2:]).size,
        np.unique(r[:, :2]).size, tail_stats(c, g).W))
    assert c.npairs >= 100 and (c.n_seam >= 10 or lg[0] == 2)  # (two columns: the column is the same on either side)
    assert c.n_pole >= 200
    # every cell row and every column occurs (a grid of 4096 in one axis has more of them than the family has triangles)
    for met, n in ((np.unique(r[:, 2:]).size, lg[1]), (np.unique(r[:, :2]).size, lg[0])):
        assert met == n if n <= 256 else met >= 1500, (met, n)
    assert (c.verts.reshape(-1, 3).view(np.uint32) == bits(f32(SS.L))).all(1).sum() >= 4  # the vertex at the light, bit for bit


def test_pairs_are_adjacent_floats_in_different_cells(O):
    """flip_pairs on each grid: the two points differ by one ulp in one coordinate and the oracle bins them apart."""
    rng = np.random.default_rng(5)
    for kind, cfg, A, B, axis in (
            ("u", dict(dims=(12, 10, 3), bbmin=UBOX[0], bbmax=UBOX[1]), rng.uniform(0.15, 0.4, (50, 3)), 0.45, 0),
            ("p", dict(rows=None), camera(O)[1] + 10.0 * camera(O)[2][rng.integers(0, PW * PH, 50)], 6.0, 0),
            ("s", dict(lg=(32, 16)), SS.L + 5.0 * unit(rng.normal(size=(50, 3))), 3.0, 1)):
        cell_of = cell_fn(O, kind, **cfg)
        A = f32(A)
        Bp = A.copy()
        Bp[:, axis] += np.float32(B)
        Pa, Pb = flip_pairs(cell_of, A, Bp, axis)
        assert len(Pa) >= 10
        assert (np.abs(to_ord(Pa[:, axis]) - to_ord(Pb[:, axis])) == 1).all()
        assert (cell_of(Pa) != cell_of(Pb)).all()
        other = [k for k in range(3) if k != axis]
        assert (bits(Pa[:, other]) == bits(Pb[:, other])).all()


@pytest.mark.parametrize("grid,name", TAIL_CASES)
def test_tail_cases_meet_their_branch(O, grid, name):
    """From the oracle's sizes and scan: the case's figures are the ones its name promises."""
    c = tail_case(O, grid, name)
    st = tail_stats(c, oracle(O, c))
    print("%s %s: F %d, wide %d, narrow references %d in %d parts, longest part %d triangles, %d parts inside one triangle, "
          "longest narrow run of a cell %d, R %d" % (grid, name, st.F, st.W, st.Rn, st.nparts, st.nrun_max, st.whole_parts,
                                                      st.longest, st.R))
    for k, v in c.expect.items():
        got = getattr(st, k)
        assert (list(got) == v) if isinstance(v, list) else (got == v), (k, got, v)
    assert st.R == st.Rn + st.W * st.full
    if name == "one_fills_parts":
        assert st.whole_parts >= 1  # f_first == f_last
    if name == "W_padded_wave":
        assert st.F % 256 != 0 and st.waves[-1] == (st.F - 1) // 64
    if name == "W_spread":
        assert st.waves.size >= 30 and np.unique(st.waves // 4).size >= 10


def test_fill_parts_span_both_sides_of_the_lds_run(O):
    """Over the tail cases of each grid: parts of exactly FILL_LDS triangles and of more, in the uniform and the
    spherical grid behind wide triangles, in the perspective band also behind off-band ones."""
    for grid in TAIL_GRIDS:
        runs = np.concatenate([tail_stats(c, oracle(O, c)).nrun for c in
                               (tail_case(O, g, n) for g, n in TAIL_CASES if g == grid)])
        assert (runs == FILL_LDS).any() and (runs > FILL_LDS).any() and (runs == 1).any(), grid
    for name in ("off1024", "off1025"):
        assert tail_stats(tail_case(O, "pband", name), oracle(O, tail_case(O, "pband", name))).W == 0


def test_one_and_two_cell_grids(O):
    """`full > 1`: a grid of one cell has no wide triangle, a grid of two has."""
    one, two = sort_case(O, 1), sort_case(O, 2)
    s1, s2 = tail_stats(one, oracle(O, one)), tail_stats(two, oracle(O, two))
    assert s1.full == 1 and s1.W == 0 and s1.Rn == s1.F == s1.R
    assert s2.full == 2 and s2.W >= 2 and s2.Rn > 0


@pytest.mark.parametrize("cells", sorted(SORT_DIMS))
def test_sort_cases_have_their_cell_counts(O, cells):
    c = sort_case(O, cells)
    g = oracle(O, c)
    st = tail_stats(c, g)
    print("%d cells %r: F %d, R %d, wide %d, cells used %d, sort bits %d" % (cells, c.dims, c.F, st.R, st.W, st.used, st.bits))
    assert st.cells == cells == int(np.prod(SORT_DIMS[cells])) and st.bits == SORT_BITS[cells]
    assert g["span"][-1] >= 1  # the last cell is used: the highest key occurs
    # 65 537 is prime, and no dims within the ABI's [1,1024] multiply to it
    assert all(65537 % d for d in range(2, 1025))


def test_stride_cases_cross_the_fill_s_block_limits(O):
    for ntri, limit in ((20, FILL_MAX_BLOCKS_COUNTING), (40, FILL_MAX_BLOCKS)):
        c = stride_case(O, ntri)
        st = tail_stats(c, oracle(O, c))
        print("%d triangles over all but one layer of %r: %d narrow references, %d parts (limit %d)" % (
            ntri, STRIDE_DIMS, st.Rn, st.nparts, limit))
        assert st.W == 0 and st.nparts > limit and st.whole_parts > 1000
    assert st.Rn > 2000000 and tail_stats(stride_case(O, 20), oracle(O, stride_case(O, 20))).nparts <= FILL_MAX_BLOCKS


@pytest.mark.parametrize("kind", ["p", "s"])
@pytest.mark.parametrize("slabs", SLABS)
def test_slab_cases_meet_their_corner(O, kind, slabs):
    for name in SLAB_CASES:
        c = slab_case(O, kind, name, slabs)
        g = oracle(O, c)
        z, (zlo, zhi), zl = g["zmin"], g["zrange"], g["zlist"]
        print("%s slabs %d %s: F %d, R %d, zMin %r zMax %r, slabs used %d, depths < 0: %d, not finite: %d" % (
            kind, slabs, name, c.F, g["R"], zlo, zhi, np.unique(zl).size, (z < 0).sum(), (~np.isfinite(z)).sum()))
        assert len(g["span"]) == active_cells(c) * slabs
        if name in ("equal", "single"):
            assert zlo == zhi and c.F == (1 if name == "single" else 50)
        if name == "negative":
            assert ((z < 0).sum() >= 10) if kind == "p" else ((z == 0).sum() >= 1)
            assert (zl[~(z >= 0)] == 0).all()
        if name == "edges":
            with np.errstate(all="ignore"):
                x = np.float32(slabs) * ((z - np.float32(zlo)) / (np.float32(zhi) - np.float32(zlo))).astype(np.float32)
            on_edge = (x == np.floor(x)) & (x > 0) & (x < slabs)
            if kind == "s":
                assert on_edge.sum() >= 1 and np.unique(zl).size == slabs
            else:  # pairs of depths one float apart whose slabs differ
                assert c.F >= 4 and (zl[2:2 + (c.F - 2) // 2] != zl[2 + (c.F - 2) // 2:]).all()
        if name == "family":
            assert np.unique(zl).size >= 2


@pytest.mark.parametrize("grid", ["u", "s"])
def test_shard_windows(O, grid):
    """The windows are unequal, at 16 parts four are empty (first, last, two in the middle), one edge lies inside the
    run of wide triangles; by the oracle the shards' references add up to the full build's."""
    c = shard_case(O, grid)
    full = oracle(O, c)
    st = tail_stats(c, full)
    assert st.wide[SHARD_WIDE_RUN[0]:SHARD_WIDE_RUN[1]].all() and st.W == 100
    for nparts in (1, 2, 16):
        w = windows_of(c.F, nparts, SHARD_WIDE_RUN)
        assert len(w) == nparts and w[0][0] == 0 and w[-1][1] == c.F and all(a[1] == b[0] for a, b in zip(w, w[1:]))
        assert nparts == 1 or any(SHARD_WIDE_RUN[0] < a < SHARD_WIDE_RUN[1] for a, _ in w)
        if nparts == 16:
            empty = [i for i, (a, b) in enumerate(w) if a == b]
            assert 0 in empty and 15 in empty and len(empty) == 4 and len({b - a for a, b in w}) > 4
        assert sum(oracle(O, c, window=x)["R"] for x in w) == full["R"]


# -- the arbiter of the uniform grid: the brute force
@pytest.fixture(scope="module")
def OC(tmp_path_factory):
    """oc_trace_any / oc_brute_any of tests/occlusion_ref.c."""
    import ctypes
    import os
    import subprocess

    import test_reflect_shadows as RS

    out = str(tmp_path_factory.mktemp("grid_build_synthetic") / "libocclusion_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(RS.HERE, "occlusion_ref.c"), "-lm"], check=True, capture_output=True)
    return RS.OcclusionRef(ctypes.CDLL(out))


@functools.lru_cache(maxsize=None)
def family_rays(O, dims):
    """Rays at interior points of the uniform family's triangles: along the normal from both sides, and along each axis
    from both sides; those in cell-face planes included.  -> rays [n, 6], the point aimed at, its triangle."""
    c = uniform_family(O, dims)
    rng = np.random.default_rng([20261109, dims[0]])
    v = c.verts.reshape(-1, 3, 3).astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    # (not the PAIRS' triangles: two of them coincide but for one ulp of one vertex and tie in t; the walk keeps the one
    # whose cell it meets first, the brute force the lower id, and ties are not what this is about)
    ok = np.flatnonzero((area > 1e-4) & (np.abs(v).max((1, 2)) < 2.0) & ~c.pair_faces)
    k = np.concatenate([ok, c.plane_faces, c.plane_faces])
    b = 0.15 + 0.55 * rng.dirichlet([1, 1, 1], k.size)
    Q = (v[k] * b[:, :, None]).sum(1)
    n = nrm[k] / area[k, None]
    dirs = np.concatenate([n, -n] + [np.broadcast_to(s * np.eye(3)[a], n.shape) for a in range(3) for s in (1.0, -1.0)])
    Q, k = np.tile(Q, (8, 1)), np.tile(k, 8)
    grazing = np.abs((dirs * np.tile(n, (8, 1))).sum(1)) < 0.05
    Q, k, dirs = Q[~grazing], k[~grazing], dirs[~grazing]
    o = f32(Q - dirs * rng.uniform(0.005, 0.05, (len(Q), 1)))
    d = f32(unit(Q - o.astype(np.float64)))
    lo, hi = np.array([w[0] for w in c.walls]), np.array([w[-1] for w in c.walls])
    inside = ((Q > lo) & (Q < hi)).all(1) & ((o > lo) & (o < hi)).all(1)  # the walk sees what lies inside the grid
    return np.concatenate([o, d], 1)[inside], Q[inside], k[inside]


@pytest.mark.parametrize("dims", UDIMS)
def test_uniform_family_walk_equals_brute_force(O, OC, dims):
    """O.trace_dda over O.grid_uniform of the family == O.brute_nearest on rays at its triangles; a ray may differ only
    where its float64 hit point lies on a cell face, and 0.1 % of the rays at the most do."""
    c = uniform_family(O, dims)
    g = oracle(O, c)
    rays, Q, k = family_rays(O, dims)
    N = len(rays)
    act = np.ones(N, np.int32)
    t, ids, _ = O.trace_dda(g, c.verts, c.faces, rays.reshape(-1), act, 0, N, N)
    bt, bids = O.brute_nearest(c.verts, c.faces, rays.reshape(-1), act, 0, N, N)
    differ = np.flatnonzero((ids != bids) | (bits(t) != bits(bt)))
    in_plane = np.isin(k, c.plane_faces)
    print("uniform %r: %d rays (%d at triangles in a cell-face plane), %d hit, %d hit their own triangle, %d differ from the "
          "brute force" % (dims, N, in_plane.sum(), (bids >= 0).sum(), (bids == k).sum(), differ.size))
    assert (bids >= 0).sum() >= 0.9 * N and (bids[in_plane] == k[in_plane]).sum() >= 100
    hit = rays[differ, :3].astype(np.float64) + bt[differ, None].astype(np.float64) * rays[differ, 3:].astype(np.float64)
    lo, cs = g["ug"][0:3].astype(np.float64), g["ug"][3:6].astype(np.float64)
    x = (hit - lo) / cs
    on_face = (np.abs(x - np.round(x)) < 1e-5).any(1)
    assert on_face.all() and differ.size <= 1e-3 * N, (differ.size, (~on_face).sum())
    # the any-hit walk around the hit: t_max one float below, at and above it
    # oc_trace_any takes one t_max per call.  With t_max one float below and at the hit: every ray.  One float above it:
    # every ray whose nearest triangle lies in no axis plane, and 30 of those whose
    # nearest one does (the in-plane triangles, and those of the others whose three vertices drew the same wall or the
    # floats next to it).  The walk
    # visits the cells whose entry parameter is below t_max; a hit on a triangle in a cell-face plane IS its cell's entry,
    # so with t_max one float above it the visit hangs on the rounding of the entry: about one such ray in ten differs.
    # That is the exemption (the hit point lies on a cell face), and these rays are few enough here to stay inside the cap.
    rng = np.random.default_rng([20261110, dims[0]])
    hits = bids >= 0
    tv = c.verts.reshape(-1, 3, 3)
    flat = (tv.max(1) - tv.min(1) < 1e-6).any(1)  # (a wall and the floats on either side of it count as one plane)
    flat_hit = hits & flat[np.maximum(bids, 0)]
    sample = np.concatenate([rng.choice(np.flatnonzero(flat_hit), 30, replace=False), np.flatnonzero(hits & ~flat_hit)])
    one = np.ones(1, np.int32)
    hit64 = rays[:, :3].astype(np.float64) + bt[:, None].astype(np.float64) * rays[:, 3:].astype(np.float64)
    x = (hit64 - lo) / cs
    on_face = (np.abs(x - np.round(x)) < 1e-5).any(1)
    for name, tm in (("below", np.nextafter(bt, np.float32(-1))), ("at", bt), ("above", np.nextafter(bt, np.float32(9e9)))):
        bad, occluded = [], 0
        sel = sample if name == "above" else np.flatnonzero(hits)  # (below and at the hit: every ray)
        for p in sel:
            w = OC.trace_any(g, c.verts, c.faces, rays[p], one, float(tm[p]), 0, 1, 1)
            b = OC.brute_any(c.verts, c.faces, rays[p], one, float(tm[p]), 0, 1, 1)
            if w[0] != b[0]:
                bad.append(p)
            occluded += int(b[0] != 0)
        print("   any-hit, t_max %s the hit: %d of %d rays occluded by the brute force, %d differ (%d of them on a triangle "
              "in an axis plane, %d with the hit on a cell face)" % (name, occluded, sel.size, len(bad), flat_hit[bad].sum(),
                                                              on_face[bad].sum()))
        assert on_face[bad].all() and len(bad) <= 1e-3 * sel.size


# ------------------------------------------------------------------------------------------------ the reference's kernels

REF_STAGES = ("persp", "sph", "pslab", "lslab")
RECORD = "buildsyn"
REF_LG = (32, 16)
REF_SLABS = 3


def ref_families(O):
    return persp_family(O, None), sph_family(O, REF_LG)


def ref_stage_inputs(O):
    """The perspective family (full frame) and the spherical family at (32,16) as the reference's count, slab and fill
    kernels take them (oracle/ref_kernels.cpp), every input the oracle's."""
    fp, fs = ref_families(O)
    gp, gs = oracle(O, fp), oracle(O, fs)
    zp, zs = oracle(O, fp, slabs=REF_SLABS), oracle(O, fs, slabs=REF_SLABS)
    cc, lcc = camera(O)[0].cc, light(O).cc
    nbx, nby = PW // 8, PH // 8
    p = dict(cc=cc, faces=fp.faces.reshape(-1), verts=fp.verts.reshape(-1), nbx=nbx, nby=nby)
    l = dict(cc=lcc, faces=fs.faces.reshape(-1), verts=fs.verts.reshape(-1), nbx=REF_LG[0], nby=REF_LG[1], xM=PI_F, yM=PI_F)
    return {"persp": dict(p, scan=gp["scan"]), "sph": dict(l, scan=gs["scan"]),
            "pslab": dict(p, scan=zp["scan"], zmin=zp["zmin"], zMin=zp["zrange"][0], zMax=zp["zrange"][1], slabs=REF_SLABS,
                          spherical=0),
            "lslab": dict(l, scan=zs["scan"], zmin=zs["zmin"], zMin=zs["zrange"][0], zMax=zs["zrange"][1], slabs=REF_SLABS,
                          spherical=1)}


def nan_angle_triangles(O):
    """The spherical family's triangles with a vertex whose column or row angle is acos(0/0) by construction: at L, on
    +-up (the column's projection has length 0) or on +-right (the row's)."""
    fs = sph_family(O, REF_LG)
    d = fs.verts.reshape(-1, 3, 3).astype(np.float64) - SS.L
    on_up, on_right = (d[:, :, 0] == 0) & (d[:, :, 2] == 0), (d[:, :, 0] == 0) & (d[:, :, 1] == 0)
    return (on_up | on_right).any(1)


def pinned(O, stage, out):
    """What of a stage's outputs is compared with the reference's kernels.  They are compiled for the host here, where the
    (int) of a NaN angle in getEffective_x/y is INT_MIN or whatever else the host's conversion leaves; on the GPU it is 0,
    which is what the oracle and the product compute (tests/test_shadow_synthetic.py: pinned).  So the spherical family's
    triangles with such a vertex are left out: their sizes, and the references the fill writes for them (the fill takes
    the oracle's scan, so their places in the lists are the same on either side)."""
    if stage in ("persp", "pslab"):
        return out
    fs = sph_family(O, REF_LG)
    keep = ~nan_angle_triangles(O)
    scan = oracle(O, fs, slabs=REF_SLABS if stage == "lslab" else 1)["scan"].astype(np.int64)
    owner = np.searchsorted(scan, np.arange(scan[-1]), side="right")
    res = dict(out)
    for k in ("sizes", "zmin", "zlist"):
        if k in out:
            res[k] = np.ascontiguousarray(out[k])[keep]
    for k in ("keys", "vals"):
        res[k] = np.ascontiguousarray(out[k])[keep[owner]]
    return res


def ref_oracle_outputs(O):
    fp, fs = ref_families(O)
    gp, gs = oracle(O, fp), oracle(O, fs)
    zp, zs = oracle(O, fp, slabs=REF_SLABS), oracle(O, fs, slabs=REF_SLABS)
    pk, pv = O.fill_2d(gp["rng"], gp["scan"], PH // 8)
    sk, sv = O.fill_2d(gs["rng"], gs["scan"], REF_LG[1])
    zpk, zpv = O.fill_slabs(zp["rng"], zp["scan"], zp["zlist"], PH // 8, REF_SLABS)
    zsk, zsv = O.fill_slabs(zs["rng"], zs["scan"], zs["zlist"], REF_LG[1], REF_SLABS)
    return {"persp": dict(sizes=gp["sizes"], zmin=gp["zmin"], keys=pk, vals=pv),
            "sph": dict(sizes=gs["sizes"], zmin=gs["zmin"], keys=sk, vals=sv),
            "pslab": dict(zlist=zp["zlist"], keys=zpk, vals=zpv), "lslab": dict(zlist=zs["zlist"], keys=zsk, vals=zsv)}


def test_oracle_equals_reference_kernels_on_the_boundary_families(O):
    """The record of the reference's own count, slab and fill kernels on the two families (tests/golden/
    ref_kernels_buildsyn.npz, written by tests/golden/make_ref_kernels.py) against the oracle, always; the live kernels
    where they are built.  The perspective family is compared whole, vertices on the eye plane included."""
    import test_reference_kernels as RK

    rec = RK.load_record(RECORD)
    ins, outs = ref_stage_inputs(O), ref_oracle_outputs(O)
    nan = nan_angle_triangles(O)
    print("reference record: %d of the spherical family's %d triangles hold a vertex with a NaN angle and are left out" % (
        nan.sum(), nan.size))
    assert 100 <= nan.sum() <= 0.3 * nan.size
    for stage in REF_STAGES:
        assert RK.input_sha(ins[stage]) == str(rec[stage + "/input_sha"]), \
            "%s: stage inputs differ from the recorded ones (generator or oracle drift)" % stage
        RK.assert_matches_record(rec, RECORD, stage, pinned(O, stage, outs[stage]), "oracle")
    if O.ref_kernels_live():
        for stage in REF_STAGES:
            got = RK.run_reference(RECORD, stage, ins[stage])
            RK.assert_matches_record(rec, RECORD, stage, pinned(O, stage, got), "reference")
            if stage == "sph":  # outside the triangles left out nothing differs, and inside them something does
                differs = np.ascontiguousarray(got["sizes"]) != outs["sph"]["sizes"]
                assert not (differs & ~nan).any() and differs.any()


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Builder:
    """Contexts by configuration; a case is uploaded, built through the C ABI and compared with the oracle."""

    def __init__(self, ugrt, O):
        self.ugrt, self.O, self.ctxs = ugrt, O, {}

    def ctx_of(self, c, fresh=False):
        key = (c.kind, c.rows, c.slabs, c.lg, tuple(c.dims) if c.dims else None, c.img)
        if fresh or key not in self.ctxs:
            ctx = self.ugrt.Context(c.img[0], c.img[1], light_grid=c.lg or (16, 8), rows=c.rows, uniform_dims=c.dims or (8, 8, 8),
                                    slabs=c.slabs)
            ctx.set_option("uniform_reuse", 0)
            ctx.set_option("light_reuse", 0)
            if fresh:
                return ctx
            self.ctxs[key] = ctx
        return self.ctxs[key]

    def which(self, c):
        u = self.ugrt
        return {"u": u.GRID_UNIFORM, "p": u.GRID_PERSPECTIVE, "s": u.GRID_SPHERICAL}[c.kind]

    def upload(self, ctx, c):
        return ctx.upload(c.faces.reshape(-1)), ctx.upload(c.verts.reshape(-1))

    def build(self, ctx, c, dev):
        df, dv = dev
        if c.kind == "u":
            ctx.grid_build_uniform(df, dv, c.F, c.bbmin, c.bbmax)
        elif c.kind == "p":
            ctx.upload_camera(camera(self.O, c.img)[0].cc)
            ctx.grid_build_perspective(df, dv, c.F)
        else:
            ctx.upload_camera(light(self.O).cc)
            ctx.grid_build_spherical(df, dv, c.F, PI_F, PI_F)

    def arrays(self, ctx, c):
        ctx.synchronize()
        value, key, span, offset, gi = ctx.grid_arrays(self.which(c))
        ctx.synchronize()
        return dict(keys=u32(key).copy(), vals=u32(value).copy(), span=u32(span).copy(), offset=u32(offset).copy(),
                    R=int(gi.total_refs), used=int(gi.cells_used), cells=int(gi.num_cells))

    def check(self, ctx, c, want, what):
        got = self.arrays(ctx, c)
        assert got["R"] == want["R"], "%s: total_refs %d, oracle %d" % (what, got["R"], want["R"])
        assert got["cells"] == len(want["span"]), "%s: num_cells" % what
        for name in ("span", "offset", "keys", "vals"):
            np.testing.assert_array_equal(got[name], want[name], err_msg="%s: %s" % (what, name))
        assert got["used"] == want["used"], "%s: cells_used %d, oracle %d" % (what, got["used"], want["used"])
        if c.slabs > 1:
            si = ctx.grid_slabs(self.which(c))
            assert si.slabs == c.slabs
            zr = np.array([si.z_min, si.z_max], np.float32)
            assert (bits(zr) == bits(np.array(want["zrange"], np.float32))).all(), "%s: zMin/zMax %r, oracle %r" % (what, zr, want["zrange"])
            pz = u32(ctx.wrap_u32(si.d_proj_coord_z, c.F)).view(np.float32)
            same = (bits(pz) == bits(want["zmin"])) | (np.isnan(pz) & np.isnan(want["zmin"]))
            assert same.all(), "%s: projCoordZ differs for %d triangles" % (what, (~same).sum())

    def forms(self, c, want=None, ctx=None, batch=True, options=()):
        """The waiting build, the second build of the same inputs under async_build 1, and (uniform, spherical) a batch.
        The library takes the asynchronous form only with one slab and up to 3000 wide triangles in the build before
        (build_common); the slab cases, W4096 and W4097 are therefore built a second time in the waiting form, and in a
        batch at once.  No state tells which form ran."""
        want = oracle(self.O, c) if want is None else want
        ctx = self.ctx_of(c) if ctx is None else ctx
        dev = self.upload(ctx, c)
        if c.window is not None:
            ctx.set_face_window(*c.window)
        try:
            for key, value in options:
                ctx.set_option(key, value)
            ctx.set_option("async_build", 0)
            self.build(ctx, c, dev)
            self.check(ctx, c, want, "waiting")
            ctx.set_option("async_build", 1)
            self.build(ctx, c, dev)
            self.check(ctx, c, want, "second build, async_build 1")
            if batch and c.kind != "p":
                ctx.grid_build_batch_begin()
                self.build(ctx, c, dev)
                ctx.grid_build_batch_end()
                self.check(ctx, c, want, "batch")
        finally:
            ctx.set_option("async_build", 0)
            for key, _ in options:
                ctx.set_option(key, -1)
            if c.window is not None:
                ctx.set_face_window(0, -1)


@pytest.fixture(scope="module")
def B(ugrt, O, torch):
    b = Builder(ugrt, O)
    yield b
    b.ctxs.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", UDIMS)
def test_uniform_boundary_family(B, O, dims):
    B.forms(uniform_family(O, dims))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [None, BAND])
def test_perspective_boundary_family(B, O, rows):
    B.forms(persp_family(O, rows))


@pytest.mark.gpu
@pytest.mark.parametrize("lg", SPH_GRIDS)
def test_spherical_boundary_family(B, O, lg):
    B.forms(sph_family(O, lg))


@pytest.mark.gpu
@pytest.mark.parametrize("grid,name", TAIL_CASES)
def test_tail_case(B, O, grid, name):
    B.forms(tail_case(O, grid, name))


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["p", "pband"])
def test_the_screen_grid_puts_its_merge_off_up_to_4096_wide_triangles(B, O, grid):
    """build_defers_merge: a waiting build of the screen grid with 1 .. 4096 wide triangles leaves the merge to whoever
    asks for the lists (the rank kernel orders the ids then); with 4097 the radix sort orders them and the merge runs at
    once, and with none there is nothing to merge.  Asking for the arrays completes a pending merge."""
    for name, put_off in (("W4096", 1), ("W4097", 0), ("no_wide", 0), ("W1", 1), ("all_wide", 1), ("W1025", 1)):
        c = tail_case(O, grid, name)
        ctx = B.ctx_of(c)
        dev = B.upload(ctx, c)
        before = ctx.get_state("primary_deferred_merges"), ctx.get_state("primary_completed_merges")
        B.build(ctx, c, dev)
        assert ctx.get_state("primary_merge_pending") == put_off, name
        assert ctx.get_state("primary_deferred_merges") - before[0] == put_off, name
        B.check(ctx, c, oracle(O, c), "%s, waiting" % name)
        assert ctx.get_state("primary_merge_pending") == 0
        assert ctx.get_state("primary_completed_merges") - before[1] == put_off, name


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["u", "s"])
def test_a_grid_no_triangle_touches(B, O, grid):
    """An empty face window: R = 0 and W = 0, every span 0."""
    c = tail_case(O, grid, "no_wide")
    c = case(c.kind, c.verts.reshape(-1, 3, 3), window=(7, 7), **{k: getattr(c, k) for k in ("dims", "bbmin", "bbmax", "lg")})
    want = oracle(O, c)
    assert want["R"] == 0 and want["used"] == 0
    B.forms(c, want)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", sorted(TAIL_GRIDS))
def test_one_context_builds_the_tail_cases_in_turn(B, O, grid):
    """Large then small, W > 0 then W = 0 and back, in one context: buffers with stale contents, the wide counter that
    the span scan resets, an asynchronous build behind a waiting build of other inputs' size."""
    order = ["W4097", "R1", "all_wide", "no_wide", "W1025", "R257", "parts1027", "R256", "W_spread", "run1025", "W1", "R1",
             "W4096", "no_wide", "W65"]
    ctx = B.ctx_of(tail_case(O, grid, "R1"), fresh=True)
    for name in order:
        B.forms(tail_case(O, grid, name), ctx=ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(SORT_DIMS))
def test_sort_bits_and_passes(B, O, cells):
    B.forms(sort_case(O, cells))


@pytest.mark.gpu
@pytest.mark.parametrize("ntri", [20, 40])
def test_fill_grid_stride(B, O, ntri):
    """More parts than the fill launches workgroups: with the first sort digit counted in the fill (the waiting and the
    asynchronous build), without (a batch, and the library sort)."""
    c = stride_case(O, ntri)
    want = oracle(O, c)
    B.forms(c, want)
    B.forms(c, want, batch=False, options=(("sort_library", 1),))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["p", "s"])
@pytest.mark.parametrize("slabs", SLABS)
def test_slabs(B, O, kind, slabs):
    for name in SLAB_CASES:
        B.forms(slab_case(O, kind, name, slabs))


@pytest.mark.gpu
@pytest.mark.parametrize("nparts", [1, 2, 16])
@pytest.mark.parametrize("grid", ["u", "s"])
def test_shards_and_their_merge(B, O, grid, nparts):
    """Each shard (set_face_window) equals O.grid_*(window=), and ugrt_grid_merge_shards of them the oracle's full build."""
    c = shard_case(O, grid)
    ctx = B.ctx_of(c)
    dev = B.upload(ctx, c)
    parts = []
    try:
        for w in windows_of(c.F, nparts, SHARD_WIDE_RUN):
            ctx.set_face_window(*w)
            want = oracle(O, c, window=w)
            for async_build in (0, 1):  # (the second build of a window runs on the first one's counts)
                ctx.set_option("async_build", async_build)
                B.build(ctx, c, dev)
                B.check(ctx, c, want, "shard %r, async_build %d" % (w, async_build))
            value, key, span, offset, gi = ctx.grid_arrays(B.which(c))
            parts.append((key.clone(), value.clone(), span.clone(), int(gi.total_refs)))
        ctx.grid_merge_shards(B.which(c), [p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts],
                              [p[3] for p in parts])
        B.check(ctx, c, oracle(O, c), "merge of %d shards" % nparts)
    finally:
        ctx.set_option("async_build", 0)
        ctx.set_face_window(0, -1)
