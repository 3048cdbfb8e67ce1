"""The primary pass's culls (d_cull_cr: tile box, d_cull_cr4: quadrant boxes, d_cull_tlow: depth bound, all of
csrc/ugrt_packet.h) on triangles placed under the camera's own rays: edge-on hits on the corners of the direction boxes,
and pairs of tile-filling triangles whose depths differ by the depth bound's margin.

The other primary tests render cornell, hall, crash and random soups: rays that pass the exact test on a triangle by
less than a cull's margin do not occur there, and the oracle tests every reference of a cell, so a cull that drops what
the exact test accepts goes unseen.  Here each pixel's float32 direction is taken from the oracle (O.trace_primary,
"dir") and the triangles are placed under chosen rays with numpy in float64, rounded once to float32, seeded:
* chosen pixels, per 8 x 8 tile: the four corners (lanes 0, 7, 56, 63: the corners of the tile's direction box), the
  four pixels where the 4 x 4 quadrants meet (lanes 27, 28, 35, 36: corners of the quadrant boxes that d_cull_cr4 gives
  one shared radius), and 16 other pixels at random;
* each gets one small triangle with a point of an edge (70 %) or a vertex (30 %) on the pixel's ray, at a distance
  log-uniform over 1 .. 100, footprint 0.3 to 3 pixels, either winding (the sign of det selects the side of
  d_cull_decide), any of its edges or vertices; a share of them moved off the ray by 1e-6 and by 1e-5 of the distance;
* depth pairs, on the tiles of even column and even row (their triangles do not reach each other's tiles): two tilted
  triangles that each cover the whole tile, at a distance of 300 .. 600 (behind every small triangle), the second in
  list order closer than the first by a relative gap of 0, 1e-7, 1e-6,
  1e-5 or 1e-4 (gap 0: the same plane through other vertices, so that T and det round differently), and the same in
  the reverse order; also by 1e-2 and 0.3, where the bound does drop the farther one.  The bound may drop only what
  cannot win under the strict `<`.
Cases: "near" 128 x 64, the eye near the coordinate origin; "far" the same scene and eye moved 1e3 scene extents (1e5)
away: float32 then resolves 0.008, more than a pixel's width at a distance of 1, so its nearest triangles are whatever
the rounding left of them.  That case does NOT test the margins (no edge lies on its ray any more, and the build without
margins passes it): it tests long lists and large coordinates, and the sharpness assertions leave it out; "band"
72 x 40, tile rows 1 .. 5; "wide" = near plus six view-filling triangles behind
everything (the wide-list path of k_trace_primary); "narrow" 512 x 256 with a field of view of 0.05 degrees from the
coordinate origin along +z: small triangles on the tiles of odd column and row, pairs 0 and 1e-7 apart that face the eye
on the tiles of even column and row, 128 pairs per gap and order.  There a tile is 2.7e-5 rad across, t is the same on
all of a tile's rays to 1e-10 and the tile box's bound of det is det to 1e-9, so d_cull_tlow differs from the rays' own
t by rounding alone: mT, mD, the boxes' floor and the factor 0.99988 are what keeps the second triangle of a pair.  The
bound is held against a quadrant's hits between rounds of jobs, so the pairs meet it at four jobs a round
(primary_chunk 4: the jobs of the triangle with the lower bound run first, the other's are then held against them).

CPU tests (unmarked): conditions on the oracle that let the GPU tests fail.  GPU tests: ids, t bits, normals and
directions equal to the oracle's primary pass on O.grid_perspective: the full frame and a row band, z-slabs 2 and 4, the
wide list, the gather path without triangle records, the primary launch-shape options; the work counters of a counting
context show that the culls ran and that the depth bound dropped jobs.

Oracle figures                                   near (= wide)      far            band (rows 1 .. 5)
  triangles / screen-grid references             3 136 / 4 904      3 136 / 7 876  1 110 / 1 338    (wide: 3 142 / 5 672)
  longest list / hit pixels                      48 / 6 571 of 8 192  136 / 8 192  46 / 2 541 of 2 880
  edge and vertex rays, not moved, that hit their triangle / do not
    tile corners                                 149 / 160          22 / 290       32 / 60
    quadrant corners                             142 / 161          22 / 280       39 / 47
    other pixels                                 624 / 616          94 / 1 138     156 / 184
  ... with their triangle as the expected id: these four cases 2 195, narrow 3 906
  chosen pixels that flip when every small triangle moves by 1e-6 / 1e-5:  near 805 / 806 of 1 852, far 1 / 10 of 1 846
  depth pairs, near, pixels of their tiles won by the first / the second of the list
    gap 0     closer one second 94 / 40 (3 pairs), closer one first 23 / 66 (2 pairs)
    gap 1e-7  66 / 68 and 80 / 3;   gap 1e-6  0 / 124 and 94 / 0;   gap 1e-5  0 / 136 and 87 / 0
    gap 1e-4  0 / 102 and 91 / 0;   gap 1e-2  0 / 94 and 87 / 0;    gap 0.3   0 / 89 and 97 / 0
    (band: one pair per gap and order in its rows, the same pattern; far: what float32 leaves of the nearest small
    triangles covers most of the picture, the pairs win 0 to 52 pixels a gap)
Measured on an MI355X: the 15 GPU tests of this file take 2.5 s together (the slowest 0.2 s).  Work counters of the
counting context: wide 5 672 references, 5 166 survive the tile cull, 9 786 jobs, 730 dropped by the depth bound; far
7 876, 6 369, 20 121, 2 805.
  narrow: 13 312 triangles, 26 795 references, longest list 32; edge and vertex rays that hit / do not: tile corners
    642 / 550, quadrant corners 644 / 606, others 2 620 / 2 389; pairs, pixels won by the first / the second: gap 0
    5 637 / 2 541 (closer one second) and 6 096 / 2 060, gap 1e-7 2 518 / 5 648 and 7 710 / 459
A build with K = 0, the boxes not widened (1.0001, + 1e-6) and d_cull_tlow's factor 1 fails
test_pairs_in_a_narrow_field by 394 pixels of the pairs' tiles at primary_chunk 4 and by 16 at primary_chunk 4 with
primary_order 0 (none at the default chunk or at 64: all jobs of a tile then run in one round), and
test_frame_equals_the_oracle[narrow] by 112 chosen pixels.  On the 45-degree cases it fails 8 tests, each by ONE
pixel, a chosen one: test_frame_equals_the_oracle[near], [wide], test_row_band_of_the_main_frame, test_z_slabs[near-2],
[near-4], test_launch_shapes_change_no_pixel[near], [wide], test_the_culls_ran[wide]; far and band pass.  Of the suite as it
was before this file, 603 GPU tests, that build fails none for the primary pass (3 for the bounce, 5 for the shadow
pass); the record of this file's main frame (tests/test_reference_kernels.py, cullsyn_128x64) sees the same pixel.
On the 45-degree cases no depth-pair pixel fails on that build: there the least t over a tile lies below the greatest
over one of its quadrants by 1e-3 at least, so the bound's margins never decide; their pairs check that the closer one
wins in either list order, ties included, and the gaps of 1e-2 and 0.3 and the backdrop of "wide" are what the bound
drops.  The narrow case is where the margins decide.
"""
import functools
import types

import numpy as np
import pytest

FOVY = 45.0
EYE = np.array([0.3, 0.2, -0.1])
LOOK = np.array([0.2, 0.1, 1.0])
FAR_OFFSET = 1e5 * np.array([1.0, -0.7, 0.4]) / np.linalg.norm([1.0, -0.7, 0.4])
CASES = {"near": (128, 64, None, False, False), "far": (128, 64, None, True, False), "band": (72, 40, (1, 5), False, False),
         "wide": (128, 64, None, False, True), "narrow": (512, 256, None, False, False)}  # W, H, rows, far eye, view-filling triangles
SEEDS = {"band": 0, "far": 1, "near": 2, "wide": 2, "narrow": 5}
# "narrow": a field of view of 0.05 degrees from the coordinate origin along +z, pairs 0 and 1e-7 apart (the docstring)
NARROW_FOVY = 0.05
NARROW_GAPS = (0.0, 1e-7)
CORNER_LANES, QUADRANT_LANES = (0, 7, 56, 63), (27, 28, 35, 36)
RANDOM_PER_TILE = 16
GAPS = (0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-2, 0.3)  # (the last two: far enough apart for the bound to drop the farther one)
MOVES = (1e-6, 1e-5)


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def aspect_of(W, H):
    return float(np.float32(W) / np.float32(H))


def camera_params(far, narrow=False):
    if narrow:
        return dict(eye=(0.0, 0.0, 0.0), look=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), near=0.1, far=5000.0)
    eye = EYE + (FAR_OFFSET if far else 0.0)
    eye = np.float32(eye).astype(np.float64)
    return dict(eye=tuple(eye), look=tuple(eye + LOOK), up=(0.0, 1.0, 0.0), near=0.1, far=5000.0)


def camera(O, W, H, far, narrow=False):
    return O.cam_from(camera_params(far, narrow), NARROW_FOVY if narrow else FOVY, aspect_of(W, H))


def perp(rng, d):
    """Two unit vectors per direction d [n, 3]: e at random across d, f = d x e."""
    r = rng.normal(size=d.shape)
    e = unit(r - (r * d).sum(1, keepdims=True) * d)
    return e, np.cross(d, e)


@functools.lru_cache(maxsize=None)
def pixel_rays(O, W, H, far, narrow=False):
    """(camera, eye as the tracer has it, each pixel's float32 direction [N, 3]): the directions do not depend on the scene."""
    cam = camera(O, W, H, far, narrow)
    eye = cam.worldori[:3].astype(np.float64)
    v = np.float32(eye + np.array([[0, 0, 5.0], [1, 0, 5.0], [0, 1, 5.0]]))
    f = np.arange(3, dtype=np.int32).reshape(1, 3)
    out = O.trace_primary(cam, W, H, O.grid_perspective(cam.cc, f, v, W // 8, H // 8), v, f)
    d = out["dir"].reshape(-1, 3).astype(np.float64)
    assert np.isfinite(d).all() and (np.abs(np.linalg.norm(d, axis=1) - 1.0) < 1e-6).all()
    return cam, eye, d


@functools.lru_cache(maxsize=None)
def scene(O, case, move_all=0.0):
    """The triangles of a case; move_all: every small triangle moved off its ray by that share of its distance.
    (tests/golden/ref_kernels_cullsyn_128x64.npz records case "near": a change here that moves a vertex of it needs the
    record written again, tests/golden/make_ref_kernels.py.)"""
    W, H, rows, far, wide = CASES[case]
    narrow = case == "narrow"
    cam, eye, dirs = pixel_rays(O, W, H, far, narrow)
    rng = np.random.default_rng([20261022, SEEDS[case]])
    nbx, nby = W // 8, H // 8
    pix = float(np.median(np.linalg.norm(dirs[1:] - dirs[:-1], axis=1)))  # a pixel's width at distance 1
    # -- the chosen pixels
    lanes = []
    for tile in range(nbx * nby):
        rest = np.setdiff1d(np.arange(64), CORNER_LANES + QUADRANT_LANES)
        lanes.append(np.concatenate([CORNER_LANES, QUADRANT_LANES, rng.choice(rest, RANDOM_PER_TILE, replace=False)]))
    lanes = np.asarray(lanes)
    tile = np.repeat(np.arange(nbx * nby), lanes.shape[1])
    lane = lanes.reshape(-1)
    col, row = (tile % nbx) * 8 + lane % 8, (tile // nbx) * 8 + lane // 8
    p = row * W + col
    n = p.size
    where = np.where(np.isin(lane, CORNER_LANES), 0, np.where(np.isin(lane, QUADRANT_LANES), 1, 2))
    # -- a small triangle under each
    d = dirs[p]
    t = np.exp(rng.uniform(np.log(1.0), np.log(100.0), n))
    Q = eye + t[:, None] * d
    e, f = perp(rng, d)
    e, f = e + rng.uniform(-1, 1, (n, 1)) * d, f + rng.uniform(-1, 1, (n, 1)) * d  # tilted against the ray
    s = (np.exp(rng.uniform(np.log(0.3), np.log(3.0), n)) * t * pix)[:, None]
    vertex = rng.random(n) < 0.3
    a = np.where(vertex, 0.0, rng.uniform(0.1, 0.9, n))[:, None]
    A, B = Q - a * s * e, Q + (1.0 - a) * s * e
    Cc = Q + rng.uniform(0.3, 1.0, (n, 1)) * s * f * rng.choice([-1.0, 1.0], (n, 1)) + rng.uniform(-0.5, 0.5, (n, 1)) * s * e
    tri = np.stack([A, B, Cc], 1)
    roll = rng.integers(0, 3, n)  # which edge or vertex of the triangle, and (by the side of Cc) which winding
    tri = tri[np.arange(n)[:, None], (np.arange(3)[None, :] + roll[:, None]) % 3]
    move = rng.choice(np.array([0.0, MOVES[0], MOVES[1]]), n, p=[0.6, 0.2, 0.2])
    off = unit(e * rng.normal(size=(n, 1)) + f * rng.normal(size=(n, 1)))
    tri = tri + (np.where(move_all > 0, move_all, move) * t)[:, None, None] * off[:, None, :]
    small = tri
    # -- depth pairs on every other tile
    tx, ty = np.meshgrid(np.arange(nbx), np.arange(nby), indexing="xy")
    ptile = np.flatnonzero(((tx % 2 == 0) & (ty % 2 == 0)).reshape(-1))
    m = ptile.size
    gaps = NARROW_GAPS if narrow else GAPS
    gap = np.asarray(gaps)[np.arange(m) % len(gaps)]
    reverse = (np.arange(m) // len(gaps)) % 2 == 1
    if narrow:  # small triangles on the tiles of odd column and odd row only: the pairs' tiles hold next to nothing else
        keep = ((tile % nbx) % 2 == 1) & ((tile // nbx) % 2 == 1)
        small, p, where, vertex, move, t = small[keep], p[keep], where[keep], vertex[keep], move[keep], t[keep]
        n = int(keep.sum())
    px = ((ptile // nbx) * 8)[:, None, None] * W + (np.arange(8) * W)[None, :, None] + ((ptile % nbx) * 8)[:, None, None] + np.arange(8)[None, None, :]
    px = px.reshape(m, 64)
    dc = unit(dirs[px].mean(1))
    T = rng.uniform(513.0, 560.0, m) if narrow else rng.uniform(300.0, 600.0, m)  # (narrow: where an ulp of t is largest)
    Cn = eye + T[:, None] * dc
    pe, pf = perp(rng, dc)
    h = 5.2 * pix * T  # the tile's rays lie within 3.5 * sqrt(2) = 4.95 pixel widths of its middle
    tilt = rng.uniform(-0.5, 0.5, m) * (0.0 if narrow else 1.0)  # (narrow: the plane faces the eye)
    th0 = rng.uniform(0, 2 * np.pi, m)

    def covering(th0, R):
        th = th0[:, None] + np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
        inpl = R[:, None, None] * (np.cos(th)[:, :, None] * pe[:, None, :] + np.sin(th)[:, :, None] * pf[:, None, :])
        along = tilt[:, None] * (inpl * pe[:, None, :]).sum(2)
        return Cn[:, None, :] + inpl + along[:, :, None] * dc[:, None, :]

    first = covering(th0, 2.0 * h)
    second = eye + (1.0 - gap)[:, None, None] * (covering(th0 + np.pi / 3.0, 2.3 * h) - eye)
    flip = rng.random(m) < 0.5  # (either winding)
    first[flip] = first[flip][:, ::-1]
    second[~flip] = second[~flip][:, ::-1]
    pairs = np.where(reverse[:, None, None, None], np.stack([second, first], 1), np.stack([first, second], 1)).reshape(-1, 3, 3)
    parts = [small, pairs]
    if wide:
        c = eye + 2000.0 * unit(LOOK)
        we, wf = perp(rng, np.repeat(unit(LOOK)[None, :], 6, 0))
        th = rng.uniform(0, 2 * np.pi, 6)[:, None] + np.array([0.0, 2.0, 4.0]) * np.pi / 3.0
        parts.append(c + 9000.0 * (np.cos(th)[:, :, None] * we[:, None, :] + np.sin(th)[:, :, None] * wf[:, None, :])
                     + rng.uniform(-200, 200, (6, 3, 1)) * unit(LOOK))
    verts = np.ascontiguousarray(np.concatenate(parts).reshape(-1, 3), np.float32)
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    return types.SimpleNamespace(case=case, W=W, H=H, N=W * H, rows=rows, cam=cam, verts=verts, faces=faces, F=len(faces),
                                 p=p, k=np.arange(n), where=where, vertex=vertex, move=np.where(move_all > 0, move_all, move),
                                 t=t, nsmall=n, ptile=ptile, ppx=px, pfirst=n + 2 * np.arange(m), gap=gap, reverse=reverse,
                                 nwide=6 if wide else 0)


@functools.lru_cache(maxsize=None)
def want(O, case, slabs=1, rows="case", move_all=0.0):
    S = scene(O, case, move_all)
    rows = S.rows if rows == "case" else rows
    g = O.grid_perspective(S.cam.cc, S.faces, S.verts, S.W // 8, S.H // 8, rows, slabs=slabs)
    out = O.trace_primary(S.cam, S.W, S.H, g, S.verts, S.faces, rows, slabs=slabs)
    out["grid"] = g
    return out


def in_band(S, rows, p):
    lo, hi = rows if rows is not None else (0, S.H // 8)
    return (p >= lo * 8 * S.W) & (p < hi * 8 * S.W)


# ------------------------------------------------------------------------------------------------ CPU: the inputs

def test_edge_rays_can_fail(O):
    """By the oracle, among the rays with an edge or a vertex of their triangle on them (not moved): at least a quarter
    hit it and at least a quarter do not, in every case and at each of the three places in the tile; at least 1000 have
    it as the expected id."""
    total = 0
    for case in sorted(CASES):
        S, w = scene(O, case), want(O, case)
        ids = w["id"][S.p]
        sharp = (S.move == 0) & in_band(S, S.rows, S.p)
        hit = ids == S.k
        total += (hit & sharp).sum()
        for place, name in enumerate(("tile corners", "quadrant corners", "other pixels")):
            sel = sharp & (S.where == place)
            print("%s, %s: %d edge and vertex rays, %d hit their triangle, %d do not (vertex rays: %d of %d hit)" % (
                case, name, sel.sum(), (hit & sel).sum(), (~hit & sel).sum(), (hit & sel & S.vertex).sum(), (sel & S.vertex).sum()))
            if case != "far":  # (far: float32 leaves of the nearest triangles what it can; the counts are recorded)
                assert (hit & sel).sum() >= 0.25 * sel.sum() and (~hit & sel).sum() >= 0.25 * sel.sum()
        print("%s: %d triangles, R %d, longest list %d, hit pixels %d of %d" % (
            case, S.F, w["grid"]["R"], w["grid"]["span"].max(), (w["id"] >= 0).sum(), S.N))
    print("edge and vertex rays that end on their triangle: %d" % total)
    assert total >= 1000


@pytest.mark.parametrize("case", ["near", "far"])
def test_moved_triangles_change_the_hits(O, case):
    """The exact test decides the chosen rays at the scale of the culls' margins: with every small triangle moved off its
    ray by 1e-6 and by 1e-5 of its distance, a counted share of the chosen pixels changes between hitting and missing
    its triangle."""
    S = scene(O, case)
    base = want(O, case)["id"][S.p] == S.k
    sharp = S.move == 0
    for rel in MOVES:
        moved = want(O, case, move_all=rel)["id"][S.p] == S.k
        print("%s: triangles moved by %g: %d of %d chosen pixels flip" % (case, rel, ((moved != base) & sharp).sum(), sharp.sum()))
        if case == "near":
            # a ray on the edge to within the rounding of a vertex (6e-8 of the distance) is put to either side by a move
            # 16 or 160 times that: about half of them flip
            assert ((moved != base) & sharp).sum() >= 0.2 * sharp.sum()


def pair_winners(S, ids):
    """Per depth pair: (pixels of its tile won by the first in list order, by the second)."""
    own = ids[S.ppx]
    return (own == S.pfirst[:, None]).sum(1), (own == S.pfirst[:, None] + 1).sum(1)


@pytest.mark.parametrize("case", ["near", "far", "band", "narrow"])
def test_depth_pairs_can_fail(O, case):
    """Both outcomes (the first of the list wins, the second wins) occur at every gap, except where geometry forbids
    one: from 1e-6 on the closer triangle wins, so both occur once both list orders are there.  At gap 0 (one plane,
    other vertices) and 1e-7 the rounding of T and det decides, a tie stays with the first, and both occur too."""
    S = scene(O, case)
    first, second = pair_winners(S, want(O, case)["id"])
    inb = in_band(S, S.rows, S.ppx[:, 0])
    for g in (NARROW_GAPS if case == "narrow" else GAPS):
        orders = 0
        for rev in (False, True):
            sel = inb & (S.gap == g) & (S.reverse == rev)
            print("%s: gap %g, closer one %s in the list: %d pairs, pixels won by the first %d, by the second %d" % (
                case, g, "first" if rev else "second", sel.sum(), first[sel].sum(), second[sel].sum()))
            if sel.sum() == 0:
                assert case == "band"  # (ten pairs in its rows)
                continue
            orders += 1
            # (the small triangles, 24 to a tile, cover less than three quarters of it)
            if case != "far":  # (far: what float32 leaves of the nearest small triangles covers most of the picture)
                assert (first + second)[sel].min() >= 16
            # geometry: the closer one wins every pixel of the tile that no small triangle covers (far: the vertices'
            # rounding, 0.008 at a distance of 450, is a relative 2e-5)
            if g >= (1e-2 if case == "far" else 1e-6):
                assert (first if not rev else second)[sel].sum() == 0
        # (far is left out: what float32 leaves of its nearest small triangles hides most of the pairs)
        if case != "far" and (g < 1e-6 or orders == 2):
            sel = inb & (S.gap == g)
            assert first[sel].sum() > 0 and second[sel].sum() > 0, g


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Primary:
    """A context with a case's camera and triangles uploaded and its screen grid built."""

    def __init__(self, ugrt, torch, S, rows=None, slabs=1, flags=0):
        self.S, self.torch = S, torch
        self.ctx = ctx = ugrt.Context(S.W, S.H, light_grid=(16, 16), rows=rows, slabs=slabs, flags=flags)
        ctx.upload_camera(S.cam.cc)
        self.dv, self.df = ctx.upload(S.verts.reshape(-1)), ctx.upload(S.faces.reshape(-1))
        ctx.grid_build_perspective(self.df, self.dv, S.F)

    def trace(self, lists=None, dv=None, df=None):
        ctx, torch, N = self.ctx, self.torch, self.S.N
        out = dict(normal=torch.full((3 * N,), 7.0, device=ctx.device), t=torch.full((N,), 7.0, device=ctx.device),
                   dir=torch.full((3 * N,), 7.0, device=ctx.device),
                   shadowed=torch.full((N,), 7, dtype=torch.int32, device=ctx.device),
                   id=torch.full((N,), 7, dtype=torch.int32, device=ctx.device))
        value, span, offset = lists if lists is not None else (None, None, None)
        ctx.trace_primary(value, span, offset, out["normal"], out["t"], out["dir"], out["shadowed"], out["id"],
                          self.dv if dv is None else dv, self.df if df is None else df)
        ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


def assert_primary_equal(S, got, w, rows, what):
    a, b = (0, S.N) if rows is None else (rows[0] * 8 * S.W, rows[1] * 8 * S.W)
    bad = np.flatnonzero((got["id"][a:b] != w["id"][a:b]) | (bits(got["t"][a:b]) != bits(w["t"][a:b]))) + a
    chosen = np.isin(bad, S.p).sum()
    assert bad.size == 0, "%s: %d pixels differ (%d of them chosen pixels), first %d: id %d t %r, oracle id %d t %r" % (
        what, bad.size, chosen, bad[0], got["id"][bad[0]], got["t"][bad[0]], w["id"][bad[0]], w["t"][bad[0]])
    for name in ("normal", "dir"):
        np.testing.assert_array_equal(bits(got[name][3 * a:3 * b]), bits(w[name][3 * a:3 * b]), err_msg="%s: %s" % (what, name))
    assert (got["shadowed"][a:b] == w["shadowed"][a:b]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_equals_the_oracle(ugrt, O, torch, case):
    """Through the context's own grid (triangle records, the wide list where there is one), twice; through the merged
    lists; and with vertex and face arrays that are not the built ones (the gather path)."""
    S, w = scene(O, case), want(O, case)
    s = Primary(ugrt, torch, S, rows=S.rows)
    for rep in range(2):
        assert_primary_equal(S, s.trace(), w, S.rows, "%s, own grid, call %d" % (case, rep))
    value, key, span, offset, gi = s.ctx.grid_arrays(ugrt.GRID_PERSPECTIVE)
    assert gi.total_refs == w["grid"]["R"]
    np.testing.assert_array_equal(value.cpu().numpy().view(np.uint32), w["grid"]["vals"])
    assert_primary_equal(S, s.trace(lists=(value, span, offset)), w, S.rows, case + ", merged lists")
    assert_primary_equal(S, s.trace(dv=s.dv.clone(), df=s.df.clone()), w, S.rows, case + ", gathered, own grid")
    assert_primary_equal(S, s.trace(lists=(value, span, offset), dv=s.dv.clone(), df=s.df.clone()), w, S.rows,
                         case + ", gathered, merged lists")


@pytest.mark.gpu
def test_row_band_of_the_main_frame(ugrt, O, torch):
    S, rows = scene(O, "near"), (2, 6)
    w = want(O, "near", rows=rows)
    s = Primary(ugrt, torch, S, rows=rows)
    got = s.trace()
    assert_primary_equal(S, got, w, rows, "band")
    assert (got["id"][:rows[0] * 8 * S.W] == 7).all() and (got["id"][rows[1] * 8 * S.W:] == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("slabs", [2, 4])
@pytest.mark.parametrize("case", ["near", "far"])
def test_z_slabs(ugrt, O, torch, case, slabs):
    S, w = scene(O, case), want(O, case, slabs=slabs)
    s = Primary(ugrt, torch, S, slabs=slabs)
    assert_primary_equal(S, s.trace(), w, None, "%s, %d slabs" % (case, slabs))


@pytest.mark.gpu
def test_pairs_in_a_narrow_field(ugrt, O, torch):
    """Case "narrow": the depth bound is as tight as the rays' own t.  With four jobs a round (primary_chunk 4) the four
    quadrants' jobs of the triangle with the lower bound run first and the other triangle's are then held against what
    they found; in list order (primary_order 0) each round holds both triangles of one quadrant pair."""
    S, w = scene(O, "narrow"), want(O, "narrow")
    first, second = pair_winners(S, w["id"])
    assert (first + second).min() >= 48  # (small triangles of a diagonal neighbour reach a few corner pixels here and there)
    s = Primary(ugrt, torch, S)
    wrong = []
    for opts in ((), (("primary_chunk", 4),), (("primary_chunk", 4), ("primary_order", 0)), (("primary_chunk", 64),),
                 (("primary_order", 0),)):
        for key, value in opts:
            s.ctx.set_option(key, value)
        try:
            got = s.trace()
        finally:
            for key, _ in opts:
                s.ctx.set_option(key, -1)
        # the pairs' tiles alone (test_frame_equals_the_oracle[narrow] holds the whole picture), every option before the verdict
        px = S.ppx.reshape(-1)
        bad = (got["id"][px] != w["id"][px]) | (bits(got["t"][px]) != bits(w["t"][px]))
        print("narrow %r: pixels of the pairs' tiles that differ from the oracle: %d" % (opts, bad.sum()))
        wrong.append((opts, int(bad.sum())))
    assert all(n == 0 for _, n in wrong), wrong


PRIMARY_SHAPES = [("primary_centre", 0), ("primary_waves", 64), ("primary_waves", 4096), ("primary_xcd_run", 0),
                  ("primary_xcd_run", 1), ("primary_xcd_run", 7), ("primary_xcd_run", 4096), ("primary_order", 0),
                  ("primary_chunk", 4), ("primary_chunk", 64), ("primary_seg", 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["near", "wide"])
def test_launch_shapes_change_no_pixel(ugrt, O, torch, case):
    """The primary options that test_launch_shape_options_do_not_change_a_result walks, each alone, then the defaults."""
    S, w = scene(O, case), want(O, case)
    s = Primary(ugrt, torch, S)
    for key, value in PRIMARY_SHAPES:
        s.ctx.set_option(key, value)
        try:
            assert_primary_equal(S, s.trace(), w, None, "%s, %s=%d" % (case, key, value))
        finally:
            s.ctx.set_option(key, -1)
    assert_primary_equal(S, s.trace(), w, None, case + ", defaults again")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["wide", "far"])
def test_the_culls_ran(ugrt, O, torch, case):
    """A counting context: the tile and quadrant culls dropped references, the depth bound dropped jobs before their
    exact tests, and the picture is the oracle's."""
    S, w = scene(O, case), want(O, case)
    s = Primary(ugrt, torch, S, flags=ugrt.FLAG_COUNT_WORK)
    assert_primary_equal(S, s.trace(), w, None, case + ", counting")
    st = s.ctx.stats_primary()
    print(case, st)
    assert st["references"] >= w["grid"]["R"] > 0
    assert 0 < st["tile_survivors"] < st["references"]
    assert 0 < st["quadrant_survivors"] < 4 * st["tile_survivors"]
    assert st["jobs"] > 0 and st["rounds"] > 0 and st["hits"] > 0
    assert st["jobs_dropped_by_the_depth_bound"] > 0
