"""Split cells of the primary pass: the last segment wave to arrive finishes the tile (k_trace_primary).

A cell with more than primary_seg references is cut into work items that run on different waves.  The scan that writes
the work list writes the cell's number of segments into the context's per-cell counter.  Each wave merges its hits into
the context's per-pixel slots with a 64-bit atomicMin, then takes 1 off the counter; the wave whose subtraction returns
1 takes the merged words (an exchange against all ones, which re-arms the slot) and finishes the 64 pixels; the counter
is then 0 again.  There is no resolve launch.  What can go wrong: a wrong segment count (the tile is finished early,
twice or never), slots or counters that are not left re-armed (the NEXT frame is wrong), a band whose first pixel is
not pixel 0, lists whose tie-break is a position instead of an id.

Frame: 64 x 64 pixels = 8 x 8 cells, primary_seg 64 (the minimum), triangles placed with numpy (float64, rounded once,
seeded) under the oracle's own pixel directions, each inside the middle of one cell so that the cell's count is exact:
  cell (1,2) 63 references (not split), (2,2) 64 (exactly one item), (3,2) 65 and (2,3) 129 (the last item holds one
  triangle), (1,3) 128, (4,4) 5 * 64 + 3 = 323 (many items; 60 of its triangles are copies of others, so equal t bits
  meet across items and the first of the list must win), (5,3) 200 triangles a tenth of a pixel small BETWEEN the rays:
  a split cell none of whose pixels is hit, (3,0) 150 and (6,7) 70 outside the band of the band cases, every other
  cell empty.  With n wide triangles (backdrops larger than the view, scattered through the id range) every cell holds
  n more, and the narrow counts are n less, so the totals stay what they are.
Everything is compared with the oracle (O.grid_perspective, O.trace_primary) on raw bits.  A last case fills a flush
to 127 staged triangles, the most the staging buffer ever holds.
Measured on an MI355X: the 42 GPU tests of this file take 2.6 s together (the slowest 0.2 s).
"""
import functools
import types

import numpy as np
import pytest

W = H = 64
NB = 8
SEG = 64
BAND = (2, 6)
CAM_A = dict(eye=(0.0, 0.0, 0.0), look=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), near=0.1, far=100.0)
CAM_B = dict(eye=(0.4, 0.3, 0.5), look=(0.1, 0.2, -1.0), up=(0.0, 1.0, 0.0), near=0.1, far=100.0)
MISS_CELL = (5, 3)
TIE_CELL = (4, 4)
COUNTS = {(1, 2): 63, (2, 2): 64, (3, 2): 65, (1, 3): 128, (2, 3): 129, TIE_CELL: 5 * 64 + 3, MISS_CELL: 200,
          (3, 0): 150, (6, 7): 70}
OUTS = ("id", "t", "normal", "dir", "shadowed")
PER_PIXEL = dict(id=1, t=1, normal=3, dir=3, shadowed=1)


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


@functools.lru_cache(maxsize=None)
def pixel_rays(O, which):
    """(camera, the eye as the tracer has it, each pixel's float32 direction [H, W, 3])."""
    cam = O.cam_from(CAM_A if which == "A" else CAM_B, 45.0, 1.0)
    eye = cam.worldori[:3].astype(np.float64)
    v = np.float32(eye + np.array([[0, 0, -5.0], [1, 0, -5.0], [0, 1, -5.0]]))
    f = np.arange(3, dtype=np.int32).reshape(1, 3)
    out = O.trace_primary(cam, W, H, O.grid_perspective(cam.cc, f, v, NB, NB), v, f)
    d = out["dir"].reshape(H, W, 3).astype(np.float64)
    assert np.isfinite(d).all()
    return cam, eye, d


def _towards(dirs, x, y):
    """Directions through the picture positions (x, y) in pixels (the ray of pixel (c, r) goes through (c, r))."""
    c, r = np.floor(x).astype(int), np.floor(y).astype(int)
    a, b = (x - c)[:, None], (y - r)[:, None]
    return (dirs[r, c] * (1 - a) * (1 - b) + dirs[r, c + 1] * a * (1 - b) + dirs[r + 1, c] * (1 - a) * b
            + dirs[r + 1, c + 1] * a * b)


def _triangles(rng, eye, dirs, x, y, size_px, dist):
    """One triangle around each picture position, no vertex further than size_px pixels from it."""
    pix = float(np.linalg.norm(dirs[32, 33] - dirs[32, 32]))
    ctr = eye + dist[:, None] * _towards(dirs, x, y)
    ex, ey = dirs[32, 33] - dirs[32, 32], dirs[33, 32] - dirs[32, 32]
    ex, ey = ex / np.linalg.norm(ex), ey / np.linalg.norm(ey)
    th = rng.uniform(0, 2 * np.pi, len(x))[:, None] + np.array([0.0, 2.0, 4.0]) * np.pi / 3 + rng.uniform(-0.4, 0.4, (len(x), 3))
    rad = (0.7 * size_px * dist * pix)[:, None]
    along = rng.uniform(-0.5, 0.5, (len(x), 3)) * rad  # tilted against the view
    return (ctr[:, None, :] + (rad * np.cos(th))[:, :, None] * ex + (rad * np.sin(th))[:, :, None] * ey
            + along[:, :, None] * dirs[32, 32])


def _wide(rng, n):
    """n backdrops larger than the view of either camera, 60 to 70 away."""
    tri = []
    for k in range(n):
        j = rng.uniform(0.8, 1.2, 6)
        d = 60.0 + 10.0 * k / max(n, 1)
        tri.append([[-900 * j[0], -900 * j[1], -d], [900 * j[2], -900 * j[3], -d], [40 * j[4], 900 * j[5], -d]])
    return np.array(tri, np.float64).reshape(-1, 3, 3)


@functools.lru_cache(maxsize=None)
def scene(O, n_wide):
    cam, eye, dirs = pixel_rays(O, "A")
    rng = np.random.default_rng([20261020, n_wide])
    tris = []
    for (cx, cy), total in sorted(COUNTS.items()):
        n = total - n_wide
        if (cx, cy) == MISS_CELL:  # between the rays: x and y end on .5, a tenth of a pixel small
            x = cx * 8 + rng.integers(1, 6, n) + 0.5
            y = cy * 8 + rng.integers(1, 6, n) + 0.5
            tris.append(_triangles(rng, eye, dirs, x, y, np.full(n, 0.1), rng.uniform(2.0, 50.0, n)))
            continue
        x, y = cx * 8 + rng.uniform(1.6, 5.4, n), cy * 8 + rng.uniform(1.6, 5.4, n)
        t = _triangles(rng, eye, dirs, x, y, rng.uniform(0.4, 1.5, n), np.exp(rng.uniform(np.log(2.0), np.log(50.0), n)))
        if (cx, cy) == TIE_CELL:  # copies: equal t bits in different items of the cell
            t[100:120], t[200:220], t[260:280] = t[0:20], t[0:20], t[40:60]
        tris.append(t)
    tris = np.concatenate(tris)
    tris = tris[rng.permutation(len(tris))]  # the cells' triangles interleave in the id range
    if n_wide:
        tris = np.insert(tris, np.sort(rng.integers(0, len(tris) + 1, n_wide)), _wide(rng, n_wide), axis=0)
    verts = np.ascontiguousarray(tris.reshape(-1, 3), np.float32)
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    return types.SimpleNamespace(verts=verts, faces=faces, F=len(faces), n_wide=n_wide)


@functools.lru_cache(maxsize=None)
def want(O, n_wide, which="A", rows=None, cap=False):
    """The oracle's grid and primary pass: computed once per case and left unchanged."""
    S = cap_scene(O) if cap else scene(O, n_wide)
    cam = pixel_rays(O, which)[0]
    g = O.grid_perspective(cam.cc, S.faces, S.verts, NB, NB, rows=rows)
    out = O.trace_primary(cam, W, H, g, S.verts, S.faces, rows=rows)
    out["grid"] = g
    return out


def cell_pixels(cx, cy):
    return ((cy * 8 + np.arange(8))[:, None] * W + cx * 8 + np.arange(8)[None, :]).reshape(-1)


def items_of(span, rows=None, seg=SEG):
    lo, hi = rows if rows is not None else (0, NB)
    sp = span.reshape(NB, NB)[:, lo:hi].astype(np.int64)  # cell = cx * nby + cy
    return int(np.maximum(1, (sp + seg - 1) // seg).sum()), int(sp.sum())


CAP_CELL = (3, 3)


@functools.lru_cache(maxsize=None)
def cap_scene(O):
    """One cell of 128 references in one item: the first batch of 64 leaves 63 survivors of the tile cull (number 63 of
    the list lies between the cell's last column of rays and the cell's edge: in the cell, outside the rays' box), the
    second 64, so the flush runs on 127 staged triangles, the most there can be: the staging buffer's last record."""
    cam, eye, dirs = pixel_rays(O, "A")
    rng = np.random.default_rng(20261021)
    cx, cy = CAP_CELL
    x, y = cx * 8 + rng.uniform(1.6, 5.4, 128), cy * 8 + rng.uniform(1.6, 5.4, 128)
    size = rng.uniform(0.8, 1.5, 128)
    t = _triangles(rng, eye, dirs, x, y, size, np.exp(rng.uniform(np.log(2.0), np.log(50.0), 128)))
    # number 63: one edge parallel to the last column of rays and half a pixel beyond it, the third vertex further out.
    # (The tile cull drops a triangle when one of its EDGES has the whole box of directions on its outer side; it does
    # not test the box's own sides, so a triangle of any other orientation this close to the box survives it.)
    t[63] = eye + 10.0 * _towards(dirs, cx * 8 + np.array([7.5, 7.5, 7.6]), cy * 8 + np.array([3.0, 4.0, 3.5]))
    verts = np.ascontiguousarray(t.reshape(-1, 3), np.float32)
    return types.SimpleNamespace(verts=verts, faces=np.arange(len(verts), dtype=np.int32).reshape(-1, 3), F=128, n_wide=0)


# ------------------------------------------------------------------------------------------------ CPU: the inputs

@pytest.mark.parametrize("n_wide", [0, 1, 7])
def test_the_cells_hold_what_the_cases_need(O, n_wide):
    S, w = scene(O, n_wide), want(O, n_wide)
    span = w["grid"]["span"].reshape(NB, NB)
    for cx in range(NB):
        for cy in range(NB):
            assert span[cx, cy] == COUNTS.get((cx, cy), n_wide), (cx, cy)
    assert (np.bincount(w["grid"]["vals"], minlength=S.F) == NB * NB).sum() == n_wide
    ids = w["id"]
    if n_wide == 0:
        assert (ids[cell_pixels(*MISS_CELL)] == -2).all()  # the split cell without a hit
        assert (ids[cell_pixels(0, 0)] == -2).all()
    else:
        assert (ids >= 0).all()  # the backdrops
    for cell in (c for c in COUNTS if c != MISS_CELL):
        own = ids[cell_pixels(*cell)]
        assert (own >= 0).sum() >= 8 and len(np.unique(own)) >= 5, cell
    # the band sees the same cells
    wb = want(O, n_wide, rows=BAND)
    np.testing.assert_array_equal(wb["grid"]["span"].reshape(NB, NB)[:, BAND[0]:BAND[1]], span[:, BAND[0]:BAND[1]])
    # the second camera still splits cells
    assert (want(O, n_wide, which="B")["grid"]["span"] > SEG).sum() >= 2


def test_copies_tie_across_the_items_of_a_cell(O):
    """In the cell of 323 some pixel is won by a triangle that has a copy later in the list, in another item."""
    S, w = scene(O, 0), want(O, 0)
    cell = TIE_CELL[0] * NB + TIE_CELL[1]
    g = w["grid"]
    refs = g["vals"][g["offset"][cell]:g["offset"][cell] + g["span"][cell]]
    tri = S.verts.reshape(-1, 3, 3)
    winners = np.unique(w["id"][cell_pixels(*TIE_CELL)])
    found = 0
    for a in winners[winners >= 0]:
        later = [k for k, b in enumerate(refs) if b != a and (tri[b] == tri[a]).all()]
        first = int(np.flatnonzero(refs == a)[0])
        assert all(b > a for b in refs[later])  # the first of the list won
        found += any(k // SEG != first // SEG for k in later)
    assert found >= 1


def test_the_cap_scene_fills_one_cell(O):
    w = want(O, 0, cap=True)
    span = w["grid"]["span"].reshape(NB, NB)
    assert span[CAP_CELL] == 128 and span.sum() == 128
    cell = CAP_CELL[0] * NB + CAP_CELL[1]
    np.testing.assert_array_equal(w["grid"]["vals"][w["grid"]["offset"][cell]:][:128], np.arange(128))
    assert 63 not in w["id"]


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


class Primary:
    """A context with a scene uploaded; build(camera) makes its screen grid, trace() the primary pass."""

    def __init__(self, ugrt, torch, S, rows=None, flags=0, options=(("primary_seg", SEG),)):
        self.ugrt, self.torch, self.S = ugrt, torch, S
        self.ctx = ctx = ugrt.Context(W, H, light_grid=(16, 16), rows=rows, flags=flags)
        for k, v in options:
            ctx.set_option(k, v)
        self.dv, self.df = ctx.upload(S.verts.reshape(-1)), ctx.upload(S.faces.reshape(-1))
        self.gv, self.gf = self.dv.clone(), self.df.clone()  # not the built arrays: no triangle records, the gather path

    def build(self, cam):
        self.ctx.upload_camera(cam.cc)
        self.ctx.grid_build_perspective(self.df, self.dv, self.S.F)

    def trace(self, lists=False, gather=False):
        ctx, torch, N = self.ctx, self.torch, W * H
        out = dict(normal=torch.full((3 * N,), 7.0, device=ctx.device), t=torch.full((N,), 7.0, device=ctx.device),
                   dir=torch.full((3 * N,), 7.0, device=ctx.device),
                   shadowed=torch.full((N,), 7, dtype=torch.int32, device=ctx.device),
                   id=torch.full((N,), 7, dtype=torch.int32, device=ctx.device))
        value = span = offset = None
        if lists:
            value, _, span, offset, _ = ctx.grid_arrays(self.ugrt.GRID_PERSPECTIVE)
        ctx.trace_primary(value, span, offset, out["normal"], out["t"], out["dir"], out["shadowed"], out["id"],
                          self.gv if gather else self.dv, self.gf if gather else self.df)
        ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def armed(self):
        return self.ctx.get_state("primary_slots_unarmed") == 0


def assert_equal(got, w, rows, what):
    a, b = (0, W * H) if rows is None else (rows[0] * 8 * W, rows[1] * 8 * W)
    for n in OUTS:
        k = PER_PIXEL[n]
        g, x = bits(got[n]).reshape(-1, k), bits(w[n]).reshape(-1, k)
        bad = np.flatnonzero((g[a:b] != x[a:b]).any(1)) + a
        assert bad.size == 0, "%s: %s differs at %d pixels, first %d (cell %d,%d): %r, oracle %r" % (
            what, n, bad.size, bad[0], (bad[0] % W) // 8, (bad[0] // W) // 8, got[n].reshape(-1, k)[bad[0]], w[n].reshape(-1, k)[bad[0]])
        # what lies outside the band is not written
        seven = bits(np.full(1, 7, got[n].dtype))[0]
        assert (g[:a] == seven).all() and (g[b:] == seven).all(), what + ": written outside the band"


@pytest.mark.gpu
@pytest.mark.parametrize("async_build", [0, 1])
@pytest.mark.parametrize("rows", [None, BAND])
@pytest.mark.parametrize("n_wide", [0, 1, 7])
def test_every_route_equals_the_oracle(ugrt, O, torch, n_wide, rows, async_build):
    """The context's own grid (the wide list where there are wide triangles) with and without triangle records, then
    the merged lists a caller hands in, then the own grid again; twice (an asynchronous context's second build does not
    wait).  After every trace the slots and counters are re-armed."""
    S, w = scene(O, n_wide), want(O, n_wide, rows=rows)
    cam = pixel_rays(O, "A")[0]
    s = Primary(ugrt, torch, S, rows=rows, options=(("primary_seg", SEG), ("async_build", async_build)))
    for rep in range(3 if async_build else 2):
        s.build(cam)
        assert s.ctx.get_state("primary_merge_pending") == (1 if n_wide else 0)
        for lists, gather in ((False, False), (False, True), (True, False), (True, True), (False, False)):
            what = "wide %d, rows %r, async %d, build %d, lists %d, gather %d" % (n_wide, rows, async_build, rep, lists, gather)
            assert_equal(s.trace(lists=lists, gather=gather), w, rows, what)
            assert s.armed(), what
    assert s.ctx.stats()[0] >= items_of(w["grid"]["span"], rows)[0]  # the work list was sized for items of 64


@pytest.mark.gpu
@pytest.mark.parametrize("option", [("primary_waves", 64), ("primary_waves", 4096), ("primary_centre", 0), ("primary_centre", 1),
                                    ("primary_xcd_run", 0), ("primary_xcd_run", 1), ("primary_order", 0), ("primary_chunk", 4)])
@pytest.mark.parametrize("n_wide", [0, 7])
def test_launch_forms(ugrt, O, torch, n_wide, option):
    """Persistent waves (64: fewer waves than items, every wave takes several, the finishing wave goes on to its next
    item), one wave per item from the middle outwards and in list order: the finish depends on arrival, not on order."""
    S = scene(O, n_wide)
    cam = pixel_rays(O, "A")[0]
    for rows in (None, BAND):
        w = want(O, n_wide, rows=rows)
        s = Primary(ugrt, torch, S, rows=rows, options=(("primary_seg", SEG), option))
        s.build(cam)
        for lists in (False, True):
            for rep in range(2):
                assert_equal(s.trace(lists=lists), w, rows, "wide %d, %s=%d, rows %r, lists %d, call %d" % ((n_wide,) + option + (rows, lists, rep)))
                assert s.armed()


SPLIT_INDEPENDENT = ("references", "tile_survivors", "quadrant_survivors")


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [None, BAND])
@pytest.mark.parametrize("n_wide", [0, 7])
def test_counting_kernels(ugrt, O, torch, n_wide, rows):
    """UGRT_FLAG_COUNT_WORK: the counting instantiations finish split cells the same way.  Items and references are the
    oracle's (its spans); the survivors of the tile cull do not depend on where a list is cut, so they are equal
    between primary_seg 64 and a primary_seg that splits nothing.  (Jobs, rounds and hits depend on the hits a
    segment's wave knows of, which a cut changes.)"""
    S, w = scene(O, n_wide), want(O, n_wide, rows=rows)
    cam = pixel_rays(O, "A")[0]
    st = {}
    for seg in (SEG, 1 << 20):
        s = Primary(ugrt, torch, S, rows=rows, flags=ugrt.FLAG_COUNT_WORK, options=(("primary_seg", seg),))
        s.build(cam)
        for lists in (False, True):
            for gather in (False, True):
                what = "counting, wide %d, rows %r, seg %d, lists %d, gather %d" % (n_wide, rows, seg, lists, gather)
                assert_equal(s.trace(lists=lists, gather=gather), w, rows, what)
                assert s.armed(), what
                c = s.ctx.stats_primary()
                print(what, c)
                items, refs = items_of(w["grid"]["span"], rows, seg)
                assert c["items"] == items and c["references"] == refs, what
                st.setdefault((lists, gather), {})[seg] = c
    for key, by_seg in st.items():
        for name in SPLIT_INDEPENDENT:
            assert by_seg[SEG][name] == by_seg[1 << 20][name] > 0, (key, name)
        assert by_seg[SEG]["items"] > by_seg[1 << 20]["items"]
        assert by_seg[SEG]["hits"] > 0 and by_seg[SEG]["rounds"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("rows", [None, BAND])
@pytest.mark.parametrize("n_wide", [0, 7])
def test_three_frames_on_one_context(ugrt, O, torch, n_wide, rows, lists):
    """One camera, a second one, the first again: each frame equals the oracle, and afterwards every slot is all ones
    and every counter zero; a fourth frame is the oracle's too."""
    S = scene(O, n_wide)
    s = Primary(ugrt, torch, S, rows=rows)
    assert s.armed()
    for k, which in enumerate("ABAB"):
        s.build(pixel_rays(O, which)[0])
        assert_equal(s.trace(lists=lists), want(O, n_wide, which=which, rows=rows), rows,
                     "wide %d, rows %r, lists %d, frame %d (camera %s)" % (n_wide, rows, lists, k, which))
        assert s.armed(), k


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [SEG, 1024])
def test_a_flush_of_127_staged_triangles(ugrt, O, torch, seg):
    """The most a flush can hold: 63 survivors of the first batch and 64 of the second.  primary_seg 1024: one item, one
    flush (the counters say so); primary_seg 64: the same list as two items."""
    S, w = cap_scene(O), want(O, 0, cap=True)
    cam = pixel_rays(O, "A")[0]
    s = Primary(ugrt, torch, S, flags=ugrt.FLAG_COUNT_WORK, options=(("primary_seg", seg),))
    s.build(cam)
    for gather in (False, True):
        assert_equal(s.trace(gather=gather), w, None, "cap, seg %d, gather %d" % (seg, gather))
        c = s.ctx.stats_primary()
        print(seg, gather, c)
        assert c["references"] == 128 and c["tile_survivors"] == 127
        if seg == 1024:
            assert c["items"] == NB * NB and c["flushes"] == 1 and c["quadrant_survivors"] == 127
        assert s.armed()
    t = Primary(ugrt, torch, S, options=(("primary_seg", seg),))
    t.build(cam)
    assert_equal(t.trace(), w, None, "cap, seg %d, not counting" % seg)
