"""The shadow pass by tile fragments (option "shadow_frags", the default where the ray sort is deferred).

With the ray sort put off (ugrt_sort_rays(..., NULL) under FLAG_SHADOW_ALL_CHUNKS) ShadowPass::beams() does not key and
sort every ray: the rays of an 8x8-pixel tile that share a light cell (and, since a cell is no compact patch of
directions, the top 12 bits of their direction code) are one FRAGMENT with one (cell, direction code) key; the fragments
are sorted, their ray counts scanned, and k_shadow_expand writes the pixel ids and the cells' run
bounds (ugrt_trace_shadow.hip: k_shadow_frags, FragCountLoad, k_shadow_expand).  Inside the traced set the grouping of
rays is free, so no flag may change; fragments with equal keys come out in an order that differs from run to run, and
no flag may depend on that either.  ugrt_ctx_get_state "shadow_fragments" tells how many fragments the last pass formed
(0 = it keyed every ray).

CPU tests (unmarked): a numpy restatement of the split by cell (fragments_of) on the oracle's maps: a lower bound of the
fragments the kernel forms.  It is compared with nothing on the GPU; it shows that the frames and the synthetic cases
split tiles (several cells in a tile, up to dozens) and sizes the asynchronous test's overflow.
GPU tests: flags equal to the oracle's everywhere -- the synthetic cases of test_shadow_synthetic in the deferred
all-chunks form, whole frames, hand-made maps, the forms that must keep the per-ray path, the asynchronous form.

A ray without a direction from the light (P == L, 0 / 0) moved by hand into a cell WITH a list costs other rays of its
beam their flag, with fragments and with every ray sorted alike (53 flags of case A); ugrt_map_rays_to_light never puts
one there, and the hand-made maps here leave such rays where they are (has_direction).

Oracle figures (fragments by cell of rays in cells with a list / tiles / share of tiles with >= 2 cells / most cells in a tile):
  crash(0.02) 256 x 144  (128,128) 3 806 / 576 / 100 % / 25     (64,64) 2 800 / 576 / 97 % / 16
  hall(0.1) 256 x 256    (128,128) 2 532 / 1 024 / 86 % / 8     (64,64) 1 804 / 1 024 / 59 % / 6
  hall(0.1) 136 x 64     (128,128) 1 100 / 136 / 100 % / 25
(2 626 on hall (128,128) and 1 867 at (64,64) when cells without a list count too.)
"""
import numpy as np
import pytest

import test_light_grid_sizes as LG
import test_shadow_synthetic as SS
from test_shadow_synthetic import stage, torch  # noqa: F401  (fixtures)

EOVERFLOW = 6
ALL = sorted(SS.CASES) + ["C"]
FRAMES = [("crash", (128, 128), None), ("crash", (64, 64), None), ("hall", (128, 128), None), ("hall", (64, 64), None),
          ("hall", (128, 128), (136, 64))]  # (scene, light grid, image size or the scene's own)
frame_ids = ["%s-%dx%d%s" % (n, lg[0], lg[1], "-%dx%d" % size if size else "") for n, lg, size in FRAMES]


def fragments_of(m, n, W, C, span):
    """The split by cell (k_shadow_frags splits a cell's rays further, by direction), on an unsorted map of n entries (entry i = row i // W, column i % W of the
    band): per tile the number of distinct cells among its live entries (cell < C with a list).  -> (fragments per tile)"""
    cells = m[n:2 * n].astype(np.int64)
    live = (cells < C) & (span[np.minimum(cells, C - 1)] > 0)
    i = np.arange(n)
    tile = (i // W // 8) * (W // 8) + (i % W) // 8
    per_tile = np.zeros(n // 64, np.int64)
    pairs = np.unique(tile[live] * (C + 1) + cells[live])
    np.add.at(per_tile, pairs // (C + 1), 1)
    return per_tile


def frame_size(name, size):
    return size if size else LG.IMAGES[name][1:]


# ------------------------------------------------------------------------------------------------ CPU: the inputs

@pytest.mark.parametrize("name,lg,size", FRAMES, ids=frame_ids)
def test_frames_split_their_tiles(ugrt, O, name, lg, size):
    W, H = frame_size(name, size)
    want = LG.oracle_frame(ugrt, O, name, lg, True, size)
    per_tile = fragments_of(want["map_unsorted"], W * H, W, lg[0] * lg[1], want["lgrid"]["span"])
    share = (per_tile >= 2).mean()
    print("%s %s %dx%d: %d fragments in %d tiles, %.0f %% of the tiles hold >= 2 cells, at most %d" % (
        name, lg, W, H, per_tile.sum(), per_tile.size, 100 * share, per_tile.max()))
    assert share >= 0.5 and per_tile.max() >= 6  # most tiles are split, some of them many times
    assert per_tile.sum() > per_tile.size  # more fragments than tiles
    assert want["is_shadowed"].sum() > 0


@pytest.mark.parametrize("case", ALL)
def test_synthetic_cases_split_their_tiles(O, case):
    """The synthetic rays are dealt out per pixel at random: nearly every tile holds many cells."""
    S, w = SS.synthetic(O, case), SS.want(O, case, False)
    per_tile = fragments_of(w["map_unsorted"], w["n"], S.W, S.C, SS.light_grid(O, case)["span"])
    print(case, "fragments", per_tile.sum(), "tiles", per_tile.size, "most in a tile", per_tile.max())
    assert (per_tile >= 2).mean() >= 0.9 and per_tile.max() >= 16


def has_direction(S):
    """Per ray of case A: it has a direction from the light (a ray with P == L has none: 0 / 0).  The map puts such a
    ray where no list is; the hand-made maps must not move it into a cell with one."""
    P = S.cam_pos[None, :].astype(np.float32) + S.t[:, None] * S.dirs.reshape(-1, 3)
    d = P - np.asarray(S.lcam.cc[:3], np.float32)[None, :]
    return (np.abs(d).max(axis=1) > 0) & np.isfinite(d).all(axis=1)


def tile_of(S):
    i = np.arange(S.N)
    return (i // S.W // 8) * (S.W // 8) + (i % S.W) // 8


def finite_tiles(S):
    """Tiles whose 64 rays all have a direction."""
    return np.flatnonzero(np.bincount(tile_of(S), weights=has_direction(S), minlength=S.N // 64) == 64)


def tile_entries(S, t):
    rows, cols = np.divmod(np.arange(64), 8)
    return (t // (S.W // 8) * 8 + rows) * S.W + t % (S.W // 8) * 8 + cols


def handmade_cells(O):
    """Case A's map with three tiles rewritten: the 64 rays of the first tile of finite_tiles in 64 different cells with
    lists, the tile after it wholly in the sentinel cell, the next wholly in a cell without a list.  -> (cells, first tile)"""
    S, w = SS.synthetic(O, "A"), SS.want(O, "A", False)
    span = SS.light_grid(O, "A")["span"]
    used, empty = np.flatnonzero(span > 0), np.flatnonzero(span == 0)
    assert used.size >= 64 and empty.size >= 1
    cells = w["map_unsorted"][w["n"]:].copy()
    t0 = int(finite_tiles(S)[0])
    assert t0 + 2 < S.N // 64
    for t, value in ((t0, used[:64]), (t0 + 1, S.C), (t0 + 2, empty[0])):
        cells[tile_entries(S, t)] = value
    return cells, t0


SPARSE_TILES = 8


def sparse_cells(O):
    """Case A's map with every tile but the first SPARSE_TILES wholly in the sentinel cell: at most 64 fragments a tile
    that is left, however the kernel splits a tile."""
    S, w = SS.synthetic(O, "A"), SS.want(O, "A", False)
    return np.where(tile_of(S) < SPARSE_TILES, w["map_unsorted"][w["n"]:], S.C).astype(np.uint32)


def test_handmade_maps(O):
    S, w = SS.synthetic(O, "A"), SS.want(O, "A", False)
    span = SS.light_grid(O, "A")["span"]
    m = w["map_unsorted"].copy()
    m[w["n"]:], t0 = handmade_cells(O)
    per_tile = fragments_of(m, w["n"], S.W, S.C, span)
    print("hand-made tiles from", t0, "of", finite_tiles(S).size, "tiles whose rays all have a direction")
    assert per_tile[t0] == 64 and per_tile[t0 + 1] == 0 and per_tile[t0 + 2] == 0
    # the asynchronous test: the sparse map's estimate plus a quarter (+ 1024) lies below the fragments of the case's own map
    # (a tile's rays of one cell are at least one fragment: the kernel splits them further, by direction)
    m[w["n"]:] = sparse_cells(O)
    few = fragments_of(m, w["n"], S.W, S.C, span).sum()
    many = fragments_of(w["map_unsorted"], w["n"], S.W, S.C, span).sum()
    print("sparse map", few, "fragments at least, case A", many)
    assert 0 < few <= 64 * SPARSE_TILES and many > 2 * (64 * SPARSE_TILES + 16 * SPARSE_TILES + 1024)
    # a cell with more rays than the largest beam (shadow_beam 8192)
    real = w["map_unsorted"][w["n"]:]
    assert np.bincount(real[real < S.C]).max() > 8192


# ------------------------------------------------------------------------------------------------ GPU

def run_deferred(s, options=(), cells=None, order=None, deferred=True):
    """map (entries' cells replaced / entries permuted where given), sort put off, trace: (flags, fragments)."""
    import torch as T

    try:
        for name, value in options:
            s.ctx.set_option(name, value)
        buf = s.map()
        if cells is not None or order is not None:
            m = SS.u32(buf).copy()
            if cells is not None:
                m[s.n:2 * s.n] = cells
            if order is not None:
                m[:s.n], m[s.n:2 * s.n] = m[:s.n][order], m[s.n:2 * s.n][order]
            buf.copy_(T.from_numpy(m.view(np.int32)).to(buf.device))
        prefix, count = s.sort(buf, deferred)
        flags = s.trace(buf, prefix, count).cpu().numpy()
        return flags, s.ctx.get_state("shadow_fragments")
    finally:
        for name, _ in options:
            s.ctx.set_option(name, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_synthetic_cases(ugrt, O, stage, case):
    s, w = stage(case, all_chunks=True), SS.want(O, case, False)
    by_frags, nfrag = run_deferred(s)
    assert nfrag > 0
    SS.assert_flags_equal(by_frags, w, case + " fragments")
    assert s.ctx.get_state("shadow_key_bits") == 32
    by_rays, none = run_deferred(s, (("shadow_frags", 0),))
    assert none == 0
    SS.assert_flags_equal(by_rays, w, case + " every ray")
    np.testing.assert_array_equal(by_frags, by_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("frags", [-1, 0], ids=["fragments", "every-ray"])
@pytest.mark.parametrize("name,lg,size", FRAMES, ids=frame_ids)
def test_whole_frames(ugrt, O, torch, name, lg, size, frags):
    ctx, r = LG.make(ugrt, name, lg, True, size=size, options=(("shadow_frags", frags),))
    r.display(LG.setup_of(ugrt, name), frame_cnt=1, shadows=True)
    ctx.synchronize()
    assert (ctx.get_state("shadow_fragments") > 0) == (frags != 0)
    assert ctx.get_state("shadow_key_bits") == 32
    LG.assert_pixels_equal(r, LG.oracle_frame(ugrt, O, name, lg, True, size))


@pytest.mark.gpu
def test_band(ugrt, O, stage):
    s, w = stage("A", all_chunks=True, rows=SS.BAND_ROWS), SS.want(O, "A", False, rows=SS.BAND_ROWS)
    assert s.ctx.p0 != 0
    flags, nfrag = run_deferred(s)
    assert nfrag > 0
    SS.assert_flags_equal(flags, w, "band")


@pytest.mark.gpu
def test_handmade_tiles(ugrt, O, stage):
    """64 cells in a tile, a tile in the sentinel cell, a tile in a cell without a list."""
    S, (cells, _) = SS.synthetic(O, "A"), handmade_cells(O)
    w = SS.shadow_stage(O, S, False, cells=cells)
    flags, nfrag = run_deferred(stage("A", all_chunks=True), cells=cells)
    assert nfrag > 0
    SS.assert_flags_equal(flags, w, "hand-made tiles")
    flags, nfrag = run_deferred(stage("A", all_chunks=True), (("shadow_frags", 0),), cells=cells)
    assert nfrag == 0
    SS.assert_flags_equal(flags, w, "hand-made tiles, every ray")


@pytest.mark.gpu
def test_no_fragment_at_all(ugrt, O, stage):
    """Every ray in a cell without a list, then every ray in the sentinel cell: the pass runs, forms nothing and leaves the
    incoming flags; the pass after it is right."""
    S = SS.synthetic(O, "A")
    s = stage("A", all_chunks=True)
    empty = np.flatnonzero(SS.light_grid(O, "A")["span"] == 0)[0]
    for value in (empty, S.C):
        flags, nfrag = run_deferred(s, cells=np.full(s.n, value, np.uint32))
        assert nfrag == 0
        np.testing.assert_array_equal(flags, S.flags)
    flags, nfrag = run_deferred(s)
    assert nfrag > 0
    SS.assert_flags_equal(flags, SS.want(O, "A", False), "after the empty passes")


@pytest.mark.gpu
@pytest.mark.parametrize("beam", [64, 8192])
def test_long_cell_runs(ugrt, O, stage, beam):
    """Case A's fullest cell holds 11 552 rays: more than one beam even at 8192, 181 beams at 64."""
    flags, nfrag = run_deferred(stage("A", all_chunks=True), (("shadow_beam", beam),))
    assert nfrag > 0
    SS.assert_flags_equal(flags, SS.want(O, "A", False), "shadow_beam %d" % beam)


@pytest.mark.gpu
def test_permuted_map(ugrt, O, stage):
    """The kernel reads the pixel of an entry from the map: entries in another order give less coherent fragments and
    the same flags."""
    s = stage("A", all_chunks=True)
    order = np.random.default_rng(5).permutation(s.n)
    flags, nfrag = run_deferred(s, order=order)
    assert nfrag > 0
    SS.assert_flags_equal(flags, SS.want(O, "A", False), "permuted map")


@pytest.mark.gpu
def test_forms_that_key_every_ray(ugrt, O, stage):
    every, strict = SS.want(O, "A", False), SS.want(O, "A", True)
    a = stage("A", all_chunks=True)
    for what, s, kw, w in (("waiting sort", a, dict(deferred=False), every),
                           ("strict chunks", stage("A"), {}, strict),
                           ("64-bit keys", a, dict(options=(("shadow_key64", 1),)), every),
                           ("library sort", a, dict(options=(("sort_library", 1),)), every),
                           ("shadow_frags 0", a, dict(options=(("shadow_frags", 0),)), every)):
        flags, nfrag = run_deferred(s, **kw)
        assert nfrag == 0, what
        SS.assert_flags_equal(flags, w, what)
    flags, nfrag = run_deferred(a)
    assert nfrag > 0
    SS.assert_flags_equal(flags, every, "fragments again")


@pytest.mark.gpu
def test_asynchronous_form(ugrt, O):
    """A waiting pass on a map with rays in eight tiles leaves its count as the estimate; asynchronous passes on the same
    map are sized by it.  The case's own map then forms several times the estimate plus a quarter (test_handmade_maps):
    UGRT_EOVERFLOW at the synchronisation, the repeat (which waits) is right, and so are the asynchronous passes after it."""
    S, w = SS.synthetic(O, "A"), SS.want(O, "A", False)
    cells = sparse_cells(O)
    wc = SS.shadow_stage(O, S, False, cells=cells)
    s = SS.Stage(ugrt, S, ugrt.FLAG_SHADOW_ALL_CHUNKS)
    flags, few = run_deferred(s, cells=cells)
    SS.assert_flags_equal(flags, wc, "waiting")
    assert 0 < few <= 64 * SPARSE_TILES
    s.ctx.set_option("async_build", 1)
    for rep in range(2):
        flags, nfrag = run_deferred(s, cells=cells)
        SS.assert_flags_equal(flags, wc, "asynchronous %d" % rep)
        assert nfrag == few
    with pytest.raises(ugrt.UgrtError) as e:
        run_deferred(s)
    assert e.value.code == EOVERFLOW, e.value
    flags, many = run_deferred(s)
    SS.assert_flags_equal(flags, w, "the repeat")
    assert many > few + few // 4 + 1024
    for rep in range(2):
        flags, nfrag = run_deferred(s)
        SS.assert_flags_equal(flags, w, "asynchronous after the repeat, %d" % rep)
        assert nfrag == many


@pytest.mark.gpu
def test_order_of_ties_changes_no_flag(ugrt, O, stage):
    s, w = stage("A", all_chunks=True), SS.want(O, "A", False)
    for rep in range(3):
        flags, nfrag = run_deferred(s)
        assert nfrag > 0
        SS.assert_flags_equal(flags, w, "run %d" % rep)
