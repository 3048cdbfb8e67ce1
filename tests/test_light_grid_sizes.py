"""The shadow pass at light-grid sizes up to 2^21 cells.

ugrt_ctx_create accepts any even light grid within [2,4096]^2; the other GPU tests stop at 128 x 128.  The shadow
pass changes shape with the cell count C: ShadowPass::beams() sorts its rays on (cell, direction code) keys whose
cell field holds C + 2 values, in 32 bits while that leaves 12 bits for the code (C + 2 <= 2^20) and in 64 bits
above, where other kernels and rocPRIM's sort run (k_shadow_keys<true>, ugrt_prim_sort_pairs64, k_shadow_runs<u64>).
The cell scans get more than 64 tiles (a second look-back round) from 2^18 cells, the spherical build's sort a third
radix pass from 2^17, and a large grid has more chunks than the image has tiles, so the strict launch rule
(Q12/Q13) caps what is traced.

GPU tests: one Renderer.display per case against O.frame, as test_gpu_parity.py::test_full_frame compares them
(integers equal, RGB equal), and ugrt_ctx_get_state "shadow_key_bits" says which key form ran.
CPU tests (unmarked): conditions on the oracle's frames alone, so that the cases can fail: enough distinct ray
cells, shadowed and lit rays, ray cells in the upper half of the index range, and that dropping the high bits of
the rays' cells changes the flags.

Oracle figures per case (all chunks traced): light-grid references R / distinct ray cells / chunks
  cornell B 256^2     (256,256) 247 081 / 432 / 1 301       (512,512) 977 726 / 840 / 1 530
                      (1024,512) 1 953 126 / 1 648 / 2 178  (1024,1024) 3 889 766 / 1 648 / 2 178
                      (2048,1024) 7 774 391 / 3 009 / 3 366 (4096,256) 3 934 810 / 5 387 / 5 719
                      (4096,2) 96 108 / 5 387 / 5 719       (2,4096) 32 800 / 4 / 1 027
  hall(0.1) 256^2     (512,128) 320 690 / 353 / 1 202       (512,512) 872 114 / 353 / 1 202
                      (1024,512) 1 661 976 / 701 / 1 329    (1024,1024) 3 060 248 / 701 / 1 329
                      (2048,1024) 5 962 758 / 1 394 / 1 706 (4096,256) 3 709 812 / 2 767 / 2 829
                      (4096,2) 1 045 098 / 2 767 / 2 829    (2,4096) 616 668 / 3 / 1 027
  crash(0.02) 256x144 (512,128) 743 891 / 487 / 822         (512,512) 2 230 547 / 487 / 822
                      (1024,512) 4 349 052 / 970 / 1 234    (1024,1024) 8 221 052 / 970 / 1 234
                      (4096,256) 9 448 717 / 3 777 / 3 785  (4096,2) 1 908 981 / 3 777 / 3 785
                      (2,4096) 814 654 / 3 / 579
A ray's cell row is the same for nearly every ray of these frames (the reference's getEffective_y), so the number
of distinct ray cells follows the grid's width alone; rays in every row are tests/test_shadow_synthetic.py's.  Two
consequences for the cases:
* (256,256) gives hall 178 and crash 245 distinct ray cells, below the floor of 256: those two scenes run the 2^16
  cells as (512,128) instead (the same 15-bit direction code; 353 and 487 cells).  Cornell keeps (256,256).
* (2,4096) is in the sweep BECAUSE nearly all rays share a handful of cells (long runs, many beams per cell), which
  no case with 256 distinct ray cells can be: for it the floor on distinct cells is replaced by what the case is
  for (at most 8 cells, one of them with more rays than the largest beam), every other condition holds as it is.
"""
import functools

import numpy as np
import pytest


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


# scene -> (camera, W, H): the smallest frames whose rays spread over hundreds of light cells
IMAGES = {"cornell": ("B", 256, 256), "hall": ("ref", 256, 256), "crash": ("ref", 256, 144)}


@functools.lru_cache(maxsize=None)
def scene(ugrt, name):
    return {"cornell": lambda: ugrt.scenes.cornell(), "hall": lambda: ugrt.scenes.hall(scale=0.1),
            "crash": lambda: ugrt.scenes.crash(scale=0.02)}[name]()


def setup_of(ugrt, name):
    s = scene(ugrt, name)
    return ugrt.FrameSetup(s["cameras"][IMAGES[name][0]], s["light_camera"], s["shading_light"])


@functools.lru_cache(maxsize=2)  # (a frame at 2^21 cells holds ~100 MB: the cases that share one run next to each other)
def oracle_frame(ugrt, O, name, lg, all_chunks, size=None):
    _, W, H = IMAGES[name]
    if size is not None:
        W, H = size
    return O.frame(scene(ugrt, name), setup_of(ugrt, name), W, H, light_grid=lg, all_chunks=all_chunks)


def bits_of(v):
    """Bits that hold 0 .. v - 1."""
    b = 1
    while (1 << b) < v:
        b += 1
    return b


def key_bits(lg, key64=False, mbits=None):
    """What ShadowPass::beams() sorts on: the cell field holds the cells, the sentinel cell and "not traced"; the
    direction code gets what is left of 32 bits (24 at most), or 30 bits of a 64-bit key once fewer than 12 are left."""
    cellbits = bits_of(lg[0] * lg[1] + 2)
    if key64 or cellbits > 20:
        return 30 + cellbits
    m = min(32 - cellbits, 24)
    return (min(m, mbits) if mbits else m) + cellbits


# light grid -> the key bits the issue of this sweep states for it
GRIDS = {(256, 256): 32, (512, 128): 32, (512, 512): 32, (1024, 512): 32, (1024, 1024): 51, (2048, 1024): 52,
         (4096, 256): 51, (4096, 2): 32, (2, 4096): 32}


def grids_of(name):
    out = []
    for lg in GRIDS:
        if lg == (256, 256) and name != "cornell" or lg == (512, 128) and name == "cornell":
            continue  # 2^16 cells: (512,128) where (256,256) has fewer than 256 distinct ray cells (module docstring)
        if lg == (2048, 1024) and name == "crash":
            continue  # about 16 M references
        out.append(lg)
    return out


SWEEP = [(name, lg) for name in IMAGES for lg in grids_of(name)]
ids_of = lambda cases: ["-".join(str(x) if not isinstance(x, tuple) else "%dx%d" % x for x in c) for c in cases]


def ray_cells(want, lg, n):
    """Of the rays in real cells: the distinct cells, the rays per cell, and the rays' flags."""
    C = lg[0] * lg[1]
    pix, cells = want["map"][:n], want["map"][n:].astype(np.int64)
    real = cells < C
    u, cnt = np.unique(cells[real], return_counts=True)
    return u, cnt, want["is_shadowed"][pix[real]]


# ------------------------------------------------------------------------------------------------ CPU: the inputs

def test_the_stated_key_bits_follow_from_the_cell_counts():
    for lg, want in GRIDS.items():
        assert key_bits(lg) == want, lg
    assert key_bits((128, 128)) == 32 and key_bits((128, 128), key64=True) == 45
    assert key_bits((256, 256), key64=True) == 47 and key_bits((1024, 512), mbits=9) == 29
    # the last 32-bit layout and the first 64-bit one
    assert bits_of(1024 * 512 + 2) == 20 and bits_of(1024 * 1024 + 2) == 21


@pytest.mark.parametrize("name,lg", SWEEP, ids=ids_of(SWEEP))
def test_swept_case_can_fail(ugrt, O, name, lg):
    """Conditions on the oracle's frame (every chunk traced) that make the GPU comparison of the case worth running."""
    _, W, H = IMAGES[name]
    C = lg[0] * lg[1]
    want = oracle_frame(ugrt, O, name, lg, True)
    cells, per_cell, flags = ray_cells(want, lg, W * H)
    print("%s %s: R %d, ray cells %d, chunks %d, %d with index >= C/2, %d >= 2^20, most rays in a cell %d, shadowed %d, "
          "lit %d" % (name, lg, want["lgrid"]["R"], len(cells), want["nchunks"], (cells >= C // 2).sum(),
                      (cells >= 1 << 20).sum(), per_cell.max(), (flags == 1).sum(), (flags == 0).sum()))
    if lg == (2, 4096):  # the case of long runs: see the module docstring
        assert len(cells) <= 8 and per_cell.max() > 8192
    else:
        assert len(cells) >= 256
    assert (flags == 1).sum() >= 2000 and (flags == 0).sum() >= 2000
    if C >= 1 << 19:
        assert (cells >= C // 2).sum() >= 64
    if lg == (2048, 1024):
        assert (cells >= 1 << 20).sum() >= 64
    assert per_cell.max() > 64  # a cell of several chunks
    assert want["lgrid"]["R"] <= 1 << 24
    assert want["is_shadowed"].sum() > 0 and want["image"].max() > 0


def test_strict_cap_case_has_more_chunks_than_tiles(ugrt, O):
    want = oracle_frame(ugrt, O, "cornell", (4096, 256), False, (128, 128))
    assert want["nchunks"] > 16 * 16
    # ... and the cap matters: tracing every chunk gives other flags
    every = oracle_frame(ugrt, O, "cornell", (4096, 256), True, (128, 128))
    assert (want["is_shadowed"] != every["is_shadowed"]).any()


def flags_with_cells_masked(ugrt, O, name, lg, keep_bits):
    """The oracle's shadow stage (every chunk) over the frame's rays with each real cell index cut to its low keep_bits
    bits: what a shadow pass that dropped the higher bits of its cell field would compute."""
    _, W, H = IMAGES[name]
    n, C = W * H, lg[0] * lg[1]
    s, want = scene(ugrt, name), oracle_frame(ugrt, O, name, lg, True)
    m = want["map_unsorted"].copy()
    cells = m[n:]
    cells[cells < C] &= np.uint32((1 << keep_bits) - 1)
    prefix, nchunks = O.process_rays(m, n, C + 1, n // 64 + C + 2)
    pr = want["primary"]
    flags = pr["shadowed"].copy()
    O.trace_shadow(want["lcam"].cc, want["lgrid"], C, s["verts"], s["faces"], pr["t"], pr["dir"], flags, m, prefix,
                   want["cam"].worldori[:3].copy(), nchunks, (W // 8) * (H // 8), n, strict=False)
    return flags


@pytest.mark.parametrize("name,lg,keep_bits", [("cornell", (2048, 1024), 20), ("cornell", (1024, 512), 16)],
                         ids=["64-bit keys", "32-bit keys"])
def test_dropping_high_cell_bits_changes_the_flags(ugrt, O, name, lg, keep_bits):
    want = oracle_frame(ugrt, O, name, lg, True)
    np.testing.assert_array_equal(flags_with_cells_masked(ugrt, O, name, lg, 32), want["is_shadowed"])  # the rerun is the frame's
    wrong = flags_with_cells_masked(ugrt, O, name, lg, keep_bits)
    assert (wrong != want["is_shadowed"]).sum() >= 100, (wrong != want["is_shadowed"]).sum()


# ------------------------------------------------------------------------------------------------ GPU

def make(ugrt, name, lg, all_chunks, size=None, options=()):
    u = ugrt
    s = scene(ugrt, name)
    _, W, H = IMAGES[name]
    if size is not None:
        W, H = size
    ctx = u.Context(W, H, light_grid=lg, flags=u.FLAG_SHADOW_ALL_CHUNKS if all_chunks else 0, uniform_dims=(32, 32, 16))
    for k, v in options:
        ctx.set_option(k, v)
    return ctx, u.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])


def assert_light_grid_equal(ugrt, ctx, want):
    value, key, span, offset, gi = ctx.grid_arrays(ugrt.GRID_SPHERICAL)
    g = want["lgrid"]
    assert gi.total_refs == g["R"] and gi.num_cells == len(g["span"])
    np.testing.assert_array_equal(u32(key), g["keys"])
    np.testing.assert_array_equal(u32(value), g["vals"])
    np.testing.assert_array_equal(u32(span), g["span"])
    np.testing.assert_array_equal(u32(offset), g["offset"])


def assert_sorted_rays_equal(r, want):
    assert r.num_chunks == want["nchunks"]
    np.testing.assert_array_equal(u32(r.d_map), want["map"])
    np.testing.assert_array_equal(u32(r.prefix)[:r.num_chunks], want["prefix"][:want["nchunks"]])


def assert_pixels_equal(r, want):
    np.testing.assert_array_equal(r.t.cpu().numpy().view(np.uint32), bits(want["primary"]["t"]))
    np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), want["is_shadowed"])
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), want["mat_ids"])
    np.testing.assert_array_equal(r.image.cpu().numpy(), want["image"])


def assert_frame_equal(ugrt, ctx, r, want):
    assert_light_grid_equal(ugrt, ctx, want)
    assert_sorted_rays_equal(r, want)
    assert_pixels_equal(r, want)


SWEEP_MODES = [(name, lg, all_chunks) for name, lg in SWEEP for all_chunks in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,lg,all_chunks", SWEEP_MODES, ids=ids_of(SWEEP_MODES))
def test_light_grid_sweep(ugrt, O, torch, name, lg, all_chunks):
    ctx, r = make(ugrt, name, lg, all_chunks)
    assert ctx.get_state("shadow_key_bits") == 0
    r.display(setup_of(ugrt, name), frame_cnt=1, shadows=True)
    ctx.synchronize()
    assert ctx.get_state("shadow_key_bits") == GRIDS[lg]
    assert_frame_equal(ugrt, ctx, r, oracle_frame(ugrt, O, name, lg, all_chunks))


@pytest.mark.gpu
def test_strict_cap_with_more_chunks_than_tiles(ugrt, O, torch):
    """traced = min(num_chunks, nbx nby) - 1 where the minimum is the tile count: 4 229 chunks, 256 tiles."""
    lg, size = (4096, 256), (128, 128)
    want = oracle_frame(ugrt, O, "cornell", lg, False, size)
    assert want["nchunks"] > 16 * 16
    ctx, r = make(ugrt, "cornell", lg, False, size=size)
    r.display(setup_of(ugrt, "cornell"), frame_cnt=1, shadows=True)
    ctx.synchronize()
    assert ctx.get_state("shadow_key_bits") == 51
    assert_frame_equal(ugrt, ctx, r, want)


OPTION_CASES = [
    # scene, light grid, all chunks, options, key bits
    ("hall", (128, 128), True, (("shadow_key64", 1),), 45),
    ("cornell", (256, 256), True, (("shadow_key64", 1),), 47),
    ("crash", (1024, 512), True, (("shadow_mbits", 9),), 29),
    ("cornell", (2, 4096), True, (("shadow_beam", 64),), 32),
    ("cornell", (2, 4096), True, (("shadow_beam", 8192),), 32),
    ("hall", (1024, 1024), True, (("shadow_beam", 64),), 51),
    ("hall", (1024, 1024), True, (("shadow_beam", 8192),), 51),
    ("crash", (1024, 512), False, (("sort_library", 1),), 32),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,lg,all_chunks,options,keybits", OPTION_CASES,
                         ids=["%s-%dx%d-%s%d" % (c[0], c[1][0], c[1][1], c[3][0][0], c[3][0][1]) for c in OPTION_CASES])
def test_shadow_options_at_sizes_they_never_ran_at(ugrt, O, torch, name, lg, all_chunks, options, keybits):
    ctx, r = make(ugrt, name, lg, all_chunks, options=options)
    r.display(setup_of(ugrt, name), frame_cnt=1, shadows=True)
    ctx.synchronize()
    assert ctx.get_state("shadow_key_bits") == keybits
    if options[0][0] == "shadow_key64":
        assert keybits > 32
    assert_frame_equal(ugrt, ctx, r, oracle_frame(ugrt, O, name, lg, all_chunks))


@pytest.mark.gpu
def test_async_shadow_pass_at_64_bit_keys(ugrt, O, torch):
    """The second frame of a context with "async_build" runs builds and shadow pass in the form that does not wait;
    ugrt_ctx_synchronize reports no overflow, and the frame is the oracle's."""
    name, lg = "cornell", (1024, 1024)
    ctx, r = make(ugrt, name, lg, True, options=(("async_build", 1),))
    for _ in range(2):
        r.is_shadowed.fill_(-1)
        r.image.zero_()
        r.display(setup_of(ugrt, name), frame_cnt=1, shadows=True)
    ctx.synchronize()  # (raises on UGRT_EOVERFLOW)
    assert ctx.get_state("shadow_key_bits") == 51
    assert_frame_equal(ugrt, ctx, r, oracle_frame(ugrt, O, name, lg, True))


@pytest.mark.gpu
def test_deferred_chunk_form_at_a_wide_grid(ugrt, O, torch):
    """ugrt_sort_rays(..., NULL) under FLAG_SHADOW_ALL_CHUNKS puts the sort off: the shadow pass reads the unsorted map,
    and processData's outputs are produced when they are asked for."""
    name, lg = "hall", (4096, 256)
    _, W, H = IMAGES[name]
    want = oracle_frame(ugrt, O, name, lg, True)
    ctx, r = make(ugrt, name, lg, True)
    r.display(setup_of(ugrt, name), frame_cnt=1, shadows=True)
    ctx.synchronize()
    np.testing.assert_array_equal(u32(r._d_map), want["map_unsorted"])  # nothing sorted the map so far
    assert (np.diff(u32(r._d_map)[W * H:].astype(np.int64)) < 0).any()
    assert_pixels_equal(r, want)
    assert_sorted_rays_equal(r, want)
    assert_light_grid_equal(ugrt, ctx, want)


@pytest.mark.gpu
@pytest.mark.parametrize("all_chunks", [False, True])
def test_slab_union_feeds_the_pass_a_large_grid(ugrt, O, torch, all_chunks):
    """slabs = 2 at (512,256): the light grid has 2^18 keys and k_slab_union folds them to the 2^17 cells the shadow pass
    walks; Cornell's depth-spread camera, whose hits lie in both slabs."""
    import test_reference_kernels as RK

    u = ugrt
    build, W, H = RK.DEPTH_SPREAD["cornellBz_128"]
    s, setup = build(u)
    lg = (512, 256)
    ctx = u.Context(W, H, light_grid=lg, flags=u.FLAG_SHADOW_ALL_CHUNKS if all_chunks else 0, uniform_dims=(32, 32, 16),
                    slabs=2)
    r = u.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    r.display(setup, frame_cnt=1, shadows=True)
    ctx.synchronize()
    want = O.frame(s, setup, W, H, light_grid=lg, all_chunks=all_chunks, slabs=2)
    assert len(want["lgrid"]["span"]) == 1 << 18
    assert ctx.get_state("shadow_key_bits") == key_bits(lg) == 32
    assert_frame_equal(ugrt, ctx, r, want)
    one = O.frame(s, setup, W, H, light_grid=lg, all_chunks=all_chunks)
    assert ((one["primary"]["id"] >= 0) & (want["primary"]["id"] < 0)).sum() > 0  # the slab walk's reset path ran
    assert want["is_shadowed"].sum() > 0
