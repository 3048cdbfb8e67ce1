"""The shadow tracer's candidate pairs bucketed by counting (option "shadow_pairs", the default) against the sorted path.

Between the cull pass and the exact pass the (beam, triangle) candidates have to end up beam by beam, large apparent
size first.  "shadow_pairs" 0 sorts them on (beam << size bits | size class); the default counts them per bucket in the
cull pass, scans the counts and places the triangle ids (ugrt_trace_shadow.hip: k_shadow_cull, PairBucketLoad,
k_pair_place).  The order inside a bucket is the order in which waves happened to arrive, so it differs from run to run;
a ray's flag is 1 iff ANY triangle of its cell occludes it, so no flag may.

The inputs are the cases of test_shadow_synthetic (that file's docstring has their figures): A 256 x 128 with light
grid (32,16), B 256 x 64 with (64,32), C 64 x 64 with (512,256); cell lists of 1, 63, 64, 65, 129 and 17 000 triangles;
up to 11 552 rays in a cell; rays alone in their cell.  test_broken_stages_change_the_flags there shows that a lost
candidate changes flags (384 in case A when the lists are cut at 64).  Every comparison is flag for flag with the CPU
oracle.  Which path a pass took is read from ugrt_ctx_get_state "shadow_pairs_counted".
"""
import types

import numpy as np
import pytest

import test_shadow_synthetic as SS
from test_shadow_synthetic import stage, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ALL = sorted(SS.CASES) + ["C"]
BUCKET_WORDS = 1 << 22  # SHADOW_BUCKET_WORDS: (beam bound << size bits) up to which the pairs are counted
EOVERFLOW = 6


def bits_for(v):
    """Key bits of v values, as the library's bits_of and test_gpu_parity.bits_for_cells count them."""
    b = 1
    while (1 << b) < v:
        b += 1
    return b


def beam_bound(S):
    """Beams the rays of a context could form at most: what the waiting form's bucket table is made for."""
    return S.N // 64 + S.C + 1


def run_with(s, options):
    """One map, sort and trace under the options, which are reset to -1 afterwards: (flags, counted, radix launches)."""
    try:
        for name, value in options:
            s.ctx.set_option(name, value)
        before = s.ctx.get_state("radix_launches")
        flags = s.run()[3]
        return flags, s.ctx.get_state("shadow_pairs_counted"), s.ctx.get_state("radix_launches") - before
    finally:
        for name, _ in options:
            s.ctx.set_option(name, -1)


@pytest.mark.parametrize("pairs", [-1, 0], ids=["counted", "sorted"])
@pytest.mark.parametrize("all_chunks", [True, False], ids=["all-chunks", "strict"])
@pytest.mark.parametrize("case", ALL)
def test_flags_equal_the_oracle(ugrt, O, stage, case, all_chunks, pairs):
    s, w = stage(case, all_chunks=all_chunks), SS.want(O, case, not all_chunks)
    flags, counted, _ = run_with(s, (("shadow_pairs", pairs),))
    assert counted == (0 if pairs == 0 else 1)
    SS.assert_flags_equal(flags, w, "%s pairs %d" % (case, pairs))


SHAPES = [(("shadow_sizebits", 0),), (("shadow_sizebits", 4),), (("shadow_sizebits", 8),),
          (("shadow_beam", 64),), (("shadow_beam", 8192),), (("shadow_xseg", 64),), (("shadow_xseg", 1 << 20),),
          (("shadow_itemsort", 0),), (("shadow_sieve", 0),), (("shadow_xcd_run", 0),)]


@pytest.mark.parametrize("options", SHAPES, ids=["-".join("%s%d" % o for o in opts) for opts in SHAPES])
def test_launch_shapes_with_counted_pairs(ugrt, O, stage, options):
    """Each option alone with the counted path, then reset: 1, 16 and 256 buckets per beam, more than GCHUNK beams in a
    cell and one beam for 8192 rays, more than 255 segments of a beam's run and one, the unsorted item list, a wave per
    item, the persistent exact pass."""
    s, w = stage("A", all_chunks=True), SS.want(O, "A", False)
    assert (beam_bound(s.S) << 8) <= BUCKET_WORDS
    flags, counted, _ = run_with(s, options)
    assert counted == 1
    SS.assert_flags_equal(flags, w, str(options))
    flags, counted, _ = run_with(s, ())
    assert counted == 1
    SS.assert_flags_equal(flags, w, "after " + str(options))


@pytest.mark.parametrize("case", ALL)
def test_work_counters_equal_the_sorted_path_s(ugrt, O, stage, case):
    """Cull tests and staged candidates are sums over the beams of (triangles of the cell) and of (candidates x 64-ray
    sub-groups): equal sums pin the per-beam bucket totals to the sorted path's run lengths."""
    s, w = stage(case, all_chunks=True), SS.want(O, case, False)
    stats = {}
    for pairs in (-1, 0):
        flags, counted, _ = run_with(s, (("shadow_pairs", pairs),))
        assert counted == (0 if pairs == 0 else 1)
        SS.assert_flags_equal(flags, w, "%s pairs %d" % (case, pairs))
        stats[pairs] = s.ctx.stats()
    print(case, "beams", stats[-1][1], "cull tests", stats[-1][6], "staged candidates", stats[-1][7])
    assert stats[-1][1] == stats[0][1] > 0
    assert stats[-1][6] == stats[0][6] > 0
    assert stats[-1][7] == stats[0][7] > 0


def test_placement_order_changes_no_flag(ugrt, O, stage):
    s, w = stage("A", all_chunks=True), SS.want(O, "A", False)
    for rep in range(3):
        flags, counted, _ = run_with(s, ())
        assert counted == 1
        SS.assert_flags_equal(flags, w, "run %d" % rep)


@pytest.mark.parametrize("sbits", [-1, 0, 8])
def test_the_pair_sort_s_launches_are_gone(ugrt, O, stage, sbits):
    """The sorted path's pair sort runs one radix pass per 8 bits of (beam << size bits | class) and no histogram launch
    (the compaction counts the first digit); the counted path runs none of them, and the item sort that follows still
    finds its first digit counted (one pass, no histogram launch, in both)."""
    s = stage("A", all_chunks=True)
    launches = {}
    for pairs in (-1, 0):
        flags, counted, launches[pairs] = run_with(s, (("shadow_pairs", pairs), ("shadow_sizebits", sbits)))
        assert counted == (0 if pairs == 0 else 1)
        SS.assert_flags_equal(flags, SS.want(O, "A", False), "pairs %d" % pairs)
    G = s.ctx.stats()[1]
    passes = (bits_for(G) + (4 if sbits < 0 else sbits) + 7) // 8
    print("beams", G, "launches", launches, "pair sort passes", passes)
    assert launches[0] - launches[-1] == passes, (launches, G)


def test_asynchronous_form(ugrt, O):
    """A waiting pass leaves estimates; asynchronous passes on the same rays then give the same flags.  With 64-ray beams
    the same rays form more beams than the bucket table of the estimate has: the cull pass must not count beyond the
    table, the pass reports UGRT_EOVERFLOW at the synchronisation, and the repeat (which waits) is right, as are the
    asynchronous passes after it."""
    S, w = SS.synthetic(O, "A"), SS.want(O, "A", False)
    s = SS.Stage(ugrt, S, ugrt.FLAG_SHADOW_ALL_CHUNKS)
    SS.assert_flags_equal(s.run()[3], w, "waiting")
    beams = s.ctx.stats()[1]
    s.ctx.set_option("async_build", 1)
    for rep in range(2):
        SS.assert_flags_equal(s.run()[3], w, "asynchronous %d" % rep)
        assert s.ctx.get_state("shadow_pairs_counted") == 1
    # (the asynchronous form's beam bound: the power of two above the estimate plus a quarter)
    bound = 1
    while bound < beams + beams // 4 + 1:
        bound <<= 1
    s.ctx.set_option("shadow_beam", 64)
    with pytest.raises(ugrt.UgrtError) as e:
        s.run()
    assert e.value.code == EOVERFLOW, e.value
    SS.assert_flags_equal(s.run()[3], w, "the repeat")
    assert s.ctx.stats()[1] > bound
    for rep in range(2):
        SS.assert_flags_equal(s.run()[3], w, "asynchronous, 64-ray beams, %d" % rep)
        assert s.ctx.get_state("shadow_pairs_counted") == 1


def test_fallbacks_to_the_sorted_path(ugrt, O, stage):
    """The library's sort, and a bucket table beyond its bound (case C's 131 585 possible beams x 256 size classes),
    sort the pairs whatever "shadow_pairs" says; the flags are the same."""
    a, c = stage("A", all_chunks=True), stage("C", all_chunks=True)
    for s, options, counted in ((a, (("sort_library", 1),), 0), (a, (("sort_library", 1), ("shadow_pairs", 1)), 0),
                                (c, (("shadow_sizebits", 8),), 0), (c, (("shadow_sizebits", 8), ("shadow_pairs", 1)), 0),
                                (c, (("shadow_sizebits", 4),), 1), (c, (("shadow_pairs", 1),), 1)):
        flags, got, _ = run_with(s, options)
        assert got == counted, options
        SS.assert_flags_equal(flags, SS.want(O, s.S.case, False), str(options))
    assert (beam_bound(c.S) << 8) > BUCKET_WORDS >= (beam_bound(c.S) << 4)


def no_candidates(O, same_cell):
    """Case A's image with ONE small triangle in the light grid and every ray aimed at one point Q.  same_cell False:
    Q lies in another light cell than the triangle, no ray forms a beam.  True: Q lies in the triangle's cell, three
    degrees beside it: the rays form beams whose direction box is a point, and the cull pass keeps no pair."""
    A = SS.synthetic(O, "A")
    d = SS.unit(np.array([0.3, 0.5, 0.81]))
    side = SS.unit(np.cross(d, [0.0, 0.0, 1.0]))
    tri = (SS.L + 8.0 * d)[None, :] + 0.01 * np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    verts = np.ascontiguousarray(tri, np.float32)
    faces = np.arange(3, dtype=np.int32).reshape(1, 3)
    grid = O.grid_spherical(A.lcam.cc, faces, verts, A.lg[0], A.lg[1], xM=SS.PI_F, yM=SS.PI_F)
    for angle in ((3.0, -3.0, 2.0, -2.0, 1.0, -1.0) if same_cell else (60.0, 90.0, 120.0)):
        a = np.radians(angle)
        Q = SS.L + 20.0 * (np.cos(a) * d + np.sin(a) * side)
        dq = Q - SS.CAM_POS
        t = np.full(A.N, np.linalg.norm(dq), np.float32)
        dirs = np.ascontiguousarray(np.tile((dq / np.linalg.norm(dq)).astype(np.float32), A.N))
        S = types.SimpleNamespace(**{**vars(A), "verts": verts, "faces": faces, "F": 1, "t": t, "dirs": dirs})
        w = SS.shadow_stage(O, S, False, grid=grid)
        cells = SS.cell_of_pixel(S, w)
        assert (cells == cells[0]).all() and 0 <= cells[0] < S.C
        if (grid["span"][cells[0]] > 0) == same_cell:
            return S, w
    raise AssertionError("no direction found")


@pytest.mark.parametrize("same_cell", [False, True], ids=["no beams", "beams without candidates"])
def test_no_candidates(ugrt, O, same_cell):
    """No beam, and beams of which the cull pass keeps nothing: the pass ends clean in the waiting and in the
    asynchronous form, counted and sorted, and leaves the incoming flags as they were."""
    S, w = no_candidates(O, same_cell)
    np.testing.assert_array_equal(w["flags"], S.flags)  # (20 units from the light, the triangle at 8, three degrees off)
    s = SS.Stage(ugrt, S, ugrt.FLAG_SHADOW_ALL_CHUNKS)
    for pairs in (-1, 0):
        s.ctx.set_option("shadow_pairs", pairs)
        for async_build in (0, 1, 1):
            s.ctx.set_option("async_build", async_build)
            SS.assert_flags_equal(s.run()[3], w, "pairs %d async %d" % (pairs, async_build))
            assert s.ctx.get_state("shadow_pairs_counted") == (0 if pairs == 0 else 1)
            if not async_build:
                assert (s.ctx.stats()[1] > 0) == same_cell
