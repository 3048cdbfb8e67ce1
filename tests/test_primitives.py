"""The two primitives every stage of a frame rests on, tested directly: the single-kernel prefix sum (ugrt_scan,
ugrt_scan_pair) and the radix sort's batched, device-count and in-place forms (ugrt_sort_pairs_lists), and the ray
re-ordering built from both (ugrt_sort_rays).

Integers only: every comparison is exact equality against numpy (np.cumsum in 64 bits masked to 32, np.argsort
kind="stable"; the chunk list also against the oracle's process_rays).  Outputs are 64 words longer than needed and
prefilled with a sentinel that the tail must keep.  Every case runs twice on one context without a synchronize in
between: the state of a scan or a sort (tickets, histogram rows, epoch-tagged look-back words) must be clean after it.
"""
import ctypes

import numpy as np
import pytest

SENT = np.uint32(0xDEADBEEF)
TAIL = 64
SC_TILE = 4096  # words per scan tile; wave 0 looks back 64 tiles a round
SCAN_SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 64 * SC_TILE + 1, 65 * SC_TILE + 1, 129 * SC_TILE + 5, 1000003]
SCAN_KINDS = ["below_2^16", "zeros", "ones", "all_ffffffff", "full_32_bit", "first_only", "last_only"]
# (sort_items, sort_rank): pairs per thread of a pass; 0 = ranks by ballots, -1 = by LDS atomics where the device allows
SORT_SHAPES = [(-1, -1), (8, -1), (16, -1), (8, 0), (16, 0)]


# ---- references and checkers (numpy only) -------------------------------------------------------------------------
def scan_ref(x, inclusive):
    incl = np.cumsum(x.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    if inclusive:
        return incl.astype(np.uint32)
    return np.concatenate([np.zeros(1, np.uint64), incl[:-1]]).astype(np.uint32)


def scan_values(kind, n, rng):
    if kind == "below_2^16":
        return rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint32)
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "ones":
        return np.ones(n, np.uint32)
    if kind == "all_ffffffff":
        return np.full(n, 0xFFFFFFFF, np.uint32)
    if kind == "full_32_bit":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    x = np.zeros(n, np.uint32)
    x[0 if kind == "first_only" else n - 1] = 0x9E3779B9
    return x


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return "" if bad.size == 0 else "%d words differ, the first at %d: got %d, want %d" % (bad.size, bad[0], got[bad[0]], want[bad[0]])


def check_scan(buf, lead, x, inclusive, what=""):
    """buf: the whole output buffer (lead sentinel words, the n sums, >= TAIL sentinel words)."""
    n = x.size
    assert buf.size >= lead + n + TAIL
    d = first_difference(buf[lead:lead + n], scan_ref(x, inclusive))
    assert not d, "scan %s: %s" % (what, d)
    assert (buf[:lead] == SENT).all(), "scan %s: written in front of the output" % what
    assert (buf[lead + n:] == SENT).all(), "scan %s: written behind the output" % what


def mask_of(bits):
    return np.uint32(0xFFFFFFFF) if bits >= 32 else np.uint32((1 << bits) - 1)


def sort_ref(keys, vals, bits, m=None):
    m = keys.size if m is None else min(int(m), keys.size)
    order = np.argsort(keys[:m] & mask_of(bits), kind="stable")
    return keys[:m][order], vals[:m][order]


def check_sorted(out_k, out_v, keys, vals, bits, m=None, behind_k=None, behind_v=None, what="", want=None):
    """out_k / out_v: the whole output buffers.  The first m (default: all) pairs are the stable sort of the first m
    inputs; behind them the buffers hold behind_k / behind_v (default: the sentinel everywhere)."""
    n = keys.size
    m = n if m is None else min(int(m), n)
    want_k, want_v = sort_ref(keys, vals, bits, m) if want is None else want
    for name, out, want, behind in (("keys", out_k, want_k, behind_k), ("values", out_v, want_v, behind_v)):
        assert out.size >= n + TAIL
        d = first_difference(out[:m], want)
        assert not d, "sort %s, %s: %s" % (what, name, d)
        rest = np.full(out.size - m, SENT, np.uint32) if behind is None else behind
        d = first_difference(out[m:], rest)
        assert not d, "sort %s, %s behind the %d sorted pairs (offsets from there): %s" % (what, name, m, d)


def chunks_ref(sorted_keys):
    """First ray of every chunk of at most 64 rays that share a light cell: each run's start + 64 j, ascending."""
    n = sorted_keys.size
    starts = np.flatnonzero(np.concatenate([[True], sorted_keys[1:] != sorted_keys[:-1]]))
    ends = np.concatenate([starts[1:], [n]])
    out = [np.arange(s, e, 64) for s, e in zip(starts, ends)]
    return np.concatenate(out).astype(np.uint32)


def check_chunks(prefix, count, sorted_keys, cap=None, what=""):
    """prefix: the whole prefix buffer, count: the chunk count the call reported, cap: the capacity it was given."""
    want = chunks_ref(sorted_keys)
    assert count == want.size, "chunks %s: count %d, want %d" % (what, count, want.size)
    m = want.size if cap is None else min(cap, want.size)
    d = first_difference(prefix[:m], want[:m])
    assert not d, "chunks %s: %s" % (what, d)
    assert (prefix[m:] == SENT).all(), "chunks %s: written behind the %d chunk starts" % (what, m)


RAY_W, RAY_H = 256, 64
RAY_N = RAY_W * RAY_H
RAY_GRIDS = [(2, 2), (16, 16), (512, 256)]  # 1 pass (copy path), 2 passes (in place), 3 passes (copy path)


def ray_maps(lg):
    """name -> light-cell keys of RAY_N rays; the sentinel cell is lnbx * lnby."""
    C = lg[0] * lg[1]
    n = RAY_N
    rng = np.random.default_rng(C)
    maps = {
        "all_cell_0": np.zeros(n, np.uint32),
        "all_sentinel": np.full(n, C, np.uint32),
        "half_0_half_sentinel": rng.permutation(np.repeat(np.array([0, C], np.uint32), n // 2)),
        "random": rng.integers(0, C + 1, n, dtype=np.uint64).astype(np.uint32),
    }
    # runs of 63, 64, 65 and 128 rays in ascending cells; where the cells run out the rest lies in the sentinel cell
    lens = np.tile(np.array([63, 64, 65, 128]), n // 320 + 1)
    lens = lens[:min(C, lens.size)]
    runs = np.repeat(np.arange(lens.size, dtype=np.uint32), lens)[:n]
    runs = np.concatenate([runs, np.full(n - runs.size, C, np.uint32)])
    maps["runs_63_64_65_128"] = runs
    maps["runs_63_64_65_128_shuffled"] = rng.permutation(runs)
    if C >= n:
        maps["one_ray_per_cell"] = rng.permutation(C)[:n].astype(np.uint32)
    return maps


def ray_map(keys, seed=1):
    """[pixel ids | cell keys]; the pixel ids in a shuffled order, so that every pair is told from every other."""
    return np.concatenate([np.random.default_rng(seed).permutation(keys.size).astype(np.uint32), keys])


# ---- CPU: the calls refuse a null context, the checkers refuse spoiled results, numpy and the oracle agree --------
def test_new_calls_refuse_a_null_context(ugrt):
    P, n1, b8 = ctypes.c_void_p, (ctypes.c_size_t * 1)(1), (ctypes.c_int * 1)(8)
    one = (P * 1)(P(256))
    assert ugrt.lib.ugrt_scan(None, P(256), P(512), 1, 1) == ugrt.UGRT_EINVAL
    assert b"null" in ugrt.lib.ugrt_last_error()
    assert ugrt.lib.ugrt_scan_pair(None, P(256), P(512), P(768), P(1024), 1, 0) == ugrt.UGRT_EINVAL
    assert b"null" in ugrt.lib.ugrt_last_error()
    assert ugrt.lib.ugrt_sort_pairs_lists(None, 1, one, one, one, one, n1, b8, None) == ugrt.UGRT_EINVAL
    assert b"null" in ugrt.lib.ugrt_last_error()


def test_checkers_reject_a_swap_of_equal_keys():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 16, 1000, dtype=np.uint64).astype(np.uint32)
    vals = np.arange(1000, dtype=np.uint32)
    k, v = sort_ref(keys, vals, 8)
    tail = np.full(TAIL, SENT, np.uint32)
    check_sorted(np.concatenate([k, tail]), np.concatenate([v, tail]), keys, vals, 8)
    i = int(np.flatnonzero(k[1:] == k[:-1])[0])
    v[[i, i + 1]] = v[[i + 1, i]]  # still sorted by key, no longer stable
    with pytest.raises(AssertionError, match="values"):
        check_sorted(np.concatenate([k, tail]), np.concatenate([v, tail]), keys, vals, 8)


def test_checkers_reject_a_pair_from_behind_the_device_count():
    rng = np.random.default_rng(2)
    m, cap = 500, 800
    keys = np.concatenate([rng.integers(1, 256, m, dtype=np.uint64).astype(np.uint32), np.zeros(cap - m, np.uint32)])
    vals = np.arange(cap, dtype=np.uint32)
    rest = np.full(cap - m + TAIL, SENT, np.uint32)
    k, v = sort_ref(keys, vals, 8, m)
    check_sorted(np.concatenate([k, rest]), np.concatenate([v, rest]), keys, vals, 8, m)
    k1, v1 = sort_ref(keys, vals, 8, m + 1)  # the zero key behind the count sorts to the front
    with pytest.raises(AssertionError):
        check_sorted(np.concatenate([k1, rest[1:]]), np.concatenate([v1, rest[1:]]), keys, vals, 8, m)


def test_checkers_reject_a_chunk_start_off_by_64():
    keys = np.sort(ray_maps((16, 16))["random"])
    tail = np.full(TAIL, SENT, np.uint32)
    want = chunks_ref(keys)
    check_chunks(np.concatenate([want, tail]), want.size, keys)
    bad = want.copy()
    bad[want.size // 2] += 64
    with pytest.raises(AssertionError, match="chunks"):
        check_chunks(np.concatenate([bad, tail]), want.size, keys)
    with pytest.raises(AssertionError, match="count"):
        check_chunks(np.concatenate([want, tail]), want.size + 1, keys)


def test_checkers_reject_a_prefix_sum_off_by_one_after_a_wrap():
    x = np.full(5000, 0xFFFFFFFF, np.uint32)
    tail = np.full(TAIL, SENT, np.uint32)
    for inclusive in (True, False):
        want = scan_ref(x, inclusive)
        assert want[4999] == (np.uint32((1 << 32) - 5000) if inclusive else np.uint32((1 << 32) - 4999))  # wrapped 4999 times
        check_scan(np.concatenate([want, tail]), 0, x, inclusive)
        bad = want.copy()
        bad[4097] += 1
        with pytest.raises(AssertionError, match="4097"):
            check_scan(np.concatenate([bad, tail]), 0, x, inclusive)
    with pytest.raises(AssertionError, match="behind"):
        check_scan(np.concatenate([scan_ref(x, True), tail[:-1], [np.uint32(0)]]), 0, x, True)


@pytest.mark.parametrize("lg", RAY_GRIDS, ids=lambda lg: "%dx%d" % lg)
def test_numpy_chunk_list_equals_the_oracle(O, lg):
    C = lg[0] * lg[1]
    cap = RAY_N // 64 + C + 2
    for name, keys in ray_maps(lg).items():
        m = ray_map(keys)
        k, v = sort_ref(keys, m[:RAY_N], 32)
        work = m.copy()
        prefix, nchunks = O.process_rays(work, RAY_N, C + 1, cap)
        np.testing.assert_array_equal(work[:RAY_N], v, err_msg=name)
        np.testing.assert_array_equal(work[RAY_N:], k, err_msg=name)
        want = chunks_ref(k)
        assert nchunks == want.size, name
        np.testing.assert_array_equal(prefix[:nchunks], want, err_msg=name)
        # what the issue spells out: every chunk starts a run or lies a multiple of 64 behind its run's start
        assert (np.diff(want.astype(np.int64)) > 0).all()


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def torch():
    import torch

    return torch


def i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def sentinel(ctx, n):
    return ctx.torch.full((int(n),), int(SENT.view(np.int32)), dtype=ctx.torch.int32, device=ctx.device)


class Scans:
    """Scans enqueued on one context and checked after ONE synchronize at the end."""

    def __init__(self, ctx):
        self.ctx, self.pending = ctx, []

    def single(self, x, inclusive, in_off=0, out_off=0, reps=2, what=""):
        n = x.size
        d_in = self.ctx.upload(i32(np.concatenate([np.zeros(in_off, np.uint32), x])))[in_off:]
        for rep in range(reps):
            buf = sentinel(self.ctx, out_off + n + TAIL)
            self.ctx.scan(d_in, buf[out_off:out_off + n], inclusive=inclusive)
            self.pending.append((buf, out_off, x, inclusive, "%s n=%d %s in+%d out+%d call %d" % (
                what, n, "inclusive" if inclusive else "exclusive", in_off, out_off, rep)))

    def pair(self, xa, xb, inclusive, off=(0, 0, 0, 0), reps=2, what=""):
        n = xa.size
        ins = [self.ctx.upload(i32(np.concatenate([np.zeros(o, np.uint32), x])))[o:] for x, o in ((xa, off[0]), (xb, off[2]))]
        for rep in range(reps):
            bufs = [sentinel(self.ctx, o + n + TAIL) for o in (off[1], off[3])]
            self.ctx.scan_pair(ins[0], bufs[0][off[1]:off[1] + n], ins[1], bufs[1][off[3]:off[3] + n], inclusive=inclusive)
            for buf, o, x, ab in ((bufs[0], off[1], xa, "a"), (bufs[1], off[3], xb, "b")):
                self.pending.append((buf, o, x, inclusive, "%s pair %s n=%d %s offsets %s call %d" % (
                    what, ab, n, "inclusive" if inclusive else "exclusive", off, rep)))

    def check(self):
        self.ctx.synchronize()
        for buf, lead, x, inclusive, what in self.pending:
            check_scan(host(buf), lead, x, inclusive, what)
        self.pending = []


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_sizes_and_values(ugrt, torch, n):
    """Ragged last thread and tile, one, two and three look-back rounds, sums that wrap the 32-bit value field."""
    rng = np.random.default_rng(n)
    s = Scans(ugrt.Context(64, 64))
    for kind in SCAN_KINDS:
        x = scan_values(kind, n, rng)
        for inclusive in (True, False):
            s.single(x, inclusive, what=kind)
        s.check()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 4097, 65 * SC_TILE + 1])
def test_scan_alignment(ugrt, torch, n):
    """in / out as views at word offsets 0..3: both 16-byte aligned, either one not, neither; the same words each time."""
    rng = np.random.default_rng(n + 7)
    x = scan_values("full_32_bit", n, rng)
    s = Scans(ugrt.Context(64, 64))
    for in_off in range(4):
        for out_off in range(4):
            for inclusive in (True, False):
                s.single(x, inclusive, in_off, out_off, what="alignment")
    s.check()


@pytest.mark.gpu
def test_scan_state_over_sizes_and_contexts(ugrt, torch):
    """The state buffer grows and is zeroed again between scans; the ticket is left clean for the next scan."""
    rng = np.random.default_rng(11)
    big, small = scan_values("full_32_bit", 1000003, rng), scan_values("below_2^16", 17, rng)
    s = Scans(ugrt.Context(64, 64))
    for inclusive in (True, False):
        for x in (big, small, big):
            s.single(x, inclusive, reps=1, what="large-small-large")
    s.check()
    s = Scans(ugrt.Context(64, 64))  # fresh: the first scan allocates 256 bytes of state, the second outgrows them
    for x in (small, big, small):
        s.single(x, True, reps=1, what="small-large on a fresh context")
    s.check()


@pytest.mark.gpu
def test_scan_after_a_sort_and_after_a_grid_build(ugrt, torch):
    rng = np.random.default_rng(12)
    x = scan_values("full_32_bit", 65 * SC_TILE + 1, rng)
    ctx = ugrt.Context(64, 64, uniform_dims=(8, 8, 8))
    s = Scans(ctx)
    keys = rng.integers(0, 1 << 32, 100003, dtype=np.uint64).astype(np.uint32)
    dk = ctx.upload(i32(keys))
    ok, ov = torch.empty_like(dk), torch.empty_like(dk)
    ctx.sort_pairs(dk, ok, dk, ov, 20)
    s.single(x, True, what="after sort_pairs")
    verts = rng.uniform(-1, 1, (600, 3)).astype(np.float32)
    faces = rng.integers(0, 600, (200, 3)).astype(np.int32)
    dv, df = ctx.upload(verts.reshape(-1)), ctx.upload(faces.reshape(-1))
    ctx.grid_build_uniform(df, dv, 200, verts.min(0), verts.max(0))
    s.single(x, False, what="after grid_build_uniform")
    s.check()
    np.testing.assert_array_equal(host(ok), sort_ref(keys, keys, 20)[0])
    # the grid's own scans: offsets are the exclusive sums of the spans, the spans add up to the references
    value, key, span, offset, gi = ctx.grid_arrays(ugrt.GRID_UNIFORM)
    assert gi.num_cells == 512 and gi.total_refs > 0
    np.testing.assert_array_equal(host(offset), scan_ref(host(span), False))
    assert int(host(span).sum()) == gi.total_refs


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 4097, 65 * SC_TILE + 1, 129 * SC_TILE + 5])
def test_scan_pair(ugrt, torch, n):
    """Two scans in one launch (the second on state + tiles and ctrl + 2), interleaved with single scans."""
    rng = np.random.default_rng(n + 13)
    xa, xb = scan_values("full_32_bit", n, rng), scan_values("below_2^16", n, rng)
    xc = scan_values("full_32_bit", 2 * n + 3, rng)
    s = Scans(ugrt.Context(64, 64))
    for inclusive in (True, False):
        s.pair(xa, xb, inclusive)
        s.single(xc, inclusive, reps=1, what="between two pairs")
        s.pair(xb, xa, inclusive, reps=1)
        s.pair(xa, xb, inclusive, off=(1, 0, 0, 0), reps=1)  # one input / one output off the 16-byte grid
        s.pair(xa, xb, inclusive, off=(0, 0, 0, 3), reps=1)
    s.check()


class Lists:
    """One or two lists for ugrt_sort_pairs_lists: uploads, sentinel-filled outputs per run, one check of all runs."""

    def __init__(self, ctx, specs):
        """specs: per list (keys, vals, bits, count or None, in_place)."""
        self.ctx, self.specs, self.runs = ctx, specs, []
        self.inputs = [None if in_place else (ctx.upload(i32(keys)), ctx.upload(i32(vals))) for keys, vals, bits, count, in_place in specs]
        self.counts = [None if count is None else ctx.upload(np.array([count], np.uint32).view(np.int32))
                       for keys, vals, bits, count, in_place in specs]

    def run(self):
        dev, tail = [], np.full(TAIL, SENT, np.uint32)
        for (keys, vals, bits, count, in_place), inp, dc in zip(self.specs, self.inputs, self.counts):
            n = keys.size
            if in_place:
                k, v = self.ctx.upload(i32(np.concatenate([keys, tail]))), self.ctx.upload(i32(np.concatenate([vals, tail])))
                dev.append((k, k, v, v, bits, dc, n))
            else:
                dev.append((inp[0], sentinel(self.ctx, n + TAIL), inp[1], sentinel(self.ctx, n + TAIL), bits, dc, n))
        self.ctx.sort_pairs_lists(dev)
        self.runs.append(dev)
        return self

    def launches(self):
        """One histogram kernel and one kernel per pass level of the list with the most passes."""
        passes = [(bits + 7) // 8 for keys, vals, bits, count, in_place in self.specs if keys.size]
        return 1 + max(passes) if passes else 0

    def check(self, what=""):
        tail = np.full(TAIL, SENT, np.uint32)
        for j, (keys, vals, bits, count, in_place) in enumerate(self.specs):
            n = keys.size
            m = n if count is None else min(count, n)
            want = sort_ref(keys, vals, bits, m)
            for rep, dev in enumerate(self.runs):
                ki, ko, vi, vo = dev[j][:4]
                w = "%s call %d list %d (n %d, %d bits, count %s%s)" % (what, rep, j, n, bits, count, ", in place" if in_place else "")
                if in_place:  # behind the sorted pairs the arrays still hold their inputs
                    check_sorted(host(ko), host(vo), keys, vals, bits, m, np.concatenate([keys[m:], tail]),
                                 np.concatenate([vals[m:], tail]), what=w, want=want)
                else:
                    check_sorted(host(ko), host(vo), keys, vals, bits, m, what=w, want=want)
            if not in_place:
                assert not first_difference(host(self.inputs[j][0]), keys) and not first_difference(host(self.inputs[j][1]), vals), \
                    "%s list %d: inputs touched" % (what, j)


def rand_keys(rng, n, kind="rand"):
    if kind == "const":
        return np.full(n, 0xABCDEF, np.uint32)
    if kind == "desc":
        return np.arange(n, 0, -1, dtype=np.uint32)
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def sort_shapes(ctx):
    for items, rank in SORT_SHAPES:
        ctx.set_option("sort_items", items)
        ctx.set_option("sort_rank", rank)
        yield "sort_items %d sort_rank %d" % (items, rank)
    ctx.set_option("sort_items", -1)
    ctx.set_option("sort_rank", -1)


def plain_sort_still_right(ctx, rng):
    keys = rand_keys(rng, 12345)
    vals = rng.permutation(12345).astype(np.uint32)
    dk, dv = ctx.upload(i32(keys)), ctx.upload(i32(vals))
    ok, ov = sentinel(ctx, 12345 + TAIL), sentinel(ctx, 12345 + TAIL)
    before = ctx.get_state("radix_launches")
    ctx.sort_pairs(dk, ok, dv, ov, 15)
    assert ctx.get_state("radix_launches") - before == 3
    ctx.synchronize()
    check_sorted(host(ok), host(ov), keys, vals, 15, what="ugrt_sort_pairs afterwards")


TWO_LISTS = [
    ((1000, 8), (300000, 24), "rand"),     # 1 pass against 3: list 0 drops out
    ((300000, 20), (5, 3), "rand"),
    ((0, 8), (70000, 16), "rand"),
    ((70000, 16), (0, 8), "rand"),
    ((900000, 12), (4097, 32), "rand"),    # the large list picks tiles of 8192 for both; 2 passes against 4
    ((131072, 16), (131072, 16), "rand"),  # an exact multiple of the tile
    ((300000, 20), (1000, 8), "const"),
    ((4097, 32), (300000, 12), "desc"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("a,b,kind", TWO_LISTS, ids=lambda p: p if isinstance(p, str) else "%dx%d" % p)
def test_sort_two_lists_in_shared_launches(ugrt, torch, a, b, kind):
    """Each list equals its own stable sort and shows no value of the other (disjoint value ranges)."""
    rng = np.random.default_rng(a[0] + b[0] + a[1])
    specs = []
    for j, (n, bits) in enumerate((a, b)):
        vals = (rng.permutation(n).astype(np.uint32) + np.uint32(j << 31)).astype(np.uint32)
        specs.append((rand_keys(rng, n, kind), vals, bits, None, False))
    ctx = ugrt.Context(64, 64)
    for shape in sort_shapes(ctx):
        r = Lists(ctx, specs)
        for rep in range(2):
            before = ctx.get_state("radix_launches")
            r.run()
            assert ctx.get_state("radix_launches") - before == r.launches(), shape
        ctx.synchronize()
        r.check(shape)
    plain_sort_still_right(ctx, rng)


@pytest.mark.gpu
def test_one_list_equals_sort_pairs(ugrt, torch):
    rng = np.random.default_rng(5)
    n = 100003
    keys, vals = rand_keys(rng, n), rng.permutation(n).astype(np.uint32)
    ctx = ugrt.Context(64, 64)
    for bits in (8, 13, 20, 32):
        for shape in sort_shapes(ctx):
            dk, dv = ctx.upload(i32(keys)), ctx.upload(i32(vals))
            ok, ov = sentinel(ctx, n + TAIL), sentinel(ctx, n + TAIL)
            ctx.sort_pairs(dk, ok, dv, ov, bits)
            r = Lists(ctx, [(keys, vals, bits, None, False)]).run()
            ctx.synchronize()
            w = "%d bits %s" % (bits, shape)
            assert not first_difference(host(r.runs[0][0][1]), host(ok)), w
            assert not first_difference(host(r.runs[0][0][3]), host(ov)), w
            r.check(w)


DEVICE_CAP = 200000
DEVICE_COUNTS = [0, 1, 4095, 4096, 4097, 65536, 199999, 200000, 250000]


def counted_keys(rng, cap, m, bits):
    """Counted keys are >= 1 on the sorted bits, the keys behind the count are 0: a pair wrongly taken in sorts to the front."""
    keys = rand_keys(rng, cap)
    keys[(keys & mask_of(bits)) == 0] |= np.uint32(1)
    keys[min(m, cap):] = 0
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [8, 16, 20])
def test_sort_with_a_device_count(ugrt, torch, bits):
    """Launches sized by the capacity: the first min(count, capacity) pairs are sorted, nothing is written behind them."""
    rng = np.random.default_rng(bits)
    vals = rng.permutation(DEVICE_CAP).astype(np.uint32)
    ctx = ugrt.Context(64, 64)
    for count in DEVICE_COUNTS:
        keys = counted_keys(rng, DEVICE_CAP, count, bits)
        for shape in sort_shapes(ctx):
            before = ctx.get_state("radix_launches")
            r = Lists(ctx, [(keys, vals, bits, count, False)]).run().run()
            assert ctx.get_state("radix_launches") - before == 2 * r.launches()
            ctx.synchronize()
            r.check(shape)
    plain_sort_still_right(ctx, rng)


@pytest.mark.gpu
def test_two_lists_only_the_second_with_a_device_count(ugrt, torch):
    rng = np.random.default_rng(6)
    a = (rand_keys(rng, 50000), rng.permutation(50000).astype(np.uint32), 16, None, False)
    b = (counted_keys(rng, DEVICE_CAP, 70001, 20), rng.permutation(DEVICE_CAP).astype(np.uint32) + np.uint32(1 << 31), 20, 70001, False)
    ctx = ugrt.Context(64, 64)
    for shape in sort_shapes(ctx):
        r = Lists(ctx, [a, b]).run().run()
        ctx.synchronize()
        r.check(shape)
    plain_sort_still_right(ctx, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [9, 16, 25, 32])
def test_sort_in_place(ugrt, torch, bits):
    """2 or 4 passes: the input is read in the first pass only, the last pass writes it."""
    rng = np.random.default_rng(bits + 100)
    ctx = ugrt.Context(64, 64)
    for n in (5, 4097, 300000):
        vals = rng.permutation(n).astype(np.uint32)
        for count in (None, n - n // 3):
            keys = rand_keys(rng, n) if count is None else counted_keys(rng, n, count, bits)
            for shape in sort_shapes(ctx):
                before = ctx.get_state("radix_launches")
                r = Lists(ctx, [(keys, vals, bits, count, True)]).run().run()
                assert ctx.get_state("radix_launches") - before == 2 * r.launches()
                ctx.synchronize()
                r.check(shape)
    plain_sort_still_right(ctx, rng)


@pytest.mark.gpu
def test_sort_lists_refuses_what_it_cannot_sort(ugrt, torch):
    rng = np.random.default_rng(7)
    ctx = ugrt.Context(64, 64)
    n = 1000
    keys, vals = rand_keys(rng, n), rng.permutation(n).astype(np.uint32)

    def bufs():
        return ctx.upload(i32(keys)), ctx.upload(i32(vals)), sentinel(ctx, n + TAIL), sentinel(ctx, n + TAIL)

    def refused(lists, word):
        before = ctx.get_state("radix_launches")
        with pytest.raises(ugrt.UgrtError, match=word) as e:
            ctx.sort_pairs_lists(lists)
        assert e.value.code == ugrt.UGRT_EINVAL and ctx.get_state("radix_launches") == before

    for bits in (8, 17, 24):  # 1 or 3 passes in place
        k, v, _, _ = bufs()
        refused([(k, k, v, v, bits)], "in place")
        ctx.synchronize()
        assert not first_difference(host(k), keys) and not first_difference(host(v), vals)
    k, v, ko, vo = bufs()
    refused([(k, k, v, vo, 16)], "only one")
    refused([(k, ko, v, v, 16)], "only one")
    refused([(k, ko, v, ko, 16)], "another array")
    refused([(k, v, v, vo, 16)], "another array")
    k2, v2, ko2, vo2 = bufs()
    refused([(k, ko, v, vo, 16), (k2, ko, v2, vo2, 16)], "another array")
    refused([(k, ko, v, vo, 16), (k2, ko2, v2, k, 16)], "another array")
    refused([], r"0 lists \(1\.\.2\)")
    refused([(k, ko, v, vo, 16)] * 3, r"3 lists \(1\.\.2\)")
    refused([(k, ko, v, vo, 0)], "key_bits")
    refused([(k, ko, v, vo, 33)], "key_bits")
    refused([(k, None, v, vo, 16)], "null")
    with pytest.raises(ugrt.UgrtError, match="alias"):
        ctx.scan(k, k)
    with pytest.raises(ugrt.UgrtError, match="alias"):
        ctx.scan_pair(k, ko, v, ko)
    with pytest.raises(ugrt.UgrtError, match="null"):
        ctx.scan(k, None)
    ctx.scan(k, None, n=0)  # nothing to do
    ctx.sort_pairs_lists([(k, ko, v, vo, 16), (k2, ko2, k2, vo2, 8)])  # a list's two inputs may be one array
    ctx.synchronize()
    check_sorted(host(ko), host(vo), keys, vals, 16, what="after the refusals")
    plain_sort_still_right(ctx, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("lg", RAY_GRIDS, ids=lambda lg: "%dx%d" % lg)
def test_ray_reordering_on_synthetic_maps(ugrt, torch, O, lg):
    """ugrt_sort_rays (sort, run bounds, the scan of the chunk counts, chunk starts) on maps no camera produces."""
    C = lg[0] * lg[1]
    ctx = ugrt.Context(RAY_W, RAY_H, light_grid=lg)
    cap = ctx.prefix_capacity()
    assert ctx.npix == RAY_N and cap >= RAY_N // 64 + C + 1
    for name, keys in ray_maps(lg).items():
        m = ray_map(keys)
        k, v = sort_ref(keys, m[:RAY_N], 32)
        work = m.copy()
        oracle_prefix, oracle_count = O.process_rays(work, RAY_N, C + 1, cap)
        assert oracle_count == chunks_ref(k).size and not first_difference(work, np.concatenate([v, k])), name
        maps = [ctx.upload(i32(np.concatenate([m, np.full(TAIL, SENT, np.uint32)]))) for rep in range(2)]
        prefixes = [sentinel(ctx, cap + TAIL) for rep in range(2)]
        # the first call leaves its count on the device and does not wait, the second reads its own back
        assert ctx.sort_rays(maps[0], prefixes[0][:cap], deferred=True) == ugrt.CHUNKS_ON_DEVICE
        count = ctx.sort_rays(maps[1], prefixes[1][:cap])
        for rep in range(2):
            w = "%s call %d" % (name, rep)
            got = host(maps[rep])
            assert not first_difference(got[:RAY_N], v), w + ": pixel half"
            assert not first_difference(got[RAY_N:2 * RAY_N], k), w + ": key half"
            assert (got[2 * RAY_N:] == SENT).all(), w + ": written behind the map"
            check_chunks(host(prefixes[rep]), count, k, cap, what=w)
            assert not first_difference(host(prefixes[rep])[:count], oracle_prefix[:count]), w + ": oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("lg", RAY_GRIDS, ids=lambda lg: "%dx%d" % lg)
def test_ray_reordering_with_a_prefix_map_one_entry_short(ugrt, torch, lg):
    ctx = ugrt.Context(RAY_W, RAY_H, light_grid=lg)
    maps = ray_maps(lg)
    keys = maps["random"]
    m = ray_map(keys)
    k, v = sort_ref(keys, m[:RAY_N], 32)
    count = chunks_ref(k).size
    d_map, prefix = ctx.upload(i32(m)), sentinel(ctx, count + TAIL)
    with pytest.raises(ugrt.UgrtError, match="do not fit") as e:
        ctx.sort_rays(d_map, prefix[:count - 1])
    assert e.value.code == ugrt.UGRT_EINVAL
    ctx.synchronize()
    check_chunks(host(prefix), count, k, count - 1, what="capacity one short")
    assert not first_difference(host(d_map), np.concatenate([v, k]))
    # the context sorts the next map as if nothing had happened
    keys = maps["runs_63_64_65_128_shuffled"]
    m = ray_map(keys, seed=2)
    k, v = sort_ref(keys, m[:RAY_N], 32)
    d_map, prefix = ctx.upload(i32(m)), sentinel(ctx, ctx.prefix_capacity() + TAIL)
    count = ctx.sort_rays(d_map, prefix[:ctx.prefix_capacity()])
    assert not first_difference(host(d_map), np.concatenate([v, k]))
    check_chunks(host(prefix), count, k, ctx.prefix_capacity(), what="after the refusal")
