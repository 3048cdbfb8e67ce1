"""The screen grid's wide triangles traced from their one list (ugrt_trace_primary_grid), the merge on demand.

A perspective-grid build with wide triangles stops behind its spans and offsets; ugrt_trace_primary_grid reads a cell's
narrow run and then the wide ids and breaks ties by triangle id; the merged lists are written when ugrt_grid_get_info
(grid_arrays) or ugrt_trace_primary on the grid's own arrays asks for them.  Everything here is compared on raw bits,
three ways: the new entry point, the old path on the arrays of grid_arrays, the oracle.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OUTS = ("intersect_id", "t", "normal", "dir", "is_shadowed")
PER_PIXEL = dict(intersect_id=1, t=1, normal=3, dir=3, is_shadowed=1)
ORACLE_NAME = dict(intersect_id="id", t="t", normal="normal", dir="dir", is_shadowed="shadowed")
CAM0 = dict(eye=(0, 0, 0), look=(0, 0, -1), up=(0, 1, 0), near=0.1, far=100.0)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def cornell(ugrt):
    return cached("cornell", ugrt.scenes.cornell)


def plain_scene(verts, faces):
    return dict(verts=np.asarray(verts, np.float32), faces=np.asarray(faces, np.int32),
                matidx=np.zeros(len(faces), np.int32), mat_list=np.array([[0.2, 0.2, 0.2, 0.8, 0.8, 0.8]], np.float32),
                reflect=np.zeros(1, np.float32))


def with_wide_triangles(s, cam, n_extra, seed=3):
    """The scene plus backdrop triangles larger than the view of `cam` (every screen cell) and triangles between
    opposite corners of the scene box, interleaved with the scene's own triangles so that wide ids fall between
    narrow ids (the construction of test_gpu_parity.py)."""
    rng = np.random.default_rng(seed)
    verts, faces = s["verts"].astype(np.float32), s["faces"].astype(np.int32)
    e, look, up = (np.array(cam[k], np.float64) for k in ("eye", "look", "up"))
    f = (look - e) / np.linalg.norm(look - e)
    rt = np.cross(f, up)
    rt /= np.linalg.norm(rt)
    u = np.cross(rt, f)
    ext = []
    for k in range(n_extra):
        j = rng.uniform(0.8, 1.2, 6)
        d = 30.0 + 3.0 * k / n_extra
        ext.append(np.stack([e + d * f - 100 * j[0] * rt - 100 * j[1] * u,
                             e + d * f + 100 * j[2] * rt - 100 * j[3] * u,
                             e + d * f + 10 * j[4] * rt + 100 * j[5] * u]))
    both = np.concatenate([verts] + ext)
    lo, hi = both.min(0), both.max(0)
    for k in range(n_extra):
        c = lo + (hi - lo) * rng.uniform(0.3, 0.7, 3)
        ext.append(np.stack([lo, hi, c]))
    ext = np.concatenate(ext).astype(np.float32)
    v2 = np.concatenate([verts, ext])
    extra_faces = (len(verts) + np.arange(len(ext), dtype=np.int32)).reshape(-1, 3)
    pos = np.sort(rng.integers(0, len(faces) + 1, len(extra_faces)))
    out = dict(s)
    out.update(verts=v2, faces=np.insert(faces, pos, extra_faces, axis=0).astype(np.int32),
               matidx=np.insert(s["matidx"].astype(np.int32), pos, 0))
    return out


def oracle_for(O, key, s, cam, W, H, rows=None, slabs=1):
    """(camera, grid, primary outputs) of the oracle, computed once per case and left unchanged."""
    def make():
        ocam = O.cam_from(cam, 45.0, W / H)
        g = O.grid_perspective(ocam.cc, s["faces"], s["verts"], W // 8, H // 8, rows=rows, slabs=slabs)
        return ocam, g, O.trace_primary(ocam, W, H, g, s["verts"], s["faces"], rows=rows, slabs=slabs)
    return cached(("oracle",) + tuple(key), make)


class Tracer:
    """A context, the scene's device arrays and two sets of output arrays."""

    def __init__(self, ugrt, torch, s, W, H, rows=None, flags=0, slabs=1, options=()):
        self.ugrt, self.torch = ugrt, torch
        self.ctx = ugrt.Context(W, H, light_grid=(16, 16), rows=rows, flags=flags, uniform_dims=(8, 8, 4), slabs=slabs)
        for k, v in options:
            self.ctx.set_option(k, v)
        self.r = ugrt.Renderer(self.ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
        self.other = {n: getattr(self.r, n).clone() for n in OUTS}

    def state(self, key):
        return self.ctx.get_state(key)

    def build(self, ocam):
        self.ctx.upload_camera(ocam.cc)
        self.ctx.grid_build_perspective(self.r.d_faces, self.r.d_verts, self.r.F)

    def _run(self, o, trace):
        for n in OUTS:
            o[n].fill_(-7)  # whatever the trace does not write shows
        trace(o["normal"], o["t"], o["dir"], o["is_shadowed"], o["intersect_id"], self.r.d_verts, self.r.d_faces)
        self.ctx.synchronize()
        a, b = self.ctx.p0, self.ctx.p0 + self.ctx.npix
        return {n: raw(o[n].cpu().numpy().reshape(-1, PER_PIXEL[n])[a:b]) for n in OUTS}

    def trace_grid(self):
        return self._run({n: getattr(self.r, n) for n in OUTS}, self.ctx.trace_primary_grid)

    def trace_lists(self):
        value, _, span, offset, _ = self.ctx.grid_arrays(self.ugrt.GRID_PERSPECTIVE)
        return self._run(self.other, lambda *a: self.ctx.trace_primary(value, span, offset, *a))

    def band(self, want):
        a, b = self.ctx.p0, self.ctx.p0 + self.ctx.npix
        return {n: raw(np.asarray(want[ORACLE_NAME[n]]).reshape(-1, PER_PIXEL[n])[a:b]) for n in OUTS}

    def check_lists(self, g):
        value, key, span, offset, gi = self.ctx.grid_arrays(self.ugrt.GRID_PERSPECTIVE)
        assert gi.total_refs == g["R"] and gi.cells_used == g["used"]
        np.testing.assert_array_equal(u32(key), g["keys"])
        np.testing.assert_array_equal(u32(value), g["vals"])
        np.testing.assert_array_equal(u32(span), g["span"])
        np.testing.assert_array_equal(u32(offset), g["offset"])


def assert_same(got, want, what):
    for n in OUTS:
        np.testing.assert_array_equal(got[n], want[n], err_msg="%s: %s" % (what, n))


def three_ways(T, ocam, g, want, builds=2, deferred=True, what=""):
    """Build and trace `builds` times: the new entry point (which must not merge), then the lists (merged on demand
    AFTER the tracer ran) against the oracle's, then the old path on them."""
    wb = T.band(want)
    for k in range(builds):
        before = T.state("primary_deferred_merges"), T.state("primary_completed_merges")
        T.build(ocam)
        assert T.state("primary_merge_pending") == (1 if deferred else 0), what
        assert T.state("primary_deferred_merges") == before[0] + (1 if deferred else 0), what
        assert_same(T.trace_grid(), wb, "%s new entry point, build %d" % (what, k))
        assert T.state("primary_merge_pending") == (1 if deferred else 0), what
        assert T.state("primary_completed_merges") == before[1], what
        T.check_lists(g)
        assert T.state("primary_merge_pending") == 0 and T.state("primary_completed_merges") == before[1] + (1 if deferred else 0)
        assert_same(T.trace_lists(), wb, "%s old path, build %d" % (what, k))
        assert_same(T.trace_grid(), wb, "%s new entry point after the merge, build %d" % (what, k))
        assert T.state("primary_completed_merges") == before[1] + (1 if deferred else 0)  # (idempotent)


@pytest.mark.parametrize("static", [0, 1])
@pytest.mark.parametrize("async_build", [0, 1])
@pytest.mark.parametrize("rows", [None, (3, 9)])
@pytest.mark.parametrize("n_extra", [1, 7, 200])
def test_cornell_with_wide_triangles(ugrt, O, torch, n_extra, rows, async_build, static):
    cam = cornell(ugrt)["cameras"]["B"]
    s = cached(("wide", n_extra), lambda: with_wide_triangles(cornell(ugrt), cam, n_extra))
    W, H = 128, 96
    ocam, g, want = oracle_for(O, ("wide", n_extra, rows), s, cam, W, H, rows=rows)
    ncell_active = (W // 8) * ((rows[1] - rows[0]) if rows else H // 8)
    assert (np.bincount(g["vals"]) == ncell_active).sum() >= n_extra
    T = Tracer(ugrt, torch, s, W, H, rows=rows, flags=ugrt.FLAG_STATIC_GEOMETRY if static else 0,
               options=[("async_build", async_build)])
    # (the first build of an asynchronous context waits: no estimate yet; the second and third do not)
    three_ways(T, ocam, g, want, builds=3 if async_build else 2)


def test_pointers_kept_from_an_earlier_build_make_the_old_path_merge(ugrt, O, torch):
    """ugrt_trace_primary handed the context's own arrays (pointers of an earlier ugrt_grid_get_info) while the merge
    of a NEW build is pending: it must merge first, the list it is about to read does not exist yet."""
    cam = cornell(ugrt)["cameras"]["B"]
    s = cached(("wide", 7), lambda: with_wide_triangles(cornell(ugrt), cam, 7))
    W, H = 128, 96
    ocam, g, want = oracle_for(O, ("wide", 7, None), s, cam, W, H)
    T = Tracer(ugrt, torch, s, W, H)
    T.build(ocam)
    value, _, span, offset, _ = T.ctx.grid_arrays(ugrt.GRID_PERSPECTIVE)
    value.zero_()  # (what the kept pointers see must come from the NEXT build's merge)
    T.build(ocam)
    assert T.state("primary_merge_pending") == 1
    got = T._run(T.other, lambda *a: T.ctx.trace_primary(value, span, offset, *a))
    assert T.state("primary_merge_pending") == 0
    assert_same(got, T.band(want), "kept pointers")


def _tie_scene(order):
    """Axis-parallel right triangles in the plane z = -128 with legs of 2^k: for such a triangle the reference's t is
    tz * 1/(-dz) whatever its legs and corner, so coplanar ones give equal bits.  One fills the view (wide, twice:
    coincident copies), one is 64 units small (narrow).  `order` lists them."""
    def tri(x, y, leg):
        return [[x, y, -128.0], [x + leg, y, -128.0], [x, y + leg, -128.0]]
    t = dict(n=tri(256.0, 256.0, 64.0), w1=tri(-2048.0, -2048.0, 8192.0), w2=tri(-2048.0, -2048.0, 8192.0))
    return np.array([t[k] for k in order], np.float32).reshape(-1, 3)


@pytest.mark.parametrize("order", [("n", "w1", "w2"), ("w1", "n", "w2"), ("w1", "w2", "n")])
def test_ties_between_wide_and_narrow_triangles(ugrt, O, torch, order):
    s0 = cornell(ugrt)
    cam = s0["cameras"]["B"]
    extra = _tie_scene(order)
    verts = np.concatenate([extra, np.asarray(s0["verts"], np.float32).reshape(-1, 3)])
    faces = np.concatenate([np.arange(9, dtype=np.int32).reshape(3, 3), np.asarray(s0["faces"], np.int32) + 9])
    s = plain_scene(verts, faces)
    W, H = 128, 96
    ocam, g, want = oracle_for(O, ("ties",) + order, s, cam, W, H)
    count = np.bincount(g["vals"], minlength=3)
    ncell = (W // 8) * (H // 8)
    iw, i_n = [order.index("w1"), order.index("w2")], order.index("n")
    assert count[iw[0]] == ncell and count[iw[1]] == ncell and 0 < count[i_n] < ncell
    # the premise: where the narrow triangle alone is hit, the wide one alone gives the same t bits
    alone = {}
    for k in ("n", "w1"):
        sk = plain_scene(_tie_scene((k,)), np.arange(3, dtype=np.int32).reshape(1, 3))
        alone[k] = oracle_for(O, ("ties alone", k), sk, cam, W, H)[2]
    on_n = alone["n"]["id"] == 0
    assert on_n.sum() > 20 and (alone["w1"]["id"] == 0).all()
    np.testing.assert_array_equal(raw(alone["n"]["t"])[on_n], raw(alone["w1"]["t"])[on_n])
    # the smaller id wins
    expect = np.where(on_n, min(i_n, iw[0]), iw[0])
    np.testing.assert_array_equal(want["id"], expect)
    T = Tracer(ugrt, torch, s, W, H)
    three_ways(T, ocam, g, want, what=str(order))
    np.testing.assert_array_equal(T.r.intersect_id.cpu().numpy(), expect)


def _twelve_sheets(ugrt):
    """The scene of test_depth_layers_ties_and_grazing_triangles: twelve screen-filling sheets in shuffled id order, each
    twice with identical vertices, grazing triangles, 2000 small ones."""
    s0 = cornell(ugrt)
    rng = np.random.default_rng(20260412)
    eye = np.array([278.0, 273.0, -800.0])
    tris = []

    def sheet(z, wob):
        a = np.array([[-400, -400, z], [1000, -400, z + wob], [-400, 1000, z - wob]], np.float64)
        b = np.array([[1000, 1000, z], [-400, 1000, z - wob], [1000, -400, z + wob]], np.float64)
        return [a, b]

    for k in range(12):
        z = -500.0 + 37.0 * k
        for _ in range(2):
            tris += sheet(z, 3.0 * (k % 3))
    for k in range(40):
        d = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
        d /= np.linalg.norm(d)
        t0, t1 = rng.uniform(50, 900), rng.uniform(50, 900)
        side = np.cross(d, [0.0, 1.0, 0.0])
        tris.append(np.array([eye + t0 * d, eye + t1 * d, eye + 0.5 * (t0 + t1) * d + 40.0 * side + 1e-3 * np.array([0, 1.0, 0])]))
    for k in range(2000):
        c = np.array([rng.uniform(0, 556), rng.uniform(0, 556), rng.uniform(-600, 500)])
        tris.append(c + rng.uniform(-12, 12, (3, 3)))
    order = rng.permutation(len(tris))
    extra = np.concatenate([tris[i] for i in order]).astype(np.float32)
    verts = np.asarray(s0["verts"], np.float32).reshape(-1, 3)
    f_extra = (len(verts) + np.arange(len(extra), dtype=np.int32)).reshape(-1, 3)
    s = dict(s0)
    s.update(verts=np.concatenate([verts, extra]), faces=np.concatenate([np.asarray(s0["faces"], np.int32), f_extra]),
             matidx=np.concatenate([np.asarray(s0["matidx"], np.int32),
                                    rng.integers(0, len(s0["mat_list"]), len(f_extra)).astype(np.int32)]))
    return s


def test_twelve_sheets_ties_scene(ugrt, O, torch):
    s = cached("sheets", lambda: _twelve_sheets(ugrt))
    cam = cornell(ugrt)["cameras"]["B"]
    W, H = 192, 160
    ocam, g, want = oracle_for(O, ("sheets",), s, cam, W, H)
    assert (np.bincount(g["vals"]) == (W // 8) * (H // 8)).sum() >= 24  # the sheets are wide
    assert (want["id"] >= 0).sum() > 0.9 * want["id"].size
    three_ways(Tracer(ugrt, torch, s, W, H), ocam, g, want)
    # and through a whole frame (Renderer.display traces through the new entry point)
    setup = ugrt.FrameSetup(cam, s["light_camera"], s["shading_light"])
    ctx = ugrt.Context(W, H, light_grid=(32, 32), uniform_dims=(16, 16, 8))
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    for _ in range(2):
        r.display(setup, shadows=True, reflect=True)
        ctx.synchronize()
    assert ctx.get_state("primary_deferred_merges") == 2 and ctx.get_state("primary_completed_merges") == 0
    fw = O.frame(s, setup, W, H, light_grid=(32, 32), reflect=True, uniform_dims=(16, 16, 8))
    np.testing.assert_array_equal(raw(r.t.cpu().numpy()), raw(fw["primary"]["t"]))
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), fw["mat_ids"])
    np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), fw["is_shadowed"])
    np.testing.assert_array_equal(r.hit_id.cpu().numpy(), fw["hit_id"])
    np.testing.assert_array_equal(r.image.cpu().numpy(), fw["image"])


def _crowd_with_backdrops(n_wide):
    """3000 triangles crowded around the view axis (cells of several hundred references, 100 coincident duplicates)
    with n_wide backdrops larger than the view scattered through the id range."""
    rng = np.random.default_rng(7)
    n = 3000
    ctr = rng.uniform(-0.3, 0.3, size=(n, 1, 3)) + np.array([0, 0, -5.0])
    tri = ctr + rng.normal(scale=0.25, size=(n, 3, 3))
    tri = np.concatenate([tri, tri[:100]])
    back = []
    for k in range(n_wide):
        j = rng.uniform(0.8, 1.2, 6)
        d = 9.0 + 2.0 * k / n_wide
        back.append([[-60 * j[0], -60 * j[1], -d], [60 * j[2], -60 * j[3], -d], [5 * j[4], 60 * j[5], -d]])
    pos = np.sort(rng.integers(0, len(tri) + 1, n_wide))
    tri = np.insert(tri, pos, np.array(back), axis=0)
    verts = tri.reshape(-1, 3).astype(np.float32)
    return plain_scene(verts, np.arange(len(verts)).reshape(-1, 3))


@pytest.mark.parametrize("async_build", [0, 1])
def test_split_cells_across_the_seam(ugrt, O, torch, async_build):
    """primary_seg 64: cells of several hundred narrow references and 70 wide ones are cut into items that begin in
    the narrow run, straddle the seam (the narrow counts are no multiples of 64) and begin in the wide list."""
    s = cached("crowd", lambda: _crowd_with_backdrops(70))
    W = H = 64
    ocam, g, want = oracle_for(O, ("crowd",), s, CAM0, W, H)
    nwide = int((np.bincount(g["vals"]) == 64).sum())
    narrow = g["span"].astype(np.int64) - nwide
    assert nwide == 70 and narrow.max() > 600
    assert ((narrow > 64) & (narrow % 64 != 0)).any()  # (70 wide ones behind such a run: an item straddles the seam)
    T = Tracer(ugrt, torch, s, W, H, options=[("primary_seg", 64), ("async_build", async_build)])
    three_ways(T, ocam, g, want, builds=3)  # (the slots of the split cells must be re-armed between traces)
    assert T.ctx.stats()[0] > 64 + int(g["R"]) // 64 - 8  # the work list was sized for items of 64


def test_no_wide_triangle_takes_the_old_path(ugrt, O, torch):
    s = cornell(ugrt)
    cam = s["cameras"]["B"]
    W, H = 128, 96
    ocam, g, want = oracle_for(O, ("plain",), s, cam, W, H)
    assert np.bincount(g["vals"]).max() < (W // 8) * (H // 8)
    for async_build in (0, 1):
        T = Tracer(ugrt, torch, s, W, H, options=[("async_build", async_build)])
        three_ways(T, ocam, g, want, builds=3, deferred=False, what="async_build %d" % async_build)
        assert T.state("primary_deferred_merges") == 0 and T.state("primary_completed_merges") == 0


def test_more_than_4096_wide_triangles_merge_at_once(ugrt, O, torch):
    """The 2-cell grid of test_many_wide_triangles_tiny_grid: the wide ids go through the radix sort, nothing is deferred."""
    rng = np.random.default_rng(11)
    n = 6000
    tri = np.zeros((n, 3, 3))
    tri[:, 0] = np.c_[rng.uniform(-1.5, -0.2, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-6, -4, n)]
    tri[:, 1] = np.c_[rng.uniform(0.2, 1.5, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-6, -4, n)]
    tri[:, 2] = np.c_[rng.uniform(-1.5, 1.5, n), rng.uniform(-0.4, 0.4, n), rng.uniform(-6, -4, n)]
    tri[::5, 1, 0] = -0.1
    verts = tri.reshape(-1, 3).astype(np.float32)
    s = plain_scene(verts, np.arange(len(verts)).reshape(-1, 3))
    W, H = 16, 8
    ocam, g, want = oracle_for(O, ("tiny",), s, CAM0, W, H)
    assert (np.bincount(g["vals"]) == 2).sum() > 4096 and (np.bincount(g["vals"]) == 1).sum() > 500
    T = Tracer(ugrt, torch, s, W, H)
    three_ways(T, ocam, g, want, deferred=False)
    assert T.state("primary_deferred_merges") == 0


def test_z_slabs_merge_at_once(ugrt, O, torch):
    cam = cornell(ugrt)["cameras"]["B"]
    s = cached(("wide", 7), lambda: with_wide_triangles(cornell(ugrt), cam, 7))
    W, H = 128, 96
    ocam, g, want = oracle_for(O, ("wide slabs", 7), s, cam, W, H, slabs=2)
    T = Tracer(ugrt, torch, s, W, H, slabs=2)
    three_ways(T, ocam, g, want, deferred=False)
    assert T.state("primary_deferred_merges") == 0


def test_a_triangle_wide_for_the_band_only(ugrt, O, torch):
    """Rows 3..8 of 12: a sliver across the middle of the view covers every cell of the band, not of the grid."""
    s0 = cornell(ugrt)
    cam = s0["cameras"]["B"]
    e, look, up = (np.array(cam[k], np.float64) for k in ("eye", "look", "up"))
    f = (look - e) / np.linalg.norm(look - e)
    rt = np.cross(f, up)
    rt /= np.linalg.norm(rt)
    u = np.cross(rt, f)
    d = 200.0
    sliver = np.stack([e + d * f - 50 * d * rt - 0.25 * d * u, e + d * f + 50 * d * rt - 0.25 * d * u,
                       e + d * f + 0.25 * d * u]).astype(np.float32)
    verts = np.concatenate([np.asarray(s0["verts"], np.float32).reshape(-1, 3), sliver])
    nf = len(s0["faces"])
    faces = np.insert(np.asarray(s0["faces"], np.int32), nf // 2, len(verts) - 3 + np.arange(3, dtype=np.int32), axis=0)
    s = dict(s0)
    s.update(verts=verts, faces=faces, matidx=np.insert(np.asarray(s0["matidx"], np.int32), nf // 2, 0))
    W, H, rows = 128, 96, (3, 9)
    ocam, g, want = oracle_for(O, ("sliver", rows), s, cam, W, H, rows=rows)
    full = cached(("sliver full",), lambda: O.grid_perspective(ocam.cc, s["faces"], s["verts"], W // 8, H // 8))
    in_band, in_grid = np.bincount(g["vals"], minlength=nf + 1), np.bincount(full["vals"], minlength=nf + 1)
    assert in_band[nf // 2] == (W // 8) * 6 and in_band[nf // 2] < in_grid[nf // 2] < (W // 8) * (H // 8)
    for async_build in (0, 1):
        T = Tracer(ugrt, torch, s, W, H, rows=rows, options=[("async_build", async_build)])
        three_ways(T, ocam, g, want, builds=3)
    # the whole grid holds no wide triangle
    ocam, g, want = oracle_for(O, ("sliver", None), s, cam, W, H)
    three_ways(Tracer(ugrt, torch, s, W, H), ocam, g, want, deferred=False)


def test_two_stream_frame_runs_no_merge(ugrt, O, torch):
    """Renderer(overlap=True), asynchronous builds: frames equal the oracle's, and none of them merged."""
    cam = cornell(ugrt)["cameras"]["B"]
    s = cached(("wide", 7), lambda: with_wide_triangles(cornell(ugrt), cam, 7))
    W, H, lg, ud = 192, 160, (32, 32), (8, 8, 4)
    setup = ugrt.FrameSetup(cam, s["light_camera"], s["shading_light"])
    want = O.frame(s, setup, W, H, light_grid=lg, reflect=True, uniform_dims=ud)
    ctx = ugrt.Context(W, H, light_grid=lg, uniform_dims=ud)
    ctx.set_option("async_build", 1)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], overlap=True)
    try:
        if r.aux is not None:
            r.aux.set_option("async_build", 1)
        frames = 4
        for _ in range(frames):
            r.display(setup, shadows=True, reflect=True)
        r.synchronize()
        assert ctx.get_state("primary_deferred_merges") == frames
        assert ctx.get_state("primary_completed_merges") == 0 and ctx.get_state("primary_merge_pending") == 1
        np.testing.assert_array_equal(raw(r.t.cpu().numpy()), raw(want["primary"]["t"]))
        np.testing.assert_array_equal(raw(r.normal.cpu().numpy()), raw(want["primary"]["normal"]))
        np.testing.assert_array_equal(raw(r.dir.cpu().numpy()), raw(want["primary"]["dir"]))
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), want["mat_ids"])
        np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), want["is_shadowed"])
        np.testing.assert_array_equal(r.hit_id.cpu().numpy(), want["hit_id"])
        np.testing.assert_array_equal(r.image.cpu().numpy(), want["image"])
        # the lists are still there for whoever asks afterwards
        value, key, span, offset, gi = ctx.grid_arrays(ugrt.GRID_PERSPECTIVE)
        assert gi.total_refs == want["grid"]["R"] and ctx.get_state("primary_completed_merges") == 1
        np.testing.assert_array_equal(u32(value), want["grid"]["vals"])
        np.testing.assert_array_equal(u32(key), want["grid"]["keys"])
    finally:
        r.close()
