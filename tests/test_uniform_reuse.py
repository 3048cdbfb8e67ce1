"""ugrt_grid_build_uniform keeps the grid while its inputs stand (UGRT_FLAG_STATIC_GEOMETRY): the calls that are
reused, every change that must build again, and the frames and grids on both sides against the CPU oracle.
Cornell box, 128 x 128, light grid 32 x 32, uniform grids of 16 x 16 x 8 and 32 x 32 x 16 cells."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 128
LG = (32, 32)
UDIMS = [(16, 16, 8), (32, 32, 16)]
KEY = "uniform_builds_reused"


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_SCENE, _WANT = {}, {}


def cornell(ugrt):
    if "s" not in _SCENE:
        s = dict(ugrt.scenes.cornell())
        # (the box's own materials do not reflect: every surface half a mirror, so that the bounce walks the grid)
        s["reflect"] = np.full(len(s["reflect"]), 0.5, np.float32)
        _SCENE["s"] = s
        _SCENE["setup"] = ugrt.FrameSetup(s["cameras"]["B"], s["light_camera"], s["shading_light"])
        v0 = np.asarray(s["verts"], np.float32).reshape(-1, 3)
        _SCENE["v"] = {"v0": v0, "v1": (v0 * np.float32(0.75)).astype(np.float32)}
    return _SCENE["s"], _SCENE["setup"]


def want_for(O, ugrt, tag, ud, verts=None):
    """The oracle's frame for the geometry `tag` (computed once per geometry and grid size, never changed)."""
    s, setup = cornell(ugrt)
    if (tag, ud) not in _WANT:
        v = _SCENE["v"][tag] if verts is None else verts
        _WANT[(tag, ud)] = O.frame(s, setup, W, H, light_grid=LG, reflect=True, uniform_dims=ud, verts=v)
    return _WANT[(tag, ud)]


def make(ugrt, ud, flags=None, **kw):
    s, _ = cornell(ugrt)
    ctx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_STATIC_GEOMETRY if flags is None else flags, uniform_dims=ud)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], **kw)
    return ctx, r


def uctx(r):
    """The context that builds the uniform grid: the second one of a two-stream renderer."""
    return r.aux if r.aux is not None else r.ctx


def frames(r, setup, n=1):
    for _ in range(n):
        r.display(setup, shadows=True, reflect=True)
        r.synchronize()


def assert_grid(ugrt, c, g, what):
    value, key, span, offset, gi = c.grid_arrays(ugrt.GRID_UNIFORM)
    np.testing.assert_array_equal(u32(key), g["keys"], err_msg=what)
    np.testing.assert_array_equal(u32(value), g["vals"], err_msg=what)
    np.testing.assert_array_equal(u32(span), g["span"], err_msg=what)
    np.testing.assert_array_equal(u32(offset), g["offset"], err_msg=what)


def assert_frame(ugrt, r, want, what):
    np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), want["mat_ids"], err_msg=what)
    np.testing.assert_array_equal(bits(r.t.cpu().numpy()), bits(want["primary"]["t"]), err_msg=what)
    np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), want["is_shadowed"], err_msg=what)
    np.testing.assert_array_equal(r.hit_id.cpu().numpy(), want["hit_id"], err_msg=what)
    np.testing.assert_array_equal(bits(r.hit_t.cpu().numpy()), bits(want["hit_t"]), err_msg=what)
    np.testing.assert_array_equal(r.image.cpu().numpy(), want["image"], err_msg=what)
    assert_grid(ugrt, uctx(r), want["ugrid"], what)


def set_verts(torch, r, v):
    """The caller rewrites the vertex tensor in place (and knows the new box); it has to say so itself."""
    r.d_verts.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1)).to(r.d_verts.device))
    r.bbmin, r.bbmax = v.min(0), v.max(0)
    for c in (r.ctx, r.aux):
        if c is not None:
            c.geometry_changed()


@pytest.mark.parametrize("ud", UDIMS)
def test_second_frame_keeps_the_grid(ugrt, O, torch, ud):
    """Two frames under the flag: the counter goes 0 -> 1, the grid's arrays stay where they are and keep every byte,
    and the second frame is the oracle's."""
    s, setup = cornell(ugrt)
    ctx, r = make(ugrt, ud)
    assert ctx.get_state(KEY) == 0
    frames(r, setup)
    assert ctx.get_state(KEY) == 0
    first = ctx.grid_arrays(ugrt.GRID_UNIFORM)
    ptrs = [x.data_ptr() for x in first[:4]]
    kept = [x.clone() for x in first[:4]]
    info = (first[4].total_refs, first[4].cells_used, first[4].num_cells)
    frames(r, setup)
    assert ctx.get_state(KEY) == 1
    second = ctx.grid_arrays(ugrt.GRID_UNIFORM)
    assert [x.data_ptr() for x in second[:4]] == ptrs
    for a, b, n in zip(second[:4], kept, ("value", "key", "span", "offset")):
        assert torch.equal(a, b), n
    assert (second[4].total_refs, second[4].cells_used, second[4].num_cells) == info
    assert_frame(ugrt, r, want_for(O, ugrt, "v0", ud), "second frame")
    assert int(r.active.sum()) > 100  # (the bounce has rays to walk the kept grid with)


@pytest.mark.parametrize("ud", UDIMS)
@pytest.mark.parametrize("kind", ["geometry_changed", "animate", "box", "clone", "no_flag", "option_off"])
def test_every_change_builds_again(ugrt, O, torch, kind, ud):
    """Two frames (the second reused), then the change: the next frame builds (the counter stands still) and is the
    oracle's for the new geometry; the frame after that is reused again.  animate: ugrt_animate, then the frame's
    screen-grid build, which makes the triangle records valid again BEFORE the uniform build is asked for -- the
    records being valid says nothing about the uniform grid."""
    s, setup = cornell(ugrt)
    ctx, r = make(ugrt, ud, flags=0 if kind == "no_flag" else None)
    if kind == "option_off":
        ctx.set_option("uniform_reuse", 0)
    never = kind in ("no_flag", "option_off")
    frames(r, setup, 2)
    assert ctx.get_state(KEY) == (0 if never else 1)
    assert_frame(ugrt, r, want_for(O, ugrt, "v0", ud), kind + ": before")
    before = ctx.get_state(KEY)
    want, grid_only = want_for(O, ugrt, "v0", ud), None
    if kind == "geometry_changed":
        set_verts(torch, r, _SCENE["v"]["v1"])
        want = want_for(O, ugrt, "v1", ud)
    elif kind == "animate":
        r.init_orig_list(8, 16)
        r.rotate_bunny(0.3)
        ctx.synchronize()
        v = r.d_verts.cpu().numpy().reshape(-1, 3).copy()
        assert np.abs(v - _SCENE["v"]["v0"]).max() > 1e-3
        # the trap on its own: a screen-grid build, then the uniform build with the pointers, F and the box (the OLD
        # one, bit for bit) all what they were -- only the generation differs
        ctx.grid_build_perspective(r.d_faces, r.d_verts, r.F)
        ctx.grid_build_uniform(r.d_faces, r.d_verts, r.F, r.bbmin, r.bbmax)
        ctx.synchronize()
        assert ctx.get_state(KEY) == before
        assert_grid(ugrt, ctx, O.grid_uniform(s["faces"], v, r.bbmin, r.bbmax, ud), "animate, the old box")
        r.bbmin, r.bbmax = v.min(0), v.max(0)
        want = want_for(O, ugrt, "animated", ud, verts=v)
    elif kind == "box":
        r.bbmin = r.bbmin - np.float32(3.0)
        r.bbmax = r.bbmax + np.float32(5.0)
        grid_only = O.grid_uniform(s["faces"], s["verts"], r.bbmin, r.bbmax, ud)
    elif kind == "clone":
        r.d_verts = r.d_verts.clone()  # the same values behind a new pointer
    frames(r, setup)
    assert ctx.get_state(KEY) == before, kind
    if grid_only is not None:
        # the same triangles in other cells: the nearest hits are what they were, the grid is the oracle's for this box
        assert_grid(ugrt, ctx, grid_only, kind)
        np.testing.assert_array_equal(bits(r.hit_t.cpu().numpy()), bits(want["hit_t"]))
        assert not np.array_equal(grid_only["span"], want["ugrid"]["span"])
    else:
        assert_frame(ugrt, r, want, kind + ": after")
    frames(r, setup)
    assert ctx.get_state(KEY) == (0 if never else before + 1), kind
    if grid_only is not None:
        assert_grid(ugrt, ctx, grid_only, kind)
    else:
        assert_frame(ugrt, r, want, kind + ": reused again")


@pytest.mark.parametrize("ud", UDIMS)
def test_face_window_and_merged_shards_build_again(ugrt, O, torch, ud):
    """A changed face window builds again (and the same window is then kept); ugrt_grid_merge_shards rewrites the
    grid's arrays, so the build behind it builds too.  Every grid is the oracle's for its window."""
    s, setup = cornell(ugrt)
    ctx, r = make(ugrt, ud)
    F = r.F
    build = lambda: ctx.grid_build_uniform(r.d_faces, r.d_verts, F, r.bbmin, r.bbmax)
    full = O.grid_uniform(s["faces"], s["verts"], r.bbmin, r.bbmax, ud)
    half = O.grid_uniform(s["faces"], s["verts"], r.bbmin, r.bbmax, ud, window=(F // 3, F))
    build()
    build()
    ctx.synchronize()
    assert ctx.get_state(KEY) == 1
    assert_grid(ugrt, ctx, full, "full")
    ctx.set_face_window(F // 3, F)
    build()
    ctx.synchronize()
    assert ctx.get_state(KEY) == 1
    assert_grid(ugrt, ctx, half, "window")
    build()
    assert ctx.get_state(KEY) == 2
    ctx.set_face_window(0, -1)
    build()
    ctx.synchronize()
    assert ctx.get_state(KEY) == 2
    assert_grid(ugrt, ctx, full, "full again")
    build()
    assert ctx.get_state(KEY) == 3
    # a merge of one part (the grid itself, copied): the arrays are rewritten, the grid is no longer a build's
    value, key, span, offset, gi = ctx.grid_arrays(ugrt.GRID_UNIFORM)
    ctx.grid_merge_shards(ugrt.GRID_UNIFORM, [key.clone()], [value.clone()], [span.clone()], [gi.total_refs])
    ctx.synchronize()
    assert_grid(ugrt, ctx, full, "merged")
    build()
    ctx.synchronize()
    assert ctx.get_state(KEY) == 3
    assert_grid(ugrt, ctx, full, "built behind the merge")
    build()
    assert ctx.get_state(KEY) == 4
    frames(r, setup)
    assert ctx.get_state(KEY) == 5
    assert_frame(ugrt, r, want_for(O, ugrt, "v0", ud), "frame on the kept grid")


@pytest.mark.parametrize("helper_thread", [True, False])
def test_two_stream_renderer(ugrt, O, torch, helper_thread):
    """overlap=True: the second context builds (and keeps) the uniform grid and has to hear of a change itself."""
    ud = UDIMS[1]
    s, setup = cornell(ugrt)
    ctx, r = make(ugrt, ud, overlap=True, helper_thread=helper_thread)
    frames(r, setup, 2)
    assert r.aux.get_state(KEY) == 1 and ctx.get_state(KEY) == 0
    assert_frame(ugrt, r, want_for(O, ugrt, "v0", ud), "before")
    set_verts(torch, r, _SCENE["v"]["v1"])
    frames(r, setup)
    assert r.aux.get_state(KEY) == 1
    assert_frame(ugrt, r, want_for(O, ugrt, "v1", ud), "after the change")
    frames(r, setup, 2)
    # (one host thread: the builds are asynchronous, so the build behind the change is confirmed by a waiting one first)
    assert r.aux.get_state(KEY) == (3 if helper_thread else 2)
    assert_frame(ugrt, r, want_for(O, ugrt, "v1", ud), "reused after the change")
    r.close()


def test_two_renderers_in_flight(ugrt, O, torch):
    """Two two-stream renderers on their own streams, dealt frames in turn without a synchronisation in between;
    then a geometry change on both of them (all four contexts)."""
    ud = UDIMS[0]
    s, setup = cornell(ugrt)
    rs = []
    for i in range(2):
        stream = torch.cuda.Stream() if i else None
        with torch.cuda.stream(stream):
            ctx, r = make(ugrt, ud, overlap=True, helper_thread=False)
        r._stream = stream
        rs.append(r)

    def deal(n):
        for k in range(2 * n):
            r = rs[k % 2]
            with torch.cuda.stream(r._stream):
                r.display(setup, shadows=True, reflect=True)
        for r in rs:
            r.synchronize()
        torch.cuda.synchronize()

    deal(3)  # a waiting build, then two frames on it
    for i, r in enumerate(rs):
        assert r.aux.get_state(KEY) == 2, i
        assert_frame(ugrt, r, want_for(O, ugrt, "v0", ud), "renderer %d" % i)
    for r in rs:
        with torch.cuda.stream(r._stream):
            set_verts(torch, r, _SCENE["v"]["v1"])
    deal(3)  # an asynchronous build, the waiting one that confirms it, one frame on that
    for i, r in enumerate(rs):
        assert r.aux.get_state(KEY) == 3, i
        assert_frame(ugrt, r, want_for(O, ugrt, "v1", ud), "renderer %d after the change" % i)


@pytest.mark.parametrize("ud", UDIMS)
def test_async_build_is_confirmed_before_it_is_kept(ugrt, O, torch, ud):
    """async_build = 1, a geometry change, three frames: the first builds asynchronously, the second waits (an
    asynchronous build may have overflowed and left an emptied grid: it is never reused), the third is kept.  All three
    are the oracle's."""
    s, setup = cornell(ugrt)
    ctx, r = make(ugrt, ud)
    ctx.set_option("async_build", 1)
    frames(r, setup, 3)  # the grid's first build waits (there is no estimate yet)
    assert ctx.get_state(KEY) == 2
    set_verts(torch, r, _SCENE["v"]["v1"])
    want = want_for(O, ugrt, "v1", ud)
    for k, reused in enumerate((2, 2, 3)):
        frames(r, setup)
        assert ctx.get_state(KEY) == reused, k
        assert_frame(ugrt, r, want, "frame %d behind the change" % k)
    frames(r, setup)
    assert ctx.get_state(KEY) == 4


def test_async_build_that_overflowed_is_repaired_then_kept(ugrt, O, torch):
    """Much larger geometry behind a small one: the asynchronous uniform build overflows its estimate and is emptied.
    The synchronisation reports it, the repeated frame waits and is right, and the frames after it keep that grid."""
    ud = UDIMS[1]
    small, big = ugrt.scenes.crash(scale=0.02), ugrt.scenes.crash(scale=0.12)
    setup = ugrt.FrameSetup(small["cameras"]["ref"], small["light_camera"], small["shading_light"])
    vs, vb = (np.asarray(x["verts"], np.float32).reshape(-1, 3) for x in (small, big))
    Rs = O.grid_uniform(small["faces"], vs, vs.min(0), vs.max(0), ud)["R"]
    Rb = O.grid_uniform(big["faces"], vb, vb.min(0), vb.max(0), ud)["R"]
    assert Rb > Rs + Rs // 4 + 65536, (Rs, Rb)  # more than the launch an asynchronous build is given
    ctx = ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_STATIC_GEOMETRY, uniform_dims=ud)
    ctx.set_option("async_build", 1)
    ra = ugrt.Renderer(ctx, small["verts"], small["faces"], small["matidx"], small["mat_list"], small["reflect"])
    frames(ra, setup, 3)
    assert ctx.get_state(KEY) == 2
    rb = ugrt.Renderer(ctx, big["verts"], big["faces"], big["matidx"], big["mat_list"], big["reflect"])
    rb.display(setup, shadows=True, reflect=True)
    with pytest.raises(ugrt.UgrtError, match="asynchronous"):
        ctx.synchronize()
    assert ctx.get_state(KEY) == 2
    want = O.frame(big, setup, W, H, light_grid=LG, reflect=True, uniform_dims=ud)
    frames(rb, setup)  # the repair: every build waits
    assert ctx.get_state(KEY) == 2
    assert_frame(ugrt, rb, want, "repaired frame")
    frames(rb, setup)
    assert ctx.get_state(KEY) == 3
    assert_frame(ugrt, rb, want, "frame on the repaired grid")


def test_reused_build_inside_a_batch(ugrt, O, torch):
    """ugrt_grid_build_batch_begin / _end with a uniform build that is kept: the batch is the light grid alone, or
    nothing at all."""
    ud = UDIMS[1]
    s, setup = cornell(ugrt)
    ctx, r = make(ugrt, ud, overlap=True, helper_thread=False, batch_builds=True)
    frames(r, setup, 2)
    assert r.aux.get_state(KEY) == 1
    assert_frame(ugrt, r, want_for(O, ugrt, "v0", ud), "batch of one")
    set_verts(torch, r, _SCENE["v"]["v1"])
    want = want_for(O, ugrt, "v1", ud)
    for k, reused in enumerate((1, 1, 2)):  # a batch of two, the waiting build beside a batch of one, a batch of one
        frames(r, setup)
        assert r.aux.get_state(KEY) == reused, k
        assert_frame(ugrt, r, want, "frame %d behind the change" % k)
    lg = want["lgrid"]
    value, key, span, offset, gi = r.aux.grid_arrays(ugrt.GRID_SPHERICAL)
    np.testing.assert_array_equal(u32(key), lg["keys"])
    np.testing.assert_array_equal(u32(value), lg["vals"])
    np.testing.assert_array_equal(u32(span), lg["span"])
    r.aux.grid_build_batch_begin()
    r.aux.grid_build_uniform(r.d_faces, r.d_verts, r.F, r.bbmin, r.bbmax)
    r.aux.grid_build_batch_end()
    r.aux.synchronize()
    assert r.aux.get_state(KEY) == 3
    assert_grid(ugrt, r.aux, want["ugrid"], "an empty batch")


@pytest.mark.parametrize("ud", UDIMS)
def test_any_hit_walk_behind_a_reused_build(ugrt, O, torch, ud):
    """ugrt_trace_dda_any shares the occupancy bitmap with the bounce.  Behind a reused build, with no bounce in between,
    it has to make the bitmap itself; behind the next build it has to make it anew.  A ray is occluded (t_max beyond
    everything) exactly where the oracle's nearest-hit walk finds a hit."""
    s, setup = cornell(ugrt)
    ctx, r = make(ugrt, ud)
    N = W * H
    for tag in ("v0", "v1"):
        want = want_for(O, ugrt, tag, ud)
        if tag == "v1":
            set_verts(torch, r, _SCENE["v"]["v1"])
        before = ctx.get_state(KEY)
        for _ in range(2):
            ctx.grid_build_uniform(r.d_faces, r.d_verts, r.F, r.bbmin, r.bbmax)
        assert ctx.get_state(KEY) == before + 1
        g = ctx.grid_ptrs(ugrt.GRID_UNIFORM)
        active = np.ascontiguousarray(want["active"], np.int32)
        assert int(active.sum()) > 100
        expect = ((active != 0) & (want["hit_id"] >= 0)).astype(np.int32)
        for k in range(2):  # the second walk finds the bitmap current
            occ = torch.full((N,), -7, dtype=torch.int32, device=ctx.device)
            ctx.trace_dda_any(g[0], g[1], g[2], r.d_verts, r.d_faces, ctx.upload(want["rays"]), ctx.upload(active), 3.0e38, occ)
            ctx.synchronize()
            np.testing.assert_array_equal(occ.cpu().numpy(), expect, err_msg="%s walk %d" % (tag, k))
        assert 0 < int(expect.sum())
