"""ugrt_grid_build_spherical keeps the light grid while the light and the geometry stand (UGRT_FLAG_STATIC_GEOMETRY):
the calls that are reused, every change that must build again, and the frames and light grids on both sides against
the CPU oracle.  Cornell box with every material half a mirror, 128 x 128, camera "B", uniform grid 16 x 16 x 8, light
grids of 32 x 32 and 8 x 8 cells.  Three light cameras: L0 the scene's own, L1 moved, L2 at L0's eye but turned (only
the rotation block of the camera coordinates changes)."""
import numpy as np
import pytest

import test_lights as TL
from test_lights import LT  # noqa: F401  (the fixture: tests/lights_ref.c, for the several-lights frames)

pytestmark = pytest.mark.gpu

W = H = 128
UD = (16, 16, 8)
LGS = [(32, 32), (8, 8)]
KEY, UKEY = "light_builds_reused", "uniform_builds_reused"
# shadowed pixels per light grid and light camera, and flags that differ from L0's, on the CPU oracle (strict chunk rule)
SHADOWED = {(32, 32): {"L0": (1740, 0), "L1": (1066, 1288), "L2": (1494, 378)},
            (8, 8): {"L0": (2180, 0), "L1": (1854, 744), "L2": (2825, 649)}}


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
        base = s["light_camera"]
        _SCENE["lights"] = {"L0": base, "L1": dict(base, eye=(150, 540, 200), look=(150, 0, 200)),
                            "L2": dict(base, look=(278, 0, 330))}
        v0 = np.asarray(s["verts"], np.float32).reshape(-1, 3)
        _SCENE["v"] = {"v0": v0, "v1": (v0 * np.float32(0.75)).astype(np.float32)}
    return _SCENE["s"]


def setup_for(ugrt, light="L0"):
    s = cornell(ugrt)
    return ugrt.FrameSetup(s["cameras"]["B"], _SCENE["lights"][light], s["shading_light"])


def want_for(O, ugrt, lg, light="L0", tag="v0", verts=None, slabs=1):
    """The oracle's frame for a light camera, a geometry and a light grid (computed once each, never changed)."""
    s = cornell(ugrt)
    k = (lg, light, tag, slabs)
    if k not in _WANT:
        v = _SCENE["v"][tag] if verts is None else verts
        _WANT[k] = O.frame(s, setup_for(ugrt, light), W, H, light_grid=lg, reflect=True, uniform_dims=UD, verts=v, slabs=slabs)
    return _WANT[k]


def light_cc(O, ugrt, light="L0"):
    """The light camera's block as the oracle makes it, and the renderer's camera to upload."""
    setup = setup_for(ugrt, light)
    return (O.cam_from(setup.light_camera, setup.fovy, 1.0).cc, ugrt.renderer.make_camera(setup.light_camera, setup.fovy, 1.0))


def make(ugrt, lg, flags=None, slabs=1, **kw):
    s = cornell(ugrt)
    ctx = ugrt.Context(W, H, light_grid=lg, flags=ugrt.FLAG_STATIC_GEOMETRY if flags is None else flags, uniform_dims=UD,
                       slabs=slabs)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], **kw)
    return ctx, r


def lctx(r):
    """The context that builds the light grid: the second one of a two-stream renderer."""
    return r.aux if r.aux is not None else r.ctx


def frames(r, setup, n=1):
    for _ in range(n):
        r.display(setup, shadows=True, reflect=True)
        r.synchronize()


def assert_grid(ugrt, c, g, what):
    value, key, span, offset, gi = c.grid_arrays(ugrt.GRID_SPHERICAL)
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
    assert_grid(ugrt, lctx(r), want["lgrid"], what)


def set_verts(torch, r, v):
    """The caller rewrites the vertex tensor in place (and knows the new box); it has to say so itself."""
    r.d_verts.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1)).to(r.d_verts.device))
    r.bbmin, r.bbmax = v.min(0), v.max(0)
    for c in (r.ctx, r.aux):
        if c is not None:
            c.geometry_changed()


@pytest.mark.parametrize("lg", LGS)
def test_the_oracle_tells_the_light_cameras_apart(ugrt, O, lg):
    """Conditions on the oracle alone, so that a stale grid cannot pass below: the three light cameras' grids differ,
    and their shadow flags differ on hundreds of pixels."""
    w0 = want_for(O, ugrt, lg)
    for light in ("L0", "L1", "L2"):
        w = want_for(O, ugrt, lg, light)
        got = (int(w["is_shadowed"].sum()), int((w["is_shadowed"] != w0["is_shadowed"]).sum()))
        print("light grid %r, %s: %d shadowed, %d flags differ from L0's" % (lg, light, got[0], got[1]))
        assert got == SHADOWED[lg][light], (lg, light, got)
        if light != "L0":
            assert not np.array_equal(w["lgrid"]["span"], w0["lgrid"]["span"]), (lg, light)
    cc0, cc2 = light_cc(O, ugrt, "L0")[0], light_cc(O, ugrt, "L2")[0]
    assert np.array_equal(bits(cc0[:3]), bits(cc2[:3])) and not np.array_equal(bits(cc0[16:27]), bits(cc2[16:27]))


@pytest.mark.parametrize("lg", LGS)
def test_second_frame_keeps_the_grid(ugrt, O, torch, lg):
    """Two frames under the flag: the counter goes 0 -> 1, the light grid's arrays stay where they are and keep every
    byte, grid_info says what it said, and the second frame is the oracle's."""
    setup = setup_for(ugrt)
    ctx, r = make(ugrt, lg)
    assert ctx.get_state(KEY) == 0
    frames(r, setup)
    assert ctx.get_state(KEY) == 0
    first = ctx.grid_arrays(ugrt.GRID_SPHERICAL)
    ptrs = [x.data_ptr() for x in first[:4]]
    kept = [x.clone() for x in first[:4]]
    info = (first[4].total_refs, first[4].cells_used, first[4].num_cells)
    frames(r, setup)
    assert ctx.get_state(KEY) == 1
    second = ctx.grid_arrays(ugrt.GRID_SPHERICAL)
    assert [x.data_ptr() for x in second[:4]] == ptrs
    for a, b, n in zip(second[:4], kept, ("value", "key", "span", "offset")):
        assert torch.equal(a, b), n
    assert (second[4].total_refs, second[4].cells_used, second[4].num_cells) == info
    want = want_for(O, ugrt, lg)
    assert info == (want["lgrid"]["R"], want["lgrid"]["used"], lg[0] * lg[1])
    assert_frame(ugrt, r, want, "second frame")
    hit = want["primary"]["id"] >= 0
    flags = r.is_shadowed.cpu().numpy()
    assert int((hit & (flags == 1)).sum()) >= 1 and int((hit & (flags == 0)).sum()) >= 1


@pytest.mark.parametrize("lg", LGS)
@pytest.mark.parametrize("kind", ["L1", "L2", "geometry_changed", "animate", "clone_verts", "clone_faces", "no_flag",
                                  "option_off"])
def test_every_change_builds_again(ugrt, O, torch, kind, lg):
    """Two frames (the second reused), then the change: the next frame builds (the counter stands still) and is the
    oracle's for the new light or geometry; the frame after that is reused again.  animate: ugrt_animate, then the
    frame's screen-grid build makes the triangle records valid again BEFORE the light build is asked for -- the records
    being valid says nothing about the light grid."""
    s, setup = cornell(ugrt), setup_for(ugrt)
    ctx, r = make(ugrt, lg, flags=0 if kind == "no_flag" else None)
    if kind == "option_off":
        ctx.set_option("light_reuse", 0)
    never = kind in ("no_flag", "option_off")
    frames(r, setup, 2)
    assert ctx.get_state(KEY) == (0 if never else 1)
    assert ctx.get_state(UKEY) == (0 if kind == "no_flag" else 1)  # (the other option is the uniform grid's own)
    assert_frame(ugrt, r, want_for(O, ugrt, lg), kind + ": before")
    before = ctx.get_state(KEY)
    want = want_for(O, ugrt, lg)
    if kind in ("L1", "L2"):
        setup = setup_for(ugrt, kind)
        want = want_for(O, ugrt, lg, kind)
    elif kind == "geometry_changed":
        set_verts(torch, r, _SCENE["v"]["v1"])
        want = want_for(O, ugrt, lg, tag="v1")
    elif kind == "animate":
        r.init_orig_list(8, 16)
        r.rotate_bunny(0.3)
        ctx.synchronize()
        v = r.d_verts.cpu().numpy().reshape(-1, 3).copy()
        assert np.abs(v - _SCENE["v"]["v0"]).max() > 1e-3
        r.bbmin, r.bbmax = v.min(0), v.max(0)
        want = want_for(O, ugrt, lg, tag="animated", verts=v)
        assert not np.array_equal(want["lgrid"]["vals"], want_for(O, ugrt, lg)["lgrid"]["vals"]) or \
            not np.array_equal(want["is_shadowed"], want_for(O, ugrt, lg)["is_shadowed"])
    elif kind == "clone_verts":
        r.d_verts = r.d_verts.clone()  # the same values behind a new pointer
    elif kind == "clone_faces":
        r.d_faces = r.d_faces.clone()
    frames(r, setup)
    assert ctx.get_state(KEY) == before, kind
    assert_frame(ugrt, r, want, kind + ": after")
    frames(r, setup)
    assert ctx.get_state(KEY) == (0 if never else before + 1), kind
    assert_frame(ugrt, r, want, kind + ": reused again")
    if kind in ("L1", "L2"):  # and back: the record is the last build's, not the first one's
        frames(r, setup_for(ugrt))
        assert ctx.get_state(KEY) == before + 1
        assert_frame(ugrt, r, want_for(O, ugrt, lg), kind + ": back to L0")


@pytest.mark.parametrize("lg", LGS)
def test_xm_ym_face_window_and_merged_shards_build_again(ugrt, O, torch, lg):
    """ugrt_grid_build_spherical called directly.  Another xM or yM builds again; so does a changed face window (and the
    same window is then kept); ugrt_grid_merge_shards rewrites the grid's arrays, so the build behind it builds too.
    Every grid is the oracle's for its arguments."""
    s, setup = cornell(ugrt), setup_for(ugrt)
    ctx, r = make(ugrt, lg)
    F, PI = r.F, ugrt.renderer.PI_F
    cc, lcam = light_cc(O, ugrt)
    ctx.upload_camera(lcam.camcoords)
    faces, verts = np.asarray(s["faces"], np.int32).reshape(-1), np.asarray(s["verts"], np.float32).reshape(-1)
    oracle = lambda **kw: O.grid_spherical(cc, faces, verts, lg[0], lg[1], **kw)
    build = lambda xM=PI, yM=PI: ctx.grid_build_spherical(r.d_faces, r.d_verts, F, xM, yM)
    full = oracle()
    n = 0

    def step(reused, grid, what, **kw):
        nonlocal n
        build(**kw)
        ctx.synchronize()
        n += 1 if reused else 0
        assert ctx.get_state(KEY) == n, what
        assert_grid(ugrt, ctx, grid, what)

    step(False, full, "first build")
    step(True, full, "second build")
    wide = oracle(xM=3.0)
    assert not np.array_equal(wide["span"], full["span"])
    step(False, wide, "xM 3.0", xM=3.0)
    step(True, wide, "xM 3.0 again", xM=3.0)
    tall = oracle(xM=3.0, yM=2.5)
    assert not np.array_equal(tall["span"], wide["span"])
    step(False, tall, "yM 2.5", xM=3.0, yM=2.5)
    step(False, full, "xM and yM as they were")
    half = oracle(window=(F // 3, F))
    assert not np.array_equal(half["span"], full["span"])
    ctx.set_face_window(F // 3, F)
    step(False, half, "window")
    step(True, half, "window again")
    ctx.set_face_window(0, -1)
    step(False, full, "full again")
    step(True, full, "full, kept")
    # a merge of one part (the grid itself, copied): the arrays are rewritten, the grid is no longer a build's
    value, key, span, offset, gi = ctx.grid_arrays(ugrt.GRID_SPHERICAL)
    ctx.grid_merge_shards(ugrt.GRID_SPHERICAL, [key.clone()], [value.clone()], [span.clone()], [gi.total_refs])
    ctx.synchronize()
    assert_grid(ugrt, ctx, full, "merged")
    step(False, full, "built behind the merge")
    step(True, full, "kept behind the merge")
    frames(r, setup)
    assert ctx.get_state(KEY) == n + 1
    assert_frame(ugrt, r, want_for(O, ugrt, lg), "frame on the kept grid")


@pytest.mark.parametrize("helper_thread", [True, False])
def test_two_stream_renderer(ugrt, O, torch, helper_thread):
    """overlap=True: the second context builds (and keeps) the light grid and has to hear of a change itself."""
    lg = LGS[0]
    setup = setup_for(ugrt)
    ctx, r = make(ugrt, lg, overlap=True, helper_thread=helper_thread)
    frames(r, setup, 2)
    assert r.aux.get_state(KEY) == 1 and ctx.get_state(KEY) == 0
    assert_frame(ugrt, r, want_for(O, ugrt, lg), "before")
    set_verts(torch, r, _SCENE["v"]["v1"])
    frames(r, setup)
    assert r.aux.get_state(KEY) == 1
    assert_frame(ugrt, r, want_for(O, ugrt, lg, tag="v1"), "after the change")
    frames(r, setup, 2)
    # (one host thread: the builds are asynchronous, so the build behind the change is confirmed by a waiting one first)
    assert r.aux.get_state(KEY) == (3 if helper_thread else 2)
    assert ctx.get_state(KEY) == 0
    assert_frame(ugrt, r, want_for(O, ugrt, lg, tag="v1"), "reused after the change")
    frames(r, setup_for(ugrt, "L2"))
    assert r.aux.get_state(KEY) == (3 if helper_thread else 2)
    assert_frame(ugrt, r, want_for(O, ugrt, lg, "L2", tag="v1"), "the light turned")
    r.close()


def test_two_renderers_in_flight(ugrt, O, torch):
    """Two two-stream renderers on their own streams, dealt frames in turn without a synchronisation in between;
    then the light moves on both of them."""
    lg = LGS[0]
    rs = []
    for i in range(2):
        stream = torch.cuda.Stream() if i else None
        with torch.cuda.stream(stream):
            ctx, r = make(ugrt, lg, overlap=True, helper_thread=False)
        r._stream = stream
        rs.append(r)

    def deal(n, setup):
        for k in range(2 * n):
            r = rs[k % 2]
            with torch.cuda.stream(r._stream):
                r.display(setup, shadows=True, reflect=True)
        for r in rs:
            r.synchronize()
        torch.cuda.synchronize()

    deal(3, setup_for(ugrt))  # a waiting build, then two frames on it
    for i, r in enumerate(rs):
        assert r.aux.get_state(KEY) == 2 and r.ctx.get_state(KEY) == 0, i
        assert_frame(ugrt, r, want_for(O, ugrt, lg), "renderer %d" % i)
    deal(3, setup_for(ugrt, "L1"))  # an asynchronous build, the waiting one that confirms it, one frame on that
    for i, r in enumerate(rs):
        assert r.aux.get_state(KEY) == 3, i
        assert_frame(ugrt, r, want_for(O, ugrt, lg, "L1"), "renderer %d after the light moved" % i)


@pytest.mark.parametrize("lg", LGS)
def test_async_build_is_confirmed_before_it_is_kept(ugrt, O, torch, lg):
    """async_build = 1, L0 -> L1, three frames: the first builds asynchronously, the second waits (an asynchronous
    build may have overflowed and left an emptied grid: it is never reused), the third is kept.  All three are the
    oracle's."""
    ctx, r = make(ugrt, lg)
    ctx.set_option("async_build", 1)
    frames(r, setup_for(ugrt), 3)  # the grid's first build waits (there is no estimate yet)
    assert ctx.get_state(KEY) == 2
    want = want_for(O, ugrt, lg, "L1")
    for k, reused in enumerate((2, 2, 3)):
        frames(r, setup_for(ugrt, "L1"))
        assert ctx.get_state(KEY) == reused, k
        assert_frame(ugrt, r, want, "frame %d behind the change" % k)
    frames(r, setup_for(ugrt, "L1"))
    assert ctx.get_state(KEY) == 4
    # with the option off nothing is kept and nothing waits to confirm: every call takes the asynchronous form
    ctx.set_option("light_reuse", 0)
    frames(r, setup_for(ugrt, "L1"), 3)
    assert ctx.get_state(KEY) == 4
    assert_frame(ugrt, r, want, "light_reuse 0")


def test_two_lights_taken_in_turn_build_every_time(ugrt, O, LT, torch):
    """The several-lights frame holds one light grid: with two lights every call's inputs differ from the build before
    it, so over four frames nothing is reused; the flags of each light and the image are judged as tests/test_lights.py
    judges them.  With one light the grid is kept."""
    name = "hall"
    W2, H2 = TL.SIZES[name]
    want = TL.cpu_frame(O, ugrt, name, W2, H2)
    s = want["scene"]
    ctx = ugrt.Context(W2, H2, light_grid=TL.LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS | ugrt.FLAG_STATIC_GEOMETRY, uniform_dims=TL.UD)
    r = ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    all_lights = [(lt["params"], lt["pos"]) for lt in want["lights"]]

    def check(L, what):
        r.display(TL.setup_for(ugrt, s, all_lights[:L]), frame_cnt=3, shadows=True)
        ctx.synchronize()
        for l in range(L):
            np.testing.assert_array_equal(r.shadowed_lights[l].cpu().numpy(), want["lights"][l]["flags"],
                                          err_msg="%s: light %d of %d" % (what, l, L))
        w_img, w_ids = TL.cpu_image(LT, want, L)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids)
        np.testing.assert_array_equal(r.image.cpu().numpy(), w_img, err_msg=what)

    for k in range(4):
        check(2, "frame %d" % k)
        assert ctx.get_state(KEY) == 0, k
    # one light: the first frame builds (the held grid is the other light's), then it is kept
    for k, reused in enumerate((0, 1, 2)):
        check(1, "one light, frame %d" % k)
        assert ctx.get_state(KEY) == reused, k


def test_inputs_that_differ_every_call_never_wait(ugrt, O, torch):
    """async_build = 1 and two light cameras taken in turn, as the several-lights frame takes them: no call is reused and
    none waits to confirm the build before it.  Which form a build took shows inside an open batch: an asynchronous
    build stops in front of its sort and the grid is not there before _end, a waiting build is built at once.  The same
    camera twice in a row does wait, once."""
    lg = LGS[0]
    s = cornell(ugrt)
    ctx, r = make(ugrt, lg)
    ctx.set_option("async_build", 1)
    faces, verts = np.asarray(s["faces"], np.int32).reshape(-1), np.asarray(s["verts"], np.float32).reshape(-1)
    PI = ugrt.renderer.PI_F

    def build(light, waits):
        cc, lcam = light_cc(O, ugrt, light)
        ctx.upload_camera(lcam.camcoords)
        ctx.grid_build_batch_begin()
        ctx.grid_build_spherical(r.d_faces, r.d_verts, r.F, PI, PI)
        if waits:
            ctx.grid_info(ugrt.GRID_SPHERICAL)
        else:
            with pytest.raises(ugrt.UgrtError, match="has not been built"):
                ctx.grid_info(ugrt.GRID_SPHERICAL)
        ctx.grid_build_batch_end()
        ctx.synchronize()
        assert_grid(ugrt, ctx, O.grid_spherical(cc, faces, verts, lg[0], lg[1]), light)

    build("L0", True)  # the grid's first build waits (there is no estimate yet)
    for k in range(3):
        build("L1", False)
        build("L0", False)
        assert ctx.get_state(KEY) == 0, k
    build("L0", True)  # the same inputs behind an asynchronous build: this one confirms it
    assert ctx.get_state(KEY) == 0
    build("L0", True)  # kept (nothing is built, the grid stands)
    assert ctx.get_state(KEY) == 1


def test_reused_builds_inside_a_batch(ugrt, O, torch):
    """ugrt_grid_build_batch_begin / _end: with both builds kept the batch is empty; with the light build alone kept
    (only the uniform grid's box changes) it is the uniform grid alone."""
    lg = LGS[0]
    s, setup = cornell(ugrt), setup_for(ugrt)
    ctx, r = make(ugrt, lg, overlap=True, helper_thread=False, batch_builds=True)
    want = want_for(O, ugrt, lg)
    frames(r, setup, 2)
    assert (r.aux.get_state(KEY), r.aux.get_state(UKEY)) == (1, 1)
    assert_frame(ugrt, r, want, "an empty batch")
    before = r.aux.get_state("radix_launches")
    frames(r, setup)
    assert (r.aux.get_state(KEY), r.aux.get_state(UKEY)) == (2, 2)
    assert r.aux.get_state("radix_launches") == before  # (nothing was sorted)
    assert_frame(ugrt, r, want, "another empty batch")
    r.bbmin = r.bbmin - np.float32(3.0)
    r.bbmax = r.bbmax + np.float32(5.0)
    ug = O.grid_uniform(s["faces"], s["verts"], r.bbmin, r.bbmax, UD)
    assert not np.array_equal(ug["span"], want["ugrid"]["span"])
    for k, (lr, ur) in enumerate(((3, 2), (4, 2), (5, 3))):  # the uniform grid: asynchronous, the waiting build, kept
        frames(r, setup)
        assert (r.aux.get_state(KEY), r.aux.get_state(UKEY)) == (lr, ur), k
        what = "frame %d behind the new box" % k
        assert_grid(ugrt, r.aux, want["lgrid"], what)
        value, key, span, offset, gi = r.aux.grid_arrays(ugrt.GRID_UNIFORM)
        np.testing.assert_array_equal(u32(key), ug["keys"], err_msg=what)
        np.testing.assert_array_equal(u32(value), ug["vals"], err_msg=what)
        np.testing.assert_array_equal(u32(span), ug["span"], err_msg=what)
        # the same triangles in other cells: the frame is what it was
        np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), want["is_shadowed"], err_msg=what)
        np.testing.assert_array_equal(bits(r.hit_t.cpu().numpy()), bits(want["hit_t"]), err_msg=what)
        np.testing.assert_array_equal(r.image.cpu().numpy(), want["image"], err_msg=what)
    # a light build alone inside a batch, kept: an empty batch
    cc, lcam = light_cc(O, ugrt)
    r.aux.upload_camera(lcam.camcoords)
    r.aux.grid_build_batch_begin()
    r.aux.grid_build_spherical(r.d_faces, r.d_verts, r.F, ugrt.renderer.PI_F, ugrt.renderer.PI_F)
    r.aux.grid_build_batch_end()
    r.aux.synchronize()
    assert r.aux.get_state(KEY) == 6
    assert_grid(ugrt, r.aux, want["lgrid"], "an empty batch of one")


def test_slabs_behind_a_kept_grid(ugrt, O, torch):
    """slabs = 2 on the one-stream renderer: the second frame is reused, and the shadow pass (which takes the union of a
    cell's slabs from the kept arrays) still finds the oracle's flags."""
    lg = LGS[0]
    setup = setup_for(ugrt)
    ctx, r = make(ugrt, lg, slabs=2)
    want = want_for(O, ugrt, lg, slabs=2)
    for k in range(3):
        frames(r, setup)
        assert ctx.get_state(KEY) == k
        assert_frame(ugrt, r, want, "slabs, frame %d" % k)
    assert ctx.grid_info(ugrt.GRID_SPHERICAL).num_cells == lg[0] * lg[1] * 2
    assert 0 < int(want["is_shadowed"].sum()) < W * H
