"""Every frame path of renderer.py against the plain one-stream Renderer frame, bit for bit.

The paths: plain, plain with sharded grid builds (world 1: one shard, exchanged and merged), two streams with the
helper thread, two streams from one host thread (async builds, with and without batched builds), and a frame cut into
two bands.  The cases: shadows on and off; no reflection with simple (frame_cnt 1) and spotlight (frame_cnt 2)
shading; reflections at depth 1 and 3.  Each renderer runs two frames (the second is the one that uses the
asynchronous builds where a path has them), and every per-pixel array of the second frame is compared as bytes."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 256, 256
LG, UD = (64, 64), (32, 32, 16)  # as tests/test_reflect_depth.py
PIXEL_ARRAYS = ("image", "t", "normal", "dir", "is_shadowed", "intersect_id")
LEVEL_ARRAYS = ("rays", "active", "hit_t", "hit_id")

CASES = {"simple": dict(reflect=False, frame_cnt=1, bounces=1),
         "spotlight": dict(reflect=False, frame_cnt=2, bounces=1),
         "bounce1": dict(reflect=True, frame_cnt=1, bounces=1),
         "bounce3": dict(reflect=True, frame_cnt=1, bounces=3)}
PATHS = ("plain", "sharded", "overlapped", "inline", "inline_batch", "banded2")


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_SCENE = {}


def mirrors(ugrt):
    if not _SCENE:
        _SCENE["s"] = ugrt.scenes.mirrors(scale=0.1)
    s = _SCENE["s"]
    return s, ugrt.FrameSetup.from_scene(s)


def context(ugrt):
    return ugrt.Context(W, H, light_grid=LG, flags=ugrt.FLAG_SHADOW_ALL_CHUNKS, uniform_dims=UD)


def make(ugrt, torch, path):
    s, _ = mirrors(ugrt)
    args = (s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])
    if path == "banded2":
        return ugrt.BandedRenderer(ugrt.Context, W, H, *args, bands=2, light_grid=LG, uniform_dims=UD,
                                   flags=ugrt.FLAG_SHADOW_ALL_CHUNKS)
    kw = {"plain": {},
          "sharded": dict(shards=importlib.import_module(ugrt.__name__ + ".parallel").GridShards(
              None, torch, torch.device("cuda", 0), 0, 1)),
          "overlapped": dict(overlap=True),
          "inline": dict(overlap=True, helper_thread=False),
          "inline_batch": dict(overlap=True, helper_thread=False, batch_builds=True)}[path]
    return ugrt.Renderer(context(ugrt), *args, **kw)


def display(r, setup, shadows, case):
    c = CASES[case]
    r.display(setup, frame_cnt=c["frame_cnt"], shadows=shadows, reflect=c["reflect"], bounces=c["bounces"])


def outputs(r, torch, case):
    """name -> bytes of every array the case writes (the level-1 names, and with depth > 1 every level)."""
    r.synchronize()
    torch.cuda.synchronize()
    c = CASES[case]
    names = list(PIXEL_ARRAYS)
    if c["reflect"]:
        names += list(LEVEL_ARRAYS)
    out = {n: getattr(r, n).contiguous().view(torch.uint8).cpu().numpy() for n in names}
    if c["reflect"] and c["bounces"] > 1:
        for n in LEVEL_ARRAYS:
            out[n + "_levels"] = getattr(r, n + "_levels")[:c["bounces"]].contiguous().view(torch.uint8).cpu().numpy()
    return out


_REF = {}


def reference(ugrt, torch, shadows, case):
    """The plain one-stream frame, second of two; checked not to be vacuous."""
    key = (shadows, case)
    if key not in _REF:
        _, setup = mirrors(ugrt)
        r = make(ugrt, torch, "plain")
        for _ in range(2):
            display(r, setup, shadows, case)
        out = outputs(r, torch, case)
        if CASES[case]["bounces"] == 3:
            assert int(r.active_levels[2].sum()) > 0, "no active ray at level 3"
        if shadows:
            flags = np.unique(r.is_shadowed.cpu().numpy())
            assert 0 in flags and 1 in flags, "is_shadowed holds one value only: %s" % flags
        _REF[key] = out
    return _REF[key]


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for n in want:
        a, b = got[n], want[n]
        assert a.shape == b.shape, "%s: %s has %d bytes, not %d" % (what, n, a.size, b.size)
        diff = np.flatnonzero(a != b)
        assert diff.size == 0, "%s: %s differs in %d bytes, first at byte %d" % (what, n, diff.size, diff[0])


def close(r):
    if hasattr(r, "close"):
        r.close()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("path", PATHS)
def test_frame_path_equals_the_plain_frame(ugrt, torch, path, shadows, case):
    want = reference(ugrt, torch, shadows, case)
    _, setup = mirrors(ugrt)
    r = make(ugrt, torch, path)
    try:
        for _ in range(2):
            display(r, setup, shadows, case)
        assert_same(outputs(r, torch, case), want, "%s shadows=%s %s" % (path, shadows, case))
    finally:
        close(r)


@pytest.mark.parametrize("helper_thread", [True, False])
def test_unshaded_overlapped_frame_is_the_plain_frame(ugrt, torch, helper_thread):
    """shade=False on a two-stream renderer runs the one-stream frame on its main context (no image, no bounce)."""
    _, setup = mirrors(ugrt)
    rs = [make(ugrt, torch, "plain"), make(ugrt, torch, "overlapped" if helper_thread else "inline")]
    try:
        outs = []
        for r in rs:
            for _ in range(2):
                r.display(setup, shadows=True, reflect=True, shade=False)
            outs.append(outputs(r, torch, "simple"))
        assert_same(outs[1], outs[0], "shade=False")
        assert not outs[0]["image"].any()
    finally:
        close(rs[1])


def test_inline_batch_is_closed_after_a_failed_build(ugrt, torch):
    """A build that raises inside the batch of the inline two-stream frame: the exception propagates, the batch is
    closed (a further grid_build_batch_end has none to close) and the next two frames equal the plain frame."""
    want = reference(ugrt, torch, True, "bounce1")
    _, setup = mirrors(ugrt)
    r = make(ugrt, torch, "inline_batch")
    display(r, setup, True, "bounce1")
    target = r.aux
    real = target.grid_build_uniform

    def boom(*a, **k):
        target.grid_build_uniform = real  # only this frame
        raise RuntimeError("injected failure")

    target.grid_build_uniform = boom
    with pytest.raises(RuntimeError, match="injected"):
        display(r, setup, True, "bounce1")
    r.synchronize()
    with pytest.raises(ugrt.UgrtError):
        r.aux.grid_build_batch_end()
    for _ in range(2):
        display(r, setup, True, "bounce1")
    assert_same(outputs(r, torch, "bounce1"), want, "after the failed frame")
