"""The edge-aware gather and the shading behind it: ugrt_filter_visibility and
ugrt_shade_area_vis against tests/area_sets_ref.c (built here with the oracle's flags), and that checker against numpy
on the cases whose answer is known: radius 0, a constant mask over a plane, two planes at 90 degrees, two parallel
planes 2 * plane_tol apart, a NaN normal.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_area_light as TA
import test_reflect_shadows as RS
from test_area_light import AR  # noqa: F401  (fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, _u32, low_bits = TA._p, TA._f32, TA._i32, TA._u32, TA.low_bits
CALLS = ("ugrt_filter_visibility", "ugrt_shade_area_vis")


class SetsRef:
    def __init__(self, lib):
        self.lib = lib

    def select(self, masks, set_w, set_h, W, H, row0=0, row1=None, fill=0):
        """masks [K, W*H] -> the word of set k(p) per pixel of the band; the other pixels keep `fill`."""
        out = np.full(W * H, fill, np.uint32)
        self.lib.sets_select(_p(_u32(masks).reshape(-1)), C.c_int(set_w), C.c_int(set_h), C.c_int(W), C.c_int(H),
                             C.c_int(row0), C.c_int(H if row1 is None else row1), _p(out))
        return out

    def filter(self, mask, S, orays, oactive, R, normal_cos, plane_tol, W, H, row0=0, row1=None, fill=0):
        vis = np.full(2 * W * H, fill, np.uint32)
        self.lib.sets_filter(_p(_u32(mask)), C.c_int(S), _p(_f32(orays)), _p(_i32(oactive)), C.c_int(R), C.c_float(normal_cos),
                             C.c_float(plane_tol), C.c_int(W), C.c_int(H), C.c_int(row0), C.c_int(H if row1 is None else row1),
                             _p(vis))
        return vis

    def shade(self, img, vis, S, p0, n):
        img = np.ascontiguousarray(img, np.uint8).copy()
        self.lib.sets_shade(_p(img), _p(_u32(vis)), C.c_int(S), C.c_int(p0), C.c_int(n))
        return img


@pytest.fixture(scope="session")
def SR(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("area_sets_ref") / "libarea_sets_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "area_sets_ref.c"), "-lm"], check=True, capture_output=True)
    return SetsRef(C.CDLL(out))


def open_of(mask, S):
    m = mask & low_bits(S)
    return np.uint32(S) - sum(((m >> np.uint32(s)) & np.uint32(1)) for s in range(S)).astype(np.uint32)


def random_masks(rng, N):
    mask = rng.randint(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    mask[::5] = 0
    mask[1::11] = 0xFFFFFFFF
    return mask


def gbuffer(W, H, seed):
    """A seeded synthetic G-buffer: the floor z = 0 on the left, a wall x = const that meets it at 90 degrees on the
    right, a second floor 0.05 above the first in a square block, a slightly tilted patch (its normal within cos 0.9 of
    the floor's, positions off the plane), some inactive pixels (six zeros), one NaN position and one NaN normal.
    Positions lie on a lattice of spacing 0.01 with a little noise."""
    rng = np.random.RandomState(seed)
    N = W * H
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    x, y = x.reshape(-1), y.reshape(-1)
    o = np.stack([0.01 * x, 0.01 * y, np.zeros(N)], 1) + rng.uniform(-1e-4, 1e-4, (N, 3))
    n = np.tile([0.0, 0.0, 1.0], (N, 1))
    wall = x >= (2 * W) // 3
    o[wall] = np.stack([np.full(wall.sum(), 0.01 * ((2 * W) // 3)), 0.01 * y[wall], 0.01 * (x[wall] - (2 * W) // 3)], 1)
    n[wall] = [-1.0, 0.0, 0.0]
    step = (x < W // 3) & (y >= H // 2)
    o[step, 2] += 0.05
    tilt = (x >= W // 3) & (x < W // 2) & (y < H // 3)
    n[tilt] = np.array([0.3, 0.0, 1.0]) / np.sqrt(1.09)
    o[tilt, 2] += 0.003 * (x[tilt] - W // 3)
    active = (rng.uniform(size=N) > 0.1).astype(np.int32)
    active[N // 2 + 3] = active[N // 2 + 4] = 1
    orays = np.concatenate([o, n], 1).astype(np.float32)
    orays[N // 2 + 3, 1] = np.nan  # a NaN position
    orays[N // 2 + 4, 4] = np.nan  # a NaN normal
    orays[active == 0] = 0.0
    return orays.reshape(-1), active


def np_filter(mask, S, orays, oactive, R, ncos, ptol, W, H, row0=0, row1=None):
    """The gather in numpy, fp32 with the spec's association."""
    row1 = H if row1 is None else row1
    o = orays.reshape(H, W, 6)[..., :3].astype(np.float32)
    n = orays.reshape(H, W, 6)[..., 3:].astype(np.float32)
    act = (oactive.reshape(H, W) != 0)
    inband = np.zeros((H, W), bool)
    inband[row0:row1] = True
    opn = open_of(mask, S).reshape(H, W)
    num, den = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    P = R
    pad = lambda a, v: np.pad(a, [(P, P), (P, P)] + [(0, 0)] * (a.ndim - 2), constant_values=v)  # noqa: E731
    oq_, nq_, aq_, pq_ = pad(o, 0), pad(n, 0), pad(act & inband, False), pad(opn, 0)
    with np.errstate(invalid="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                sl = (slice(P + dy, P + dy + H), slice(P + dx, P + dx + W))
                oq, nq, aq, pq = oq_[sl], nq_[sl], aq_[sl], pq_[sl]
                cosine = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                d = oq - o
                dist = (d[..., 0] * n[..., 0] + d[..., 1] * n[..., 1]) + d[..., 2] * n[..., 2]
                same = (cosine >= np.float32(ncos)) & (np.abs(dist) <= np.float32(ptol))
                if dx == 0 and dy == 0:
                    same = np.ones((H, W), bool)
                take = same & aq & act & inband
                w = np.uint32((R + 1 - abs(dx)) * (R + 1 - abs(dy)))
                num += np.where(take, w * pq, 0).astype(np.uint32)
                den += np.where(take, w, 0).astype(np.uint32)
    return np.stack([num, den], 2).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    for name in ("filter_visibility", "shade_area_vis"):
        assert hasattr(ugrt.Context, name), name
    assert ugrt.MAX_FILTER_RADIUS == 8


@pytest.mark.parametrize("S", [1, 5, 32])
def test_radius_0_is_the_pixel_itself_and_the_bytes_of_area_shade(SR, AR, S):
    rng = np.random.RandomState(S)
    W, H = 40, 24
    N = W * H
    orays, oactive = gbuffer(W, H, S)
    mask = random_masks(rng, N)
    vis = SR.filter(mask, S, orays, oactive, 0, 0.9, 0.01, W, H)
    act = oactive != 0
    np.testing.assert_array_equal(vis[0::2], np.where(act, open_of(mask, S), 0))
    np.testing.assert_array_equal(vis[1::2], act.astype(np.uint32))
    img = rng.randint(0, 256, 3 * N).astype(np.uint8)
    img[:30] = 255
    got = SR.shade(img, vis, S, 0, N)
    want = AR.shade(img, np.where(act, mask, 0), S, 0, N)  # (den = 0 leaves the pixel: so does a zero mask)
    np.testing.assert_array_equal(got, want)
    assert int((got != img).sum()) > 100
    # every mask word at one pixel: (b * (S + 2 lit)) // (3 S) for all b
    for m in (0, 1, low_bits(S), np.uint32(0xFFFFFFFF)):
        one = np.full(256, m, np.uint32)
        v = SR.filter(one, S, np.tile(np.float32([0, 0, 0, 0, 0, 1]), 256), np.ones(256, np.int32), 0, 0.9, 0.0, 256, 1)
        ramp = np.repeat(np.arange(256, dtype=np.uint8), 3)
        np.testing.assert_array_equal(SR.shade(ramp, v, S, 0, 256), AR.shade(ramp, one, S, 0, 256))


@pytest.mark.parametrize("R", [1, 2, 8])
def test_a_constant_mask_over_a_plane_comes_back_as_it_went_in(SR, R):
    W, H, S = 24, 20, 8  # (a full window of radius 8 fits)
    N = W * H
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    orays = np.stack([0.1 * x.reshape(-1), 0.1 * y.reshape(-1), np.full(N, 2.0), np.zeros(N), np.zeros(N), np.ones(N)],
                     1).astype(np.float32).reshape(-1)
    mask = np.full(N, 0b10110, np.uint32)  # open = 5
    vis = SR.filter(mask, S, orays, np.ones(N, np.int32), R, 0.9, 1e-6, W, H)
    np.testing.assert_array_equal(vis[0::2], 5 * vis[1::2])
    tent = np.array([[(R + 1 - abs(dx)) * (R + 1 - abs(dy)) for dx in range(-R, R + 1)] for dy in range(-R, R + 1)])
    assert int(vis[1::2].max()) == int(tent.sum()) == (R + 1) ** 4
    assert int(vis[1]) == int(tent[R:, R:].sum())  # the corner pixel: a quarter of the window
    img = np.random.RandomState(R).randint(0, 256, 3 * N).astype(np.uint8)
    np.testing.assert_array_equal(SR.shade(img, vis, S, 0, N), SR.shade(img, SR.filter(mask, S, orays, np.ones(N, np.int32), 0,
                                                                                        0.9, 1e-6, W, H), S, 0, N))
    assert vis.max() <= 32 * 6561


def test_edges_exchange_nothing(SR):
    """Two planes meeting at 90 degrees, two parallel planes 2 * plane_tol apart: left and right halves hold different
    constant masks and every pixel's share stays its own half's.  The same pair of parallel planes within plane_tol mix."""
    W, H, S, R, tol = 16, 8, 8, 2, 0.01
    N = W * H
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    x, y = x.reshape(-1), y.reshape(-1)
    left = x < W // 2
    mask = np.where(left, 0b1, 0b1111111).astype(np.uint32)  # open 7 | 1
    act = np.ones(N, np.int32)
    floor = np.stack([0.001 * x, 0.001 * y, np.zeros(N), np.zeros(N), np.zeros(N), np.ones(N)], 1)
    corner = floor.copy()
    corner[~left] = np.stack([np.full(N, 0.001 * (W // 2)), 0.001 * y, 0.001 * (x - W // 2), -np.ones(N), np.zeros(N),
                              np.zeros(N)], 1)[~left]
    apart = floor.copy()
    apart[~left, 2] = 2 * tol
    for what, g in (("corner", corner), ("apart", apart)):
        vis = SR.filter(mask, S, g.astype(np.float32).reshape(-1), act, R, 0.9, tol, W, H)
        np.testing.assert_array_equal(vis[0::2], np.where(left, 7, 1) * vis[1::2], err_msg=what)
        assert (vis[1::2] > 0).all()
    near = floor.copy()
    near[~left, 2] = 0.5 * tol
    vis = SR.filter(mask, S, near.astype(np.float32).reshape(-1), act, R, 0.9, tol, W, H)
    edge = (x == W // 2 - 1) | (x == W // 2)
    assert (vis[0::2][edge] != np.where(left, 7, 1)[edge] * vis[1::2][edge]).all()
    np.testing.assert_array_equal(vis[1::2].reshape(H, W)[R:-R, R:-R], (R + 1) ** 4)


def test_a_nan_normal_isolates_its_pixel_and_a_nan_position_too(SR):
    W, H, S, R = 12, 12, 5, 2
    N = W * H
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    orays = np.stack([0.1 * x.reshape(-1), 0.1 * y.reshape(-1), np.zeros(N), np.zeros(N), np.zeros(N), np.ones(N)],
                     1).astype(np.float32)
    mask = random_masks(np.random.RandomState(0), N)
    act = np.ones(N, np.int32)
    clean = SR.filter(mask, S, orays.reshape(-1), act, R, 0.9, 1e-3, W, H)
    for col in (5, 1):  # a NaN normal component, a NaN position component
        g = orays.copy()
        p = 6 * W + 6
        g[p, col] = np.nan
        vis = SR.filter(mask, S, g.reshape(-1), act, R, 0.9, 1e-3, W, H)
        assert (int(vis[2 * p]), int(vis[2 * p + 1])) == (int(open_of(mask, S)[p]), (R + 1) ** 2)
        # its neighbours lose exactly its contribution, everybody else keeps their sums
        for q in range(N):
            qx, qy = q % W, q // W
            dx, dy = abs(qx - 6), abs(qy - 6)
            if q != p and dx <= R and dy <= R:
                w = (R + 1 - dx) * (R + 1 - dy)
                assert int(vis[2 * q + 1]) == int(clean[2 * q + 1]) - w
                assert int(vis[2 * q]) == int(clean[2 * q]) - w * int(open_of(mask, S)[p])
            elif q != p:
                assert (vis[2 * q], vis[2 * q + 1]) == (clean[2 * q], clean[2 * q + 1])


GATHER_SIZES = [(72, 40), (8, 8), (32, 8)]  # not a multiple of the 32 x 8 workgroup tile; smaller than it; equal to it


@pytest.mark.parametrize("W,H", GATHER_SIZES)
def test_the_checker_is_the_numpy_gather_on_the_synthetic_g_buffer(SR, W, H):
    orays, oactive = gbuffer(W, H, W)
    mask = random_masks(np.random.RandomState(H), W * H)
    total = 0
    for R in (0, 1, 2, 8):
        for S in (1, 5, 32):
            vis = SR.filter(mask, S, orays, oactive, R, 0.9, 0.004, W, H)
            np.testing.assert_array_equal(vis, np_filter(mask, S, orays, oactive, R, 0.9, 0.004, W, H), err_msg="R %d S %d" % (R, S))
            total += int(vis[1::2].sum())
    if (W, H) == (72, 40):  # the G-buffer's edges do cut: fewer pairs than one plane would give, but most of them
        one = SR.filter(mask, 5, np.tile(np.float32([0, 0, 0, 0, 0, 1]), W * H), np.ones(W * H, np.int32), 2, 0.9, 0.004, W, H)
        cut = SR.filter(mask, 5, orays, oactive, 2, 0.9, 0.004, W, H)
        print("72 x 40, R = 2: sum of weights %d of %d on one plane" % (int(cut[1::2].sum()), int(one[1::2].sum())))
        assert 0.3 * int(one[1::2].sum()) < int(cut[1::2].sum()) < 0.9 * int(one[1::2].sum())
        # the band (rows 16..39): neighbours across its edge do not count, pixels outside keep their words
        band = SR.filter(mask, 5, orays, oactive, 2, 0.9, 0.004, W, H, 16, 40, fill=0xABCD)
        np.testing.assert_array_equal(band[2 * 16 * W:], np_filter(mask, 5, orays, oactive, 2, 0.9, 0.004, W, H, 16, 40)[2 * 16 * W:])
        assert (band[:2 * 16 * W] == 0xABCD).all()
        assert (band[2 * 16 * W:2 * 17 * W:2] != cut[2 * 16 * W:2 * 17 * W:2]).any()


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _gather(ctx, torch, mask, S, orays, oactive, R, ncos, ptol, fill=0xABCD):
    N = ctx.width * ctx.height
    vis = torch.full((2 * N,), fill, dtype=torch.int32, device=ctx.device)
    ctx.filter_visibility(ctx.upload(mask.view(np.int32)), S, ctx.upload(orays), ctx.upload(oactive), R, ncos, ptol, vis)
    ctx.synchronize()
    return vis.cpu().numpy().view(np.uint32), vis


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", GATHER_SIZES)
def test_gather_equals_the_checker(ugrt, SR, torch, W, H):
    """R = 0, 1, 2, 8 x S = 1, 5, 32 on the seeded G-buffer (inactive pixels, the image's borders, the edges, a NaN
    position and a NaN normal), and the shading behind it; at 72 x 40 also two band contexts, whose pixels outside keep
    their words and whose neighbours across the band's edge do not count."""
    N = W * H
    orays, oactive = gbuffer(W, H, W)
    rng = np.random.RandomState(H)
    mask = random_masks(rng, N)
    img = rng.randint(0, 256, 3 * N).astype(np.uint8)
    ctx = ugrt.Context(W, H, light_grid=(16, 16), uniform_dims=(4, 4, 4))
    for R in (0, 1, 2, 8):
        for S in (1, 5, 32):
            what = "R %d S %d" % (R, S)
            got, d_vis = _gather(ctx, torch, mask, S, orays, oactive, R, 0.9, 0.004)
            want = SR.filter(mask, S, orays, oactive, R, 0.9, 0.004, W, H)
            np.testing.assert_array_equal(got, want, err_msg=what)
            d_img = ctx.upload(img)
            ctx.shade_area_vis(d_img, d_vis, S)
            ctx.synchronize()
            np.testing.assert_array_equal(d_img.cpu().numpy(), SR.shade(img, want, S, 0, N), err_msg=what)
            if R == 0:  # ugrt_shade_area's bytes
                d_ref = ctx.upload(img)
                ctx.shade_area(d_ref, ctx.upload(np.where(oactive != 0, mask, 0).astype(np.uint32).view(np.int32)), S)
                ctx.synchronize()
                assert torch.equal(d_img, d_ref), what
    if (W, H) != (72, 40):
        return
    for rows in ((0, 2), (2, 5)):
        band = ugrt.Context(W, H, light_grid=(16, 16), uniform_dims=(4, 4, 4), rows=rows)
        r0, r1 = 8 * rows[0], 8 * rows[1]
        assert (band.p0, band.npix) == (r0 * W, (r1 - r0) * W)
        for R, S in ((2, 5), (8, 32)):
            got, d_vis = _gather(band, torch, mask, S, orays, oactive, R, 0.9, 0.004)
            np.testing.assert_array_equal(got, SR.filter(mask, S, orays, oactive, R, 0.9, 0.004, W, H, r0, r1, fill=0xABCD),
                                          err_msg="rows %r R %d" % (rows, R))
            d_img = band.upload(img)
            band.shade_area_vis(d_img, d_vis, S)
            band.synchronize()
            want = SR.shade(img, got, S, band.p0, band.npix)
            np.testing.assert_array_equal(d_img.cpu().numpy(), want)
            np.testing.assert_array_equal(want[:3 * band.p0], img[:3 * band.p0])


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing(ugrt, torch):
    W = H = 8
    ctx = ugrt.Context(W, H, light_grid=(16, 16), uniform_dims=(4, 4, 4))
    orays, oactive = gbuffer(W, H, 1)
    mask = ctx.upload(np.zeros(W * H, np.int32))
    vis = torch.full((2 * W * H,), 77, dtype=torch.int32, device=ctx.device)
    img = torch.full((3 * W * H,), 200, dtype=torch.uint8, device=ctx.device)
    args = [mask, 8, ctx.upload(orays), ctx.upload(oactive), 2, 0.9, 0.01, vis]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    for h in (0, 2, 3, 7):
        fails(ctx.filter_visibility, args[:h] + [None] + args[h + 1:], b"null")
    for bad in (0, 33, -1):
        fails(ctx.filter_visibility, args[:1] + [bad] + args[2:], b"num_bits")
    for bad in (-1, 9):
        fails(ctx.filter_visibility, args[:4] + [bad] + args[5:], b"radius")
    for bad in (-1e-9, float("nan")):
        fails(ctx.filter_visibility, args[:6] + [bad] + args[7:], b"plane_tol")
    for bad in (0, 33):
        fails(ctx.shade_area_vis, [img, vis, bad], b"num_samples")
    for h in (0, 1):
        a = [img, vis, 4]
        fails(ctx.shade_area_vis, a[:h] + [None] + a[h + 1:], b"null")
    ctx.synchronize()
    assert (vis == 77).all() and (img == 200).all()
    ctx.filter_visibility(*args)  # the context is usable; plane_tol 0 and a NaN normal_cos are arguments like any other
    ctx.filter_visibility(*(args[:5] + [float("nan"), 0.0] + args[7:]))
    ctx.synchronize()
    got = vis.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[1::2], 9 * (oactive != 0).astype(np.uint32))  # a NaN cosine bound: the pixel alone, (R + 1)^2
