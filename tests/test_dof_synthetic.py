"""ugrt_dof_pixels on a synthetic g-buffer of its own: 64 x 40 pixels, the whole frame and a band.

The inputs are built so that every clause of the contract decides a pixel somewhere: a lone blurred pixel at each corner,
on each border and on either side of the band's edges; a circle of confusion that equals an integer distance to the ulp,
and lies one ulp on either side of it; coc_min met to the ulp and missed by one; radius 0, 1 and 8; t that is a NaN, an
infinity, a denormal or negative; negative ids; z <= 0.  The checker is tests/dof_ref.c, and it is itself compared with a
numpy statement of the definition."""
import numpy as np
import pytest

import test_reflect_depth as RD
from test_dof import DOF, DofRef  # noqa: F401  (fixture)

W, H = 64, 40
N = W * H
ROWS = (1, 4)  # the band context's tile rows: pixel rows 8..31
LG, UD = RD.LG, RD.UD
F32 = np.float32
AXIS = F32([0.0, 0.0, 1.0])
FOCUS = 2.0
LONE = [(0, 0), (63, 0), (0, 39), (63, 39), (30, 0), (0, 20), (63, 20), (30, 39), (20, 7), (20, 8), (40, 31), (40, 32), (32, 20)]


def empty():
    """All misses."""
    return dict(t=np.full(N, -1.0, F32), dir=np.tile(F32([0, 0, 1]), N), id=np.full(N, -1, np.int32))


def lone():
    """Hits at depth 1 along the axis, where |z - F| = z = 1 and the circle is coc_scale to the bit, at LONE; misses
    elsewhere."""
    g = empty()
    for x, y in LONE:
        g["t"][y * W + x] = 1.0
        g["id"][y * W + x] = 5
    return g


def odd():
    """A row of pixels, ten apart, each blurred widely unless its own oddity forbids it."""
    g = empty()
    nan, inf = float("nan"), float("inf")
    cases = [dict(t=nan), dict(t=inf), dict(t=-inf), dict(t=1e-40), dict(t=-4.0), dict(t=0.0), dict(t=-0.0), dict(id=-1), dict(id=-2),
             dict(id=-2 ** 31), dict(dz=-1.0), dict(dz=0.0), dict(dz=nan), dict(t=4.0, id=0), dict(t=3e38), dict(dz=-0.0),
             dict(t=2.0), dict(t=np.nextafter(F32(2), F32(3)))]
    for k, c in enumerate(cases):
        p = (6 + 14 * (k // 6)) * W + 5 + 10 * (k % 6)
        g["t"][p] = c.get("t", 4.0)
        g["id"][p] = c.get("id", 7)
        g["dir"][3 * p + 2] = c.get("dz", 1.0)
    return g


def noise(seed):
    rng = np.random.RandomState(seed)
    g = dict(t=rng.uniform(-5, 40, N).astype(F32), dir=rng.normal(size=3 * N).astype(F32), id=rng.randint(-3, 50, N).astype(np.int32))
    g["t"][rng.randint(0, N, 40)] = float("nan")
    return g


def np_pixels(g, axis, focus, coc_scale, coc_min, R):
    """The definition in numpy, fp32 operation for operation: (coc [N], flags [N])."""
    with np.errstate(all="ignore"):
        t, d = g["t"], g["dir"].reshape(N, 3)
        z = t * ((d[:, 0] * axis[0] + d[:, 1] * axis[1]) + d[:, 2] * axis[2])
        ok = (t > 0) & (g["id"] >= 0) & (z > 0)
        coc = np.where(ok, (F32(coc_scale) * np.abs(z - F32(focus))) / z, F32(0)).astype(F32).reshape(H, W)
    flags = np.zeros((H, W), np.int32)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            m = F32(max(abs(dx), abs(dy)))
            with np.errstate(invalid="ignore"):
                src = (coc >= F32(coc_min)) & (coc >= m)  # q = p + (dx, dy) reaches p
            ys, xs = np.nonzero(src)
            py, px = ys - dy, xs - dx
            keep = (py >= 0) & (py < H) & (px >= 0) & (px < W)
            flags[py[keep], px[keep]] = 1
    return coc.reshape(-1), flags.reshape(-1)


def below(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def above(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def cases():
    """(name, g-buffer, coc_scale, coc_min, R).  On lone() the circle is coc_scale to the bit."""
    out = []
    g = lone()
    for R in (0, 1, 8):
        for m in (1, 2, 3, 8):
            for what, cs in (("at", float(m)), ("below", below(m)), ("above", above(m))):
                out.append(("lone m %d %s R %d" % (m, what, R), g, cs, 0.5, R))
        out.append(("lone wide R %d" % R, g, 100.0, 0.5, R))
        out.append(("lone none R %d" % R, g, 0.0, 0.5, R))
    for cmin, what in ((1.5, "met"), (above(1.5), "missed"), (below(1.5), "passed")):
        out.append(("lone coc_min %s" % what, g, 1.5, cmin, 4))
    out.append(("lone coc_min 0", g, 3.0, 0.0, 2))  # every pixel meets it: coc >= 0 at distance 0
    out.append(("lone coc_min -1", empty(), 3.0, -1.0, 2))
    out.append(("lone negative scale", g, -3.0, -10.0, 2))  # a negative circle reaches nothing, not even its own pixel
    out.append(("lone infinite scale", g, float("inf"), 0.5, 8))
    out.append(("lone infinite coc_min", g, 3.0, float("inf"), 8))
    for R in (0, 1, 8):
        out.append(("odd R %d" % R, odd(), 9.0, 0.5, R))
    for seed, cs, cmin, R in ((1, 1.0, 0.5, 4), (2, 3.0, 0.5, 8), (3, 0.7, 0.25, 1), (4, 5.0, 2.0, 0), (5, 2.0, 0.5, 7)):
        g = noise(seed)
        out.append(("noise %d" % seed, g, cs, cmin, R))
    return out


def test_the_inputs_hold_what_they_are_built_for(DOF):
    g = lone()
    for m in (1, 2, 3, 8):
        assert DOF.coc(g, AXIS, FOCUS, float(m), W, H)[LONE[-1][1] * W + LONE[-1][0]] == F32(m)
        assert DOF.coc(g, AXIS, FOCUS, below(m), W, H).max() == np.nextafter(F32(m), F32(0))
        assert DOF.coc(g, AXIS, FOCUS, above(m), W, H).max() == np.nextafter(F32(m), F32(9))
    assert DOF.coc(g, AXIS, FOCUS, 1.5, W, H).max() == F32(1.5)
    with np.errstate(all="ignore"):
        c = DOF.coc(odd(), AXIS, FOCUS, 9.0, W, H)
    assert np.isnan(c).sum() >= 1 and np.isinf(c).sum() >= 1 and int((c == F32(4.5)).sum()) == 1  # 9 * |4 - 2| / 4
    assert int((c > 0).sum()) == 4  # the plain hit, the denormal, 3e38 and the depth one ulp behind the focus; the NaN is not > 0


def test_the_checker_is_the_definition(DOF):
    flagged = 0
    for name, g, cs, cmin, R in cases():
        coc, want = np_pixels(g, AXIS, FOCUS, cs, cmin, R)
        with np.errstate(all="ignore"):
            got_coc = DOF.coc(g, AXIS, FOCUS, cs, W, H)
        np.testing.assert_array_equal(got_coc, coc, err_msg=name)  # (a NaN equals a NaN here)
        np.testing.assert_array_equal(DOF.pixels(g, AXIS, FOCUS, cs, cmin, R, W, H, 0, N), want, err_msg=name)
        p0, n = ROWS[0] * 8 * W, (ROWS[1] - ROWS[0]) * 8 * W
        band = DOF.pixels(g, AXIS, FOCUS, cs, cmin, R, W, H, p0, n, fill=-7)
        assert (band[:p0] == -7).all() and (band[p0 + n:] == -7).all(), name
        np.testing.assert_array_equal(band[p0:p0 + n], want[p0:p0 + n], err_msg=name)
        flagged += int(want.sum())
    assert flagged > 5000


def test_a_lone_circle_flags_the_square_it_reaches(DOF):
    """coc = m exactly reaches distance m, one ulp less reaches m - 1; the window caps it; the image's borders cut it."""
    g = lone()
    for m in (1, 2, 3, 8):
        for R in (0, 1, 8):
            for cs, reach in ((float(m), min(m, R)), (below(m), min(m - 1, R)), (above(m), min(m, R))):
                flags = DOF.pixels(g, AXIS, FOCUS, cs, 0.5, R, W, H, 0, N).reshape(H, W)
                want = np.zeros((H, W), np.int32)
                for x, y in LONE:
                    want[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = 1
                np.testing.assert_array_equal(flags, want, err_msg="m %d R %d scale %r" % (m, R, cs))
    # coc_min met to the ulp flags, missed by one ulp does not
    want = np.zeros((H, W), np.int32)
    for x, y in LONE:
        want[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = 1
    np.testing.assert_array_equal(DOF.pixels(g, AXIS, FOCUS, 1.5, 1.5, 4, W, H, 0, N).reshape(H, W), want)
    assert not DOF.pixels(g, AXIS, FOCUS, 1.5, above(1.5), 4, W, H, 0, N).any()


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.mark.gpu
def test_pixels_equal_the_checker(ugrt, DOF, torch):
    """Every case, on the whole frame and on a band with row_begin > 0, into sentinel-filled flags: the checker's words,
    and the sentinel outside the band."""
    whole = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD)
    band = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD, rows=ROWS)
    assert (band.p0, band.npix) == (ROWS[0] * 8 * W, (ROWS[1] - ROWS[0]) * 8 * W)
    flagged = 0
    uploaded = {}
    for name, g, cs, cmin, R in cases():
        for ctx in (whole, band):
            key = (id(g), id(ctx))
            if key not in uploaded:
                uploaded[key] = (g, ctx.upload(g["t"]), ctx.upload(g["dir"]), ctx.upload(g["id"]))
            _, t, d, ids = uploaded[key]
            flag = torch.full((N,), -7, dtype=torch.int32, device=ctx.device)
            ctx.dof_pixels(t, d, ids, AXIS, FOCUS, cs, cmin, R, flag)
            ctx.synchronize()
            want = DOF.pixels(g, AXIS, FOCUS, cs, cmin, R, W, H, ctx.p0, ctx.npix, fill=-7)
            np.testing.assert_array_equal(flag.cpu().numpy(), want, err_msg="%s, p0 %d" % (name, ctx.p0))
            flagged += int((want == 1).sum())
    assert flagged > 5000
    # an axis that is not a coordinate axis, a focus in front of everything
    g = noise(9)
    axis = F32([0.6, -0.48, 0.64])
    t, d, ids = whole.upload(g["t"]), whole.upload(g["dir"]), whole.upload(g["id"])
    for focus, cs in ((0.5, 0.05), (25.0, 0.4)):
        flag = torch.full((N,), -7, dtype=torch.int32, device=whole.device)
        whole.dof_pixels(t, d, ids, axis, focus, cs, 0.5, 5, flag)
        whole.synchronize()
        want = DOF.pixels(g, axis, focus, cs, 0.5, 5, W, H, 0, N)
        np.testing.assert_array_equal(flag.cpu().numpy(), want)
        np.testing.assert_array_equal(want, np_pixels(g, axis, focus, cs, 0.5, 5)[1])
        assert 0 < int(want.sum()) < N
