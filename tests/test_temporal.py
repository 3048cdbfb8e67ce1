"""Temporal accumulation: ugrt_temporal_visibility, ugrt_temporal_gi, scenes.temporal_sets and
Renderer.display(..., temporal=N).

The checker is tests/temporal_ref.c (built here with the oracle's flags): the rule of include/ugrt.h, one loop per pixel.
It is itself checked against numpy float32 on the cases whose answer is known.  Every GPU comparison is exact; in the
frame tests the checker is fed the device's own masks, sums and G-buffers, frame by frame."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_ambient as AM
import test_area_light as TA
import test_filter_visibility as FV
import test_indirect as TI
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
from test_ambient import AO  # noqa: F401  (fixtures)
from test_ambient_sets import ASR  # noqa: F401
from test_filter_visibility import SR  # noqa: F401
from test_indirect import IR  # noqa: F401
from test_reflect_shadows import REFS  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
_p, _f32, _i32, _u32 = TA._p, TA._f32, TA._i32, TA._u32
CALLS = ("ugrt_temporal_visibility", "ugrt_temporal_gi")
LG, UD = (16, 16), (16, 16, 8)
f32 = np.float32


class TemporalRef:
    def __init__(self, lib):
        self.lib = lib

    def project(self, cc, o, W, H):
        out = np.zeros(3, np.float32)
        self.lib.temporal_project(_p(_f32(cc)), _p(_f32(o)), C.c_int(W), C.c_int(H), _p(out))
        return out

    def blend(self, C_, cur, S, orays, oactive, prev_cc, prev_orays, prev_oactive, hist_in, max_frames, ncos, ptol, W, H,
              row0=0, row1=None, fill=0, hist_fill=-5.0):
        """(hist_out, out, taps): C_ = 1 the pair form, 3 the GI form; pixels outside the band keep the fills."""
        CW = 4 if C_ == 3 else 2
        N = W * H
        hist_out, out = np.full(CW * N, hist_fill, np.float32), np.full(CW * N, fill, np.uint32)
        taps = np.zeros(5 * N, np.int32)
        self.lib.temporal_blend(C.c_int(C_), _p(_u32(cur)), C.c_int(S), _p(_f32(orays)), _p(_i32(oactive)), _p(_f32(prev_cc)),
                                _p(_f32(prev_orays)), _p(_i32(prev_oactive)), _p(_f32(hist_in)), C.c_int(max_frames),
                                C.c_float(ncos), C.c_float(ptol), C.c_int(W), C.c_int(H), C.c_int(row0),
                                C.c_int(H if row1 is None else row1), _p(hist_out), _p(out), _p(taps))
        return hist_out, out, taps.reshape(N, 5)


@pytest.fixture(scope="session")
def TR(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("temporal_ref") / "libtemporal_ref.so")
    subprocess.run(RS.GCC + ["-o", out, os.path.join(HERE, "temporal_ref.c"), "-lm"], check=True, capture_output=True)
    return TemporalRef(C.CDLL(out))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def synthetic_cam(W, H, scale=1.0, shift=(0.0, 0.0), kz=0.0, pitch=0.01):
    """A camera block whose vertex transform sends the world point (pitch * x, pitch * y, z) to the image position
    ((scale * x + shift_x) / w, ...), w = 1 + kz * z: the modelview is the identity, the projection is written out
    (column-major, m[4 * column + row], as dd_camcoords holds them)."""
    cc = np.zeros(64, np.float32)
    for k in range(4):
        cc[16 + 5 * k] = 1.0
    P = np.zeros((4, 4), np.float64)
    # ndc = 2 * f / size - w  ->  (ndc / w + 1) / 2 * size = f / w
    P[0, 0], P[0, 3], P[0, 2] = 2.0 * scale / (pitch * W), 2.0 * shift[0] / W - 1.0, -kz
    P[1, 1], P[1, 3], P[1, 2] = 2.0 * scale / (pitch * H), 2.0 * shift[1] / H - 1.0, -kz
    P[2, 2] = 1.0
    P[3, 2], P[3, 3] = kz, 1.0
    cc[32:48] = P.T.reshape(-1).astype(np.float32)
    return cc


def plane_buffer(W, H, z=0.0):
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    N = W * H
    g = np.stack([0.01 * x.reshape(-1), 0.01 * y.reshape(-1), np.full(N, z), np.zeros(N), np.zeros(N), np.ones(N)], 1)
    return g.astype(np.float32).reshape(-1), np.ones(N, np.int32)


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
        assert len(ugrt.PROTOTYPES[name][1]) == 14
    for name in ("temporal_visibility", "temporal_gi"):
        assert hasattr(ugrt.Context, name), name
    assert (ugrt.MAX_TEMPORAL_FRAMES, ugrt.TEMPORAL_DEN) == (64, 256)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ugrt.h")).read()
    assert "#define UGRT_MAX_TEMPORAL_FRAMES 64" in header and "#define UGRT_TEMPORAL_DEN 256u" in header
    assert "temporal accumulation, DESIGN.md section 6.12" in header
    assert hasattr(ugrt.Renderer, "temporal_reset") and hasattr(ugrt.scenes, "temporal_sets")


def test_temporal_sets_cover_all_16_sets_over_16_frames(ugrt):
    S = 4
    t16 = ugrt.scenes.ao_direction_sets(S, 16)
    for sets in (1, 4, 16):
        seen = [set() for _ in range(sets)]
        for f in range(16):
            t = ugrt.scenes.temporal_sets(t16, sets, f)
            assert t.shape == (sets, S, 3) and t.dtype == np.float32 and t.flags["C_CONTIGUOUS"]
            picks = [(k * (16 // sets) + f) % 16 for k in range(sets)]
            assert len(set(picks)) == sets  # the entries of a tile hold different sets in every frame
            for k in range(sets):
                np.testing.assert_array_equal(bits(t[k]), bits(t16[picks[k]]))
                seen[k].add(picks[k])
        assert all(s == set(range(16)) for s in seen), sets
        np.testing.assert_array_equal(bits(ugrt.scenes.temporal_sets(t16, sets, 16)), bits(ugrt.scenes.temporal_sets(t16, sets, 0)))
    a16 = ugrt.scenes.area_sample_sets(5, 16, (1.0, 2.0, 3.0), (0.0, 0.0, -1.0), 0.5)
    np.testing.assert_array_equal(bits(ugrt.scenes.temporal_sets(a16, 4, 3)), bits(a16[[3, 7, 11, 15]]))
    for bad in (0, 2, 8, None):
        with pytest.raises(ValueError):
            ugrt.scenes.temporal_sets(t16, bad, 0)
    with pytest.raises(ValueError):
        ugrt.scenes.temporal_sets(t16[:4], 4, 0)


def test_the_checker_under_an_unchanged_camera_reads_the_pixel_s_own_history(TR):
    W, H, S, N_MAX = 24, 16, 8, 64
    N = W * H
    rng = np.random.RandomState(1)
    orays, oactive = plane_buffer(W, H)
    cc = synthetic_cam(W, H)
    den = rng.randint(1, 6562, N).astype(np.uint32)
    num = (rng.uniform(size=N) * S * den).astype(np.uint32)
    cur = np.stack([num, den], 1).reshape(-1)
    hist = np.stack([rng.uniform(size=N).astype(np.float32), rng.randint(1, 70, N).astype(np.float32)], 1)
    ho, out, taps = TR.blend(1, cur, S, orays, oactive, cc, orays, oactive, hist.reshape(-1), N_MAX, 0.9, 1e-4, W, H)
    x, y = np.arange(N) % W, np.arange(N) // W
    np.testing.assert_array_equal(taps[:, 0], x)
    np.testing.assert_array_equal(taps[:, 1], y)
    assert not taps[:, 2:4].any() and (taps[:, 4] == 1).all()
    c = num.astype(np.float32) / (np.uint32(S) * den).astype(np.float32)
    n = np.minimum(hist[:, 1] + f32(1), f32(N_MAX))
    hp = (f32(256) * hist[:, 0]) / f32(256)
    h = hp + (c - hp) / n
    np.testing.assert_array_equal(bits(ho[0::2]), bits(h))
    np.testing.assert_array_equal(bits(ho[1::2]), bits(n))
    np.testing.assert_array_equal(out[1::2], 256)
    want = np.minimum(np.floor(h * f32(S * 256) + f32(0.5)).astype(np.int64), S * 256)
    np.testing.assert_array_equal(out[0::2], want)
    assert n.max() == N_MAX and n.min() == 2  # the cap holds, and a count of 1 gives 2
    # max_frames = 1 gives back the quantised input
    ho, out, _ = TR.blend(1, cur, S, orays, oactive, cc, orays, oactive, hist.reshape(-1), 1, 0.9, 1e-4, W, H)
    np.testing.assert_array_equal(bits(ho[0::2]), bits(c))
    np.testing.assert_array_equal(ho[1::2], 1)
    np.testing.assert_array_equal(out[0::2], np.floor(c * f32(S * 256) + f32(0.5)).astype(np.int64))


def test_the_checker_keeps_a_constant_and_the_running_mean_of_n_frames(TR):
    W, H, S = 24, 16, 4
    N = W * H
    orays, oactive = plane_buffer(W, H)
    # a constant input over a constant history stays what it is, under a camera that moves by fractions of a pixel too
    cur = np.tile(np.uint32([3 * 5, 5]), N)  # c = 3/4
    hist = np.tile(f32([0.75, 7.0]), N)
    for cc in (synthetic_cam(W, H), synthetic_cam(W, H, 1.0625, (0.3, -0.7))):
        ho, out, taps = TR.blend(1, cur, S, orays, oactive, cc, orays, oactive, hist, 16, 0.9, 1e-4, W, H)
        had = taps[:, 4] != 0
        assert had.sum() > N // 2
        np.testing.assert_array_equal(ho[0::2], 0.75)
        np.testing.assert_array_equal(ho[1::2], np.where(had, 8, 1))
        np.testing.assert_array_equal(out[0::2], 3 * 256)
    # n <= max_frames frames under a standing camera: the running mean, in numpy float32 in the same order
    rng = np.random.RandomState(2)
    cc = synthetic_cam(W, H)
    hist = np.zeros(2 * N, np.float32)
    mean = np.zeros(N, np.float32)
    for f in range(1, 9):
        den = rng.randint(1, 50, N).astype(np.uint32)
        num = (rng.uniform(size=N) * S * den).astype(np.uint32)
        c = num.astype(np.float32) / (np.uint32(S) * den).astype(np.float32)
        hist, out, _ = TR.blend(1, np.stack([num, den], 1).reshape(-1), S, orays, oactive, cc, orays, oactive, hist, 8, 0.9, 1e-4,
                                W, H)
        mean = c if f == 1 else mean + (c - mean) / f32(f)
        np.testing.assert_array_equal(bits(hist[0::2]), bits(mean), err_msg="frame %d" % f)
        np.testing.assert_array_equal(hist[1::2], f)
    # a ninth and a tenth frame: the count stays at the cap
    for f in (9, 10):
        hist, _, _ = TR.blend(1, np.stack([num, den], 1).reshape(-1), S, orays, oactive, cc, orays, oactive, hist, 8, 0.9, 1e-4, W, H)
        np.testing.assert_array_equal(hist[1::2], 8)


def test_the_checker_restarts_a_pixel_whose_surface_changed(TR):
    W, H, S = 16, 8, 4
    N = W * H
    orays, oactive = plane_buffer(W, H)
    cc = synthetic_cam(W, H)
    cur = np.tile(np.uint32([2, 1]), N)  # c = 1/2
    hist = np.tile(f32([0.25, 5.0]), N)
    changed = {"normal": 3 * W + 4, "plane": 3 * W + 6, "inactive before": 3 * W + 8, "count 0": 3 * W + 10, "NaN share": 5 * W + 2,
               "share above 1": 5 * W + 4, "behind the eye": 5 * W + 6}
    now, prev, pact, h = orays.copy().reshape(N, 6), orays.copy().reshape(N, 6), oactive.copy(), hist.copy().reshape(N, 2)
    now[changed["normal"], 3:] = [1.0, 0.0, 0.0]
    prev[changed["plane"], 2] = 0.5
    pact[changed["inactive before"]] = 0
    h[changed["count 0"], 1] = 0.0
    h[changed["NaN share"], 0] = np.nan
    h[changed["share above 1"], 0] = 1.0000001
    cam = synthetic_cam(W, H, kz=-2.0)
    now[changed["behind the eye"], 2] = 1.0  # w = 1 - 2 * 1 < 0 under `cam`; the others lie at z = 0, w = 1
    prev[changed["behind the eye"], 2] = 1.0
    ho, out, taps = TR.blend(1, cur, S, now.reshape(-1), oactive, cam, prev.reshape(-1), pact, h.reshape(-1), 16, 0.9, 1e-4, W, H)
    restart = np.zeros(N, bool)
    restart[list(changed.values())] = True
    np.testing.assert_array_equal(ho[1::2], np.where(restart, 1, 6))
    np.testing.assert_array_equal(ho[0::2][restart], 0.5)
    np.testing.assert_array_equal(bits(ho[0::2][~restart]), bits(np.full(N - len(changed), f32(0.25) + (f32(0.5) - f32(0.25)) / f32(6))))
    assert (taps[changed["behind the eye"], :4] == -9).all() and (taps[changed["normal"], :4] != -9).all()
    assert TR.project(cam, now[changed["behind the eye"], :3], W, H)[2] < 0
    # the band: a tap in a row outside it does not count, pixels outside keep their words
    ho, out, _ = TR.blend(1, cur, S, orays, oactive, synthetic_cam(W, H, 1.0, (0.0, 0.5)), orays, oactive, hist, 16, 0.9, 1e-4, W, H, 2, 6,
                          fill=0xABCD)
    assert (out[:2 * 2 * W] == 0xABCD).all() and (out[2 * 6 * W:] == 0xABCD).all() and (ho[:2 * 2 * W] == -5.0).all()
    np.testing.assert_array_equal(ho[1::2][2 * W:6 * W], 6)  # rows 2..4 blend rows y, y + 1; row 5 its own alone


# -- the synthetic case of the GPU test (a): built and examined here, on the CPU

A_W, A_H = 48, 40
A_BAND = (1, 4)  # tile rows: image rows 8..31


def case_a(S, max_frames, gi):
    """Seeded inputs of both exports at 48 x 40: test_filter_visibility.gbuffer's shapes for this frame and, with another
    seed, for the frame before; a previous camera that scales by 17/16 and shifts by (-0.7, -0.7) with a little
    perspective along z; one point behind that eye; stored shares with NaNs and values outside [0, 1]; stored counts
    0, 1, max_frames - 1, max_frames."""
    W, H = A_W, A_H
    N = W * H
    rng = np.random.RandomState(1000 * S + 10 * max_frames + int(gi))
    orays, oactive = FV.gbuffer(W, H, 6)  # (seeds with which every one of the 256 fractions meets a pixel: coverage_a)
    prev_orays, prev_oactive = FV.gbuffer(W, H, 106)
    orays, oactive = orays.copy(), oactive.copy()
    behind = 20 * W + 7
    orays[6 * behind:6 * behind + 6] = [0.07, 0.2, 0.75, 0.0, 0.0, 1.0]  # w = 1 - 2 * 0.75 < 0
    oactive[behind] = 1
    prev_orays = prev_orays.copy()
    prev_orays[6 * (10 * W + 10) + 4] = np.nan  # a NaN normal in the frame before (gbuffer's own NaNs sit at N/2 + 3, + 4)
    prev_orays[6 * (11 * W + 12) + 0] = np.nan  # and a NaN position
    cc = synthetic_cam(W, H, 1.0625, (-0.7, -0.7), kz=-2.0)
    CW, C_ = (4, 3) if gi else (2, 1)
    den = rng.randint(1, 6562, N).astype(np.uint32)
    den[::37] = 0  # active pixels without a pair among them
    scale = (255 if gi else 1) * S
    cur = np.zeros((N, CW), np.uint32)
    for k in range(C_):
        cur[:, k] = (rng.uniform(size=N) * scale * den).astype(np.uint32)
    cur[:, CW - 1] = den
    hist = np.zeros((N, CW), np.float32)
    hist[:, :C_] = rng.uniform(size=(N, C_)).astype(np.float32)
    hist[::29, 0] = np.nan
    hist[5::31, C_ - 1] = 1.5
    hist[7::41, 0] = -0.25
    hist[3::43, :C_] = [1.0, 0.0, 1.0][:C_]
    hist[:, CW - 1] = rng.choice(np.float32([0, 1, max_frames - 1, max_frames]), N)
    hist[11::53, CW - 1] = np.nan
    return dict(W=W, H=H, N=N, S=S, C=C_, CW=CW, cur=cur.reshape(-1), orays=orays, oactive=oactive, cc=cc, prev_orays=prev_orays,
                prev_oactive=prev_oactive, hist=hist.reshape(-1), max_frames=max_frames, cos=0.9, tol=0.004, behind=behind)


def run_a(TR, a, rows=None, fill=0xABCD):
    r0, r1 = (0, a["H"]) if rows is None else (8 * rows[0], 8 * rows[1])
    return TR.blend(a["C"], a["cur"], a["S"], a["orays"], a["oactive"], a["cc"], a["prev_orays"], a["prev_oactive"], a["hist"],
                    a["max_frames"], a["cos"], a["tol"], a["W"], a["H"], r0, r1, fill=fill)


def coverage_a(a, taps, hist_out):
    """What the case must hold, from the checker's own record."""
    W, H, CW = a["W"], a["H"], a["CW"]
    inside = taps[:, 0] != -9
    fractions = set(map(tuple, taps[inside][:, 2:4]))
    assert len(fractions) == 256, len(fractions)
    counted = taps[:, 4] != 0
    assert len(set(map(tuple, taps[counted][:, 2:4]))) == 256  # ... with a tap that counted
    ix, iy = taps[inside, 0], taps[inside, 1]
    assert (ix == -1).any() and (ix == W - 1).any() and (iy == -1).any() and (iy == H - 1).any()  # taps off every edge
    active = (a["oactive"] != 0) & (a["cur"].reshape(-1, CW)[:, CW - 1] != 0)
    assert (active & ~inside).sum() >= 10 and (taps[a["behind"], :4] == -9).all() and active[a["behind"]]
    n = hist_out.reshape(-1, CW)[:, CW - 1]
    assert set(np.unique(n[active])) >= {1.0, min(2.0, a["max_frames"]), float(a["max_frames"])}
    assert (inside & active & ~counted).sum() >= 50  # positions whose four taps were all dropped
    for m in range(1, 16):
        assert (taps[:, 4] == m).any() or m in (6, 9), m  # every subset of the four taps (the diagonals may be missing)


@pytest.mark.parametrize("gi", [False, True])
def test_case_a_covers_what_it_claims(TR, gi):
    a = case_a(3, 64, gi)
    ho, out, taps = run_a(TR, a)
    coverage_a(a, taps, ho)
    assert np.isnan(a["orays"]).sum() == 2 and np.isnan(a["prev_orays"]).sum() == 4 and np.isnan(a["hist"]).any()
    # in the band a tap above row 8 or below row 31 is dropped: pixels near its edges differ from the whole frame's
    hb, ob, tb = run_a(TR, a, A_BAND)
    CW, W = a["CW"], a["W"]
    sl = slice(CW * 8 * W, CW * 32 * W)
    assert (ob[:sl.start] == 0xABCD).all() and (ob[sl.stop:] == 0xABCD).all()
    assert (bits(hb[sl]) != bits(ho[sl])).any()
    rows = tb[8 * W:32 * W]  # taps in row 7, above the band, and in row 32, below it, beside taps inside that counted
    assert ((rows[:, 1] == 7) & (rows[:, 4] != 0)).any() and ((rows[:, 1] == 31) & (rows[:, 3] != 0) & (rows[:, 4] != 0)).any()
    inner = (np.arange(a["N"]) // W >= 8) & (np.arange(a["N"]) // W < 32) & ((taps[:, 0] == -9) | ((taps[:, 1] >= 8) & (taps[:, 1] < 31)))
    assert inner.sum() > 500  # the pixels of the band whose taps all lie in its rows: the whole frame's values
    np.testing.assert_array_equal(bits(hb.reshape(-1, CW)[inner]), bits(ho.reshape(-1, CW)[inner]))


# -- display on the recording context


def _fake(ugrt):
    r = TI._fake(ugrt)
    r.__dict__.update(ao_vis="aovis", area_vis="avis", gi_acc="giacc", ao_tvis="aotvis", area_tvis="atvis", gi_tacc="gitacc",
                      prev_ao_rays="prev_aorays", prev_ao_active="prev_aoact", _temporal={}, _temporal_set_tables={},
                      _temporal_prev_cam=None, _temporal_live=False, _temporal_serial=0, cleared=[])
    r._ensure_temporal_gbuffers = lambda: None
    r._temporal_words = lambda name, words: None
    r._temporal_alloc = lambda words: ["hist%d_a" % words, "hist%d_b" % words]
    r._temporal_clear = lambda st: (r.cleared.append(st["hist"][st["turn"]]), st.__setitem__("n", 0))
    r._ensure_area_filter_buffers = lambda: None
    r._ensure_ao_filter_buffers = lambda: None
    r._ensure_gi_buffers = lambda gather: None
    r._upload_ao_sets = lambda table: ("table", table)
    return r


def test_temporal_is_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    for bad in (1, -1, 65, 2.0, True, "8", None):
        with pytest.raises(ValueError):
            rmod.check_temporal(bad, 0.9, None, True)
    for bad in (float("nan"), "0.9", None, True):
        with pytest.raises(ValueError):
            rmod.check_temporal(8, bad, None, True)
    for bad in (-1e-9, float("nan"), "1", True):
        with pytest.raises(ValueError):
            rmod.check_temporal(8, 0.9, bad, True)
    for kw in (dict(effects=False), dict(effects=True, lights=[1]), dict(effects=True, reflect_lights=True),
               dict(effects=True, two_streams=True)):
        with pytest.raises(ValueError):
            rmod.check_temporal(8, 0.9, None, **kw)
    with pytest.raises(ValueError):
        rmod.check_temporal(0, 0.5, None)
    with pytest.raises(ValueError):
        rmod.check_temporal(0, 0.9, 0.1)
    assert rmod.check_temporal(0) is None and rmod.check_temporal(0, 0.9, None, False, [1], True, True) is None
    assert rmod.check_temporal(2, 0.5, 0.25, True) == (2, 0.5, 0.25) and rmod.check_temporal(np.int64(64), 1, None, True) == (64, 1.0, None)
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    for kw in (dict(temporal=8), dict(temporal=1, ao=4, ao_radius=1.0), dict(temporal=65, ao=4, ao_radius=1.0),
               dict(temporal=8, ao=4, ao_radius=1.0, temporal_plane=-1.0), dict(temporal=0, temporal_cos=0.5, ao=4, ao_radius=1.0)):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(setup, **kw)
        assert r.ctx.calls == [] and r.cleared == []
    r = _fake(ugrt)
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s, TL.lights_for(s, 2)), temporal=8, ao=4, ao_radius=1.0)
    with pytest.raises(ValueError):
        r.display(TL.setup_for(ugrt, s, TL.lights_for(s, 2)), temporal=8, ao=4, ao_radius=1.0, reflect=True, reflect_lights=True)
    assert r.ctx.calls == []
    r = _fake(ugrt)
    r.aux = object()  # a two-stream renderer
    with pytest.raises(ValueError):
        r.display(setup, temporal=8, ao=4, ao_radius=1.0)
    assert r.ctx.calls == []
    br = object.__new__(ugrt.BandedRenderer)
    with pytest.raises(ValueError):
        br.display(setup, temporal=8)


CAMERA_PASS, HARD = TA.CAMERA_PASS, TA.HARD
_names = TA._names


def _call(r, name, k=0):
    return [c for c in r.ctx.calls if c[0] == name][k]


def test_a_temporal_frame_enqueues_gather_blend_shade_per_effect_and_temporal_0_nothing_new(ugrt):
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    every = dict(ao=4, ao_radius=1.0, area=5, area_radius=0.5, gi=3)
    # temporal = 0: the calls of the frame that never heard of the keyword
    for kw in (dict(), dict(ao=4, ao_radius=1.0, ao_sets=16, ao_filter=2), every, dict(reflect=True, bounces=2, **every)):
        a, b = _fake(ugrt), _fake(ugrt)
        a.display(setup, **kw)
        b.display(setup, temporal=0, **kw)
        assert _names(a) == _names(b) and not [n for n in _names(b) if n.startswith("temporal")] and b.cleared == []
    r = _fake(ugrt)
    r.display(setup, temporal=8, temporal_cos=0.8, temporal_plane=0.02, **every)
    want = CAMERA_PASS + ["grid_build_uniform", "ao_rays", "trace_dda_any_area_sets", "trace_dda_any_hemi_sets", "gi_gather",
                          "shade_simple", "filter_visibility", "temporal_visibility", "shade_area_vis", "gi_filter", "temporal_gi",
                          "gi_apply", "filter_visibility", "temporal_visibility", "shade_ao_vis"]
    assert _names(r) == want, _names(r)
    # the G-buffers changed places before the frame's rays were written: ao_rays names this frame's
    assert (r.ao_rays, r.prev_ao_rays, r.ao_active, r.prev_ao_active) == ("prev_aorays", "aorays", "prev_aoact", "aoact")
    assert _call(r, "ao_rays")[-2:] == ("prev_aorays", "prev_aoact")
    cam = RLT._rmod(ugrt).make_camera(setup.camera, setup.fovy, 1.0).camcoords
    plane = float(np.float32(0.02))
    for k, (sums, S, hist_in, hist_out, out) in enumerate((("avis", 5, "hist2_a", "hist2_b", "atvis"), ("aovis", 4, "hist2_a", "hist2_b", "aotvis"))):
        c = _call(r, "temporal_visibility", k)
        assert c[1:5] == (sums, S, "prev_aorays", "prev_aoact") and c[6:9] == ("aorays", "aoact", hist_in), c
        np.testing.assert_array_equal(bits(c[5]), bits(cam))  # the first frame: its own eye (the histories are empty)
        assert c[9:] == (8, float(np.float32(0.8)), plane, hist_out, out)
    c = _call(r, "temporal_gi")
    assert c[1:5] == ("giacc", 3, "prev_aorays", "prev_aoact") and c[8:] == ("hist4_a", 8, float(np.float32(0.8)), plane, "hist4_b", "gitacc")
    # without *_filter the gathers run at radius 0; without *_sets the walks over sets get a 1 x 1 tile and frame 0's table
    assert _call(r, "filter_visibility", 0)[1:6] == ("amask", 5, "prev_aorays", "prev_aoact", 0)
    assert _call(r, "filter_visibility", 1)[1:6] == ("aomask", 4, "prev_aorays", "prev_aoact", 0)
    assert _call(r, "gi_filter")[4] == 0
    assert _call(r, "shade_ao_vis")[1:] == ("img", "aotvis", 4) and _call(r, "shade_area_vis")[1:] == ("img", "atvis", 5)
    assert _call(r, "gi_apply")[1:4] == ("img", "gitacc", 3)
    walk = _call(r, "trace_dda_any_hemi_sets")
    assert walk[8:11] == (4, 1, 1) and walk[11][0] == "table"
    t16 = ugrt.scenes.ao_direction_sets(4, 16)
    np.testing.assert_array_equal(bits(walk[11][1]), bits(ugrt.scenes.temporal_sets(t16, 1, 0)))
    # the second frame under a moved camera: the tables of frame 1, the histories the other way round, the first frame's eye
    moved = ugrt.FrameSetup(dict(setup.camera, eye=tuple(np.float64(setup.camera["eye"]) + 0.01)), setup.light_camera, setup.shading_light)
    r.ctx.calls.clear()
    r.display(moved, temporal=8, temporal_cos=0.8, temporal_plane=0.02, **every)
    assert _names(r) == want and r.cleared == []
    assert (r.ao_rays, r.prev_ao_rays) == ("aorays", "prev_aorays")
    c = _call(r, "temporal_visibility", 1)
    np.testing.assert_array_equal(bits(c[5]), bits(cam))
    assert c[3:5] == ("aorays", "aoact") and c[6:9] == ("prev_aorays", "prev_aoact", "hist2_b") and c[12] == "hist2_a"
    np.testing.assert_array_equal(bits(_call(r, "trace_dda_any_hemi_sets")[11][1]), bits(ugrt.scenes.temporal_sets(t16, 1, 1)))
    assert len(r._temporal_set_tables) == 3 and all(len(v) == 16 for v in r._temporal_set_tables.values())
    assert [r._temporal[k]["n"] for k in ("ao", "area", "gi")] == [2, 2, 2]
    # what starts a mean again: an effect's parameters (that effect alone), the light (area and gi), temporal = 0 in between,
    # the geometry, temporal_reset; a camera change did not
    r.display(moved, temporal=8, temporal_cos=0.8, temporal_plane=0.02, **dict(every, ao_radius=2.0))
    assert [r._temporal[k]["n"] for k in ("ao", "area", "gi")] == [1, 3, 3] and len(r.cleared) == 1
    lit = ugrt.FrameSetup(moved.camera, dict(setup.light_camera, eye=tuple(np.float64(setup.light_camera["eye"]) + 0.5)), setup.shading_light)
    r.display(lit, temporal=8, temporal_cos=0.8, temporal_plane=0.02, **dict(every, ao_radius=2.0))
    assert [r._temporal[k]["n"] for k in ("ao", "area", "gi")] == [2, 1, 1] and len(r.cleared) == 3
    r.display(lit, **dict(every, ao_radius=2.0))
    r.display(lit, temporal=8, temporal_cos=0.8, temporal_plane=0.02, **dict(every, ao_radius=2.0))
    assert [r._temporal[k]["n"] for k in ("ao", "area", "gi")] == [1, 1, 1] and len(r.cleared) == 6
    np.testing.assert_array_equal(bits(_call(r, "temporal_gi", -1)[5]), bits(RLT._rmod(ugrt).make_camera(lit.camera, lit.fovy, 1.0).camcoords))
    r.temporal_reset()
    assert len(r.cleared) == 9 and [r._temporal[k]["n"] for k in ("ao", "area", "gi")] == [0, 0, 0]
    r.display(lit, temporal=8, temporal_cos=0.8, temporal_plane=0.02, ao=4, ao_radius=2.0)  # area and gi sit a frame out
    r.display(lit, temporal=8, temporal_cos=0.8, temporal_plane=0.02, **dict(every, ao_radius=2.0))
    assert [r._temporal[k]["n"] for k in ("ao", "area", "gi")] == [2, 1, 1]
    r.orig, r.orig_size, r.orig_offset = "orig", 4, 0
    r.rotate_bunny(0.1)
    assert [r._temporal[k]["n"] for k in ("ao", "area", "gi")] == [0, 0, 0]
    r.display(lit, temporal=8, temporal_cos=0.8, temporal_plane=0.02, **dict(every, ao_radius=2.0))
    r.geometry_changed()
    assert [r._temporal[k]["n"] for k in ("ao", "area", "gi")] == [0, 0, 0] and "geometry_changed" in _names(r)
    # a renderer that never rendered a temporal frame: rotate_bunny enqueues what it did
    old = _fake(ugrt)
    old.orig, old.orig_size, old.orig_offset = "orig", 4, 0
    old.rotate_bunny(0.1)
    assert _names(old) == ["animate"] and old.cleared == []


def hall_buffers(ugrt, O, AO, W, H):
    """The oracle's primary hits of hall at W x H and ao_rays' {o, n} of them."""
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    fr = O.frame(s, setup, W, H, light_grid=LG)
    pr = fr["primary"]
    cam = RLT._rmod(ugrt).make_camera(setup.camera, setup.fovy, float(np.float32(W) / np.float32(H)))
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    orays, oactive = AO.rays(cam.worldori[:3].copy(), pr["t"], pr["dir"], pr["id"], verts, faces, 1e-3, 0, W * H, W * H)
    return s, setup, cam, orays, oactive


def test_a_hit_point_reprojects_onto_its_own_pixel_under_its_own_camera(ugrt, O, AO, TR):
    """The binning's mapping ((ndc + 1) / 2) * size, unflipped, sends the hit point of pixel (col, row) to (col, row): on
    hall 64 x 64 every hit pixel gets ix = col, iy = row, ax = ay = 0 and its own history alone."""
    W = H = 64
    N = W * H
    s, setup, cam, orays, oactive = hall_buffers(ugrt, O, AO, W, H)
    assert int(oactive.sum()) == N
    worst = 0.0
    for p in range(0, N, 7):
        f = TR.project(cam.camcoords, orays[6 * p:6 * p + 3], W, H)
        worst = max(worst, abs(float(f[0]) - p % W), abs(float(f[1]) - p // W))
        assert f[2] > 0
    print("largest distance of a reprojected hit point from its pixel: %.5f pixels" % worst)
    assert worst < 1.0 / 64  # (a 32nd of a pixel would reach the next sixteenth)
    cur = np.tile(np.uint32([1, 1]), N)
    hist = np.stack([np.linspace(0, 1, N).astype(np.float32), np.full(N, 3, np.float32)], 1).reshape(-1)
    ho, out, taps = TR.blend(1, cur, 4, orays, oactive, cam.camcoords, orays, oactive, hist, 8, 0.9, 0.28, W, H)
    np.testing.assert_array_equal(taps[:, 0], np.arange(N) % W)
    np.testing.assert_array_equal(taps[:, 1], np.arange(N) // W)
    assert not taps[:, 2:4].any() and (taps[:, 4] == 1).all()
    np.testing.assert_array_equal(ho[1::2], 4)


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _device_a(ctx, torch, a, hist_fill=-5.0, fill=0xABCD):
    CW, N = a["CW"], a["N"]
    hist_out = torch.full((CW * N,), hist_fill, dtype=torch.float32, device=ctx.device)
    out = torch.full((CW * N,), fill, dtype=torch.int32, device=ctx.device)
    call = ctx.temporal_gi if a["C"] == 3 else ctx.temporal_visibility
    args = [ctx.upload(a["cur"].view(np.int32)), a["S"], ctx.upload(a["orays"]), ctx.upload(a["oactive"]), a["cc"],
            ctx.upload(a["prev_orays"]), ctx.upload(a["prev_oactive"]), ctx.upload(a["hist"]), a["max_frames"], a["cos"], a["tol"],
            hist_out, out]
    call(*args)
    ctx.synchronize()
    return hist_out.cpu().numpy(), _words(out), call, args


@pytest.mark.gpu
@pytest.mark.parametrize("gi", [False, True])
def test_both_exports_equal_the_checker_on_synthetic_g_buffers(ugrt, TR, torch, gi):
    """(a) 48 x 40 (one and a half tiles wide, five high), S = 1, 3, 32 x max_frames = 1, 2, 64, on the whole frame and on
    the band of rows 8..31 with sentinel-filled outputs."""
    whole = ugrt.Context(A_W, A_H, light_grid=LG, uniform_dims=(4, 4, 4))
    band = ugrt.Context(A_W, A_H, light_grid=LG, uniform_dims=(4, 4, 4), rows=A_BAND)
    for S in (1, 3, 32):
        for max_frames in (1, 2, 64):
            a = case_a(S, max_frames, gi)
            for ctx, rows in ((whole, None), (band, A_BAND)):
                what = "S %d max_frames %d rows %r" % (S, max_frames, rows)
                want_h, want_o, taps = run_a(TR, a, rows)
                if rows is None and max_frames == 64:
                    coverage_a(a, taps, want_h)
                got_h, got_o, _, _ = _device_a(ctx, torch, a)
                np.testing.assert_array_equal(got_o, want_o, err_msg=what)
                np.testing.assert_array_equal(bits(got_h), bits(want_h), err_msg=what)
                if rows is not None:
                    CW, W = a["CW"], a["W"]
                    assert (got_o[:CW * 8 * W] == 0xABCD).all() and (got_o[CW * 32 * W:] == 0xABCD).all()
                    assert (got_h[:CW * 8 * W] == -5.0).all() and (got_h[CW * 32 * W:] == -5.0).all()
                if max_frames == 1:  # the quantised input
                    CW = a["CW"]
                    act = (want_o.reshape(-1, CW)[:, CW - 1] == 256)
                    assert (got_h.reshape(-1, CW)[act, CW - 1] == 1).all()


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing(ugrt, torch):
    """(f)"""
    ctx = ugrt.Context(A_W, A_H, light_grid=LG, uniform_dims=(4, 4, 4))
    for gi in (False, True):
        a = case_a(3, 8, gi)
        _, _, call, args = _device_a(ctx, torch, a)
        args[11].fill_(-5.0)
        args[12].fill_(0xABCD)

        def fails(a_, word):
            with pytest.raises(ugrt.UgrtError) as e:
                call(*a_)
            assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

        def swap(h, v):
            return args[:h] + [v] + args[h + 1:]

        for h in (0, 2, 3, 4, 5, 6, 7, 11, 12):
            fails(swap(h, None), b"null")
        for bad in (0, 33, -1):
            fails(swap(1, bad), b"num_dirs" if gi else b"num_bits")
        for bad in (0, 65, -1):
            fails(swap(8, bad), b"max_frames")
        fails(swap(9, float("nan")), b"normal_cos")
        for bad in (-1e-9, float("nan")):
            fails(swap(10, bad), b"plane_tol")
        fails(swap(11, args[7]), b"d_hist_in")
        fails(swap(12, args[0]), b"d_acc_out" if gi else b"d_vis_out")
        if gi:
            for h in (0, 7, 11, 12):
                fails(swap(h, args[h][1:]), b"aligned")
        ctx.synchronize()
        assert (args[11] == -5.0).all() and (_words(args[12]) == 0xABCD).all()
        call(*args)  # the context is usable
        ctx.synchronize()
        assert not (_words(args[12]) == 0xABCD).any()


# -- frames

FRAMES = {"ao": dict(ao=4, ao_sets=16, ao_filter=1), "area": dict(area=4, area_sets=16, area_filter=1),
          "gi": dict(gi=4, gi_sets=16, gi_filter=1)}
SIZES = {"hall": (64, 64), "crash": (64, 40)}


def _renderer(ugrt, s, W, H):
    ctx = ugrt.Context(W, H, light_grid=LG, uniform_dims=UD)
    return ctx, ugrt.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"])


def _radii(s):
    return dict(ao_radius=float(np.float32(0.05 * TA.extent(s))), area_radius=float(np.float32(0.10 * TA.extent(s))))


def _keywords(s, kind):
    r = _radii(s)
    return dict(FRAMES[kind], **({"ao_radius": r["ao_radius"]} if kind == "ao" else {"area_radius": r["area_radius"]} if kind == "area" else {}))


def _moved(ugrt, setup, f, step):
    eye = tuple(np.float64(setup.camera["eye"]) + f * np.float64(step))
    return ugrt.FrameSetup(dict(setup.camera, eye=eye), setup.light_camera, setup.shading_light)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "crash"])
@pytest.mark.parametrize("kind", ["ao", "area", "gi"])
def test_six_frames_under_a_moving_camera_equal_the_checker(ugrt, TR, SR, ASR, IR, torch, name, kind):
    """(b) per frame the checker gets the device's masks / sums and G-buffers and must give the gather's sums, the history,
    the output pairs and the image (the image of the same frame without the effect, rendered beside, with the effect's
    integer shading of the pair on top)."""
    W, H = SIZES[name]
    N = W * H
    s = RD.scene(ugrt, name)
    setup0 = TL.setup_for(ugrt, s)
    ctx, r = _renderer(ugrt, s, W, H)
    bctx, base = _renderer(ugrt, s, W, H)
    kw = _keywords(s, kind)
    plane = RLT._rmod(ugrt).default_filter_plane(r.bbmin, r.bbmax)
    step = np.float64([0.004, -0.003, 0.002]) * TA.extent(s)
    S, CW, C_ = 4, (4 if kind == "gi" else 2), (3 if kind == "gi" else 1)
    hist = np.zeros(CW * N, np.float32)
    prev_orays, prev_oactive, prev_cc = np.zeros(6 * N, np.float32), np.zeros(N, np.int32), None
    dropped = []
    for f in range(6):
        setup = _moved(ugrt, setup0, f, step)
        r.display(setup, temporal=8, **kw)
        base.display(setup, shadows=kind != "area")
        ctx.synchronize()
        bctx.synchronize()
        cc = RLT._rmod(ugrt).make_camera(setup.camera, setup.fovy, r.aspect).camcoords
        orays, oactive = r.ao_rays.cpu().numpy(), r.ao_active.cpu().numpy()
        if kind == "gi":
            sums = IR.filter(_words(r.gi_sum), orays, oactive, 1, 0.9, plane, W, 0, H)
            np.testing.assert_array_equal(_words(r.gi_acc), sums)
        else:
            mask = _words(r.ao_mask if kind == "ao" else r.area_mask)
            sums = SR.filter(mask, S, orays, oactive, 1, 0.9, plane, W, H)
            np.testing.assert_array_equal(_words(r.ao_vis if kind == "ao" else r.area_vis), sums)
        hist, out, taps = TR.blend(C_, sums, S, orays, oactive, cc if prev_cc is None else prev_cc, prev_orays, prev_oactive, hist, 8,
                                   0.9, plane, W, H)
        what = "%s %s frame %d" % (name, kind, f)
        np.testing.assert_array_equal(bits(r.temporal_history(kind).cpu().numpy()), bits(hist), err_msg=what)
        np.testing.assert_array_equal(_words({"ao": r.ao_tvis, "area": r.area_tvis, "gi": r.gi_tacc}[kind]), out, err_msg=what)
        img = base.image.cpu().numpy()
        if kind == "ao":
            want = ASR.shade(img, out, S, 0, N)
        elif kind == "area":
            want = SR.shade(img, out, S, 0, N)
        else:
            want = IR.apply(img, out, S, 1.0, base.intersect_id.cpu().numpy(), s["mat_list"], 0, N)
        np.testing.assert_array_equal(r.image.cpu().numpy(), want, err_msg=what)
        active = oactive != 0
        n = hist.reshape(-1, CW)[:, CW - 1]
        if f:
            dropped.append(float((n[active] == 1).mean()))
            assert (taps[active][:, 2:4] != 0).any()  # the camera did move: fractional taps
        prev_orays, prev_oactive, prev_cc = orays, oactive, cc
    print("%s %s: share of hit pixels whose history was dropped, frames 2..6: %s; frames at the end: max %d"
          % (name, kind, ["%.3f" % d for d in dropped], int(n.max())))
    assert n.max() == 6 and max(dropped) < 0.5  # most pixels kept their history all the way


_QUALITY = {}


def standing_frames(ugrt, torch):
    """Eight frames of display(ao=4, ao_sets=16, ao_filter=1, temporal=8) on hall 64 x 64 under a standing camera: per
    frame the gather's share and the history.  Rendered once, shared by (c) and (d): nobody writes to it."""
    if _QUALITY:
        return _QUALITY
    W = H = 64
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    ctx, r = _renderer(ugrt, s, W, H)
    kw = _keywords(s, "ao")
    shares, hists = [], []
    for f in range(8):
        r.display(setup, temporal=8, **kw)
        ctx.synchronize()
        vis = _words(r.ao_vis)
        with np.errstate(invalid="ignore", divide="ignore"):
            shares.append(vis[0::2].astype(np.float32) / (np.uint32(4) * vis[1::2]).astype(np.float32))
        hists.append(r.temporal_history("ao").cpu().numpy())
    _QUALITY.update(s=s, setup=setup, aspect=r.aspect, kw=kw, shares=shares, hists=hists, orays=r.ao_rays.cpu().numpy(),
                    oactive=r.ao_active.cpu().numpy(), W=W, H=H)  # (host arrays only: the context ends here)
    return _QUALITY


@pytest.mark.gpu
def test_a_standing_camera_accumulates_the_running_mean_of_the_frames(ugrt, TR, torch):
    """(c) every hit pixel reprojects onto itself (ax = ay = 0, checked with the checker on the device's G-buffer), so the
    share after f frames is the float32 running mean of the f per-frame shares and the count is f."""
    q = standing_frames(ugrt, torch)
    W, H = q["W"], q["H"]
    N = W * H
    active = q["oactive"] != 0
    assert active.sum() > 0.9 * N
    cc = RLT._rmod(ugrt).make_camera(q["setup"].camera, q["setup"].fovy, q["aspect"]).camcoords
    _, _, taps = TR.blend(1, np.tile(np.uint32([1, 1]), N), 4, q["orays"], q["oactive"], cc, q["orays"], q["oactive"],
                          np.tile(f32([0.5, 1.0]), N), 8, 0.9, 0.28, W, H)
    np.testing.assert_array_equal(taps[active, 0], (np.arange(N) % W)[active])
    np.testing.assert_array_equal(taps[active, 1], (np.arange(N) // W)[active])
    assert not taps[active, 2:4].any() and (taps[active, 4] == 1).all()
    mean = None
    for f in range(1, 9):
        c = q["shares"][f - 1]
        mean = c if f == 1 else mean + (c - mean) / f32(f)
        h = q["hists"][f - 1]
        np.testing.assert_array_equal(bits(h[0::2][active]), bits(mean[active]), err_msg="frame %d" % f)
        np.testing.assert_array_equal(h[1::2][active], f)
        assert not h.reshape(-1, 2)[~active].any()
    assert len({bits(c[active]).tobytes() for c in q["shares"]}) == 8  # eight different sample sets


@pytest.mark.gpu
def test_eight_frames_lie_closer_to_512_directions_than_one(ugrt, O, REFS, AO, torch):
    """(d) the mean absolute error of the open share against the mask of 16 x 32 directions (the CPU walk on the device's
    origins) over the hit pixels: after 8 frames strictly below the first frame's."""
    q = standing_frames(ugrt, torch)
    W, H, s = q["W"], q["H"], q["s"]
    N = W * H
    base = RS.cpu_frame(O, REFS, ugrt, "hall", W, H, 1)
    verts, faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
    table = ugrt.scenes.ao_direction_sets(32, 16)
    dark = np.zeros(N, np.float64)
    for k in range(16):
        m = AM.cpu_mask(REFS[1], AO, base["ugrid"], verts, faces, q["orays"], q["oactive"], table[k], q["kw"]["ao_radius"], 0, N, N)
        dark += sum(((m >> np.uint32(b)) & 1) for b in range(32))
    truth = 1.0 - dark / 512.0
    active = q["oactive"] != 0
    err = [float(np.abs(h[0::2][active].astype(np.float64) - truth[active]).mean()) for h in q["hists"]]
    print("hall 64 x 64, ao=4, ao_sets=16, ao_filter=1: mean absolute error of the open share after 1..8 frames %s; ratio 8 : 1 = %.3f"
          % (["%.4f" % e for e in err], err[7] / err[0]))
    assert 0.02 < truth[active].mean() < 0.98 and err[0] > 0
    assert err[7] < err[0]


@pytest.mark.gpu
def test_temporal_0_is_the_frame_as_it_was_and_every_reset_gives_frame_1(ugrt, torch):
    """(e)"""
    W = H = 64
    s = RD.scene(ugrt, "hall")
    setup = TL.setup_for(ugrt, s)
    every = dict(ao=4, ao_sets=16, ao_filter=1, area=4, area_sets=4, gi=4, gi_filter=1, **_radii(s))
    ca, a = _renderer(ugrt, s, W, H)
    cb, b = _renderer(ugrt, s, W, H)
    for c in (ca, cb):
        c.prof_enable(True)
    for _ in range(2):
        a.display(setup, **every)
        b.display(setup, temporal=0, **every)
    ca.synchronize()
    cb.synchronize()
    pa, pb = ca.prof_get(), cb.prof_get()
    assert {k: v[1] for k, v in pa.items()} == {k: v[1] for k, v in pb.items()} and pa["shade"][1] > 0
    assert torch.equal(a.image, b.image)
    assert b._temporal == {} and b.prev_ao_rays is None and b.ao_tvis is None
    for c in (ca, cb):
        c.prof_enable(False)

    def state(r):
        r.ctx.synchronize()
        return [x.cpu().numpy().copy() for x in (r.image, r.temporal_history("ao"), r.temporal_history("area"),
                                                 r.temporal_history("gi"), r.ao_tvis, r.area_tvis, r.gi_tacc)]

    def frames(r, kind):
        r.ctx.synchronize()
        h = r.temporal_history(kind).cpu().numpy().reshape(W * H, -1)[:, -1]
        return set(np.unique(h[r.ao_active.cpu().numpy() != 0]))

    kinds = ("ao", "area", "gi")
    b.display(setup, temporal=8, **every)
    first = state(b)
    assert all(frames(b, k) == {1.0} for k in kinds)
    b.display(setup, temporal=8, **every)
    b.display(_moved(ugrt, setup, 1, [0.05, 0.0, 0.0]), temporal=8, **every)
    assert all(max(frames(b, k)) == 3.0 for k in kinds)  # a camera change does not reset
    b.temporal_reset()
    b.display(setup, temporal=8, **every)
    for got, want in zip(state(b), first):
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))
    b.display(setup, temporal=8, **every)
    assert all(frames(b, k) == {2.0} for k in kinds)
    b.display(setup, temporal=8, **dict(every, ao_filter=2))  # an effect's parameters: that effect alone
    assert [frames(b, k) for k in kinds] == [{1.0}, {3.0}, {3.0}]
    lit = ugrt.FrameSetup(setup.camera, dict(setup.light_camera, eye=tuple(np.float64(setup.light_camera["eye"]) + 0.5)), setup.shading_light)
    b.display(lit, temporal=8, **dict(every, ao_filter=2))  # the light: area (and gi, whose hits it shades)
    assert [frames(b, k) for k in kinds] == [{2.0}, {1.0}, {1.0}]
    b.display(setup, **every)  # the keyword was 0 in the frame before
    b.display(setup, temporal=8, **every)
    for got, want in zip(state(b), first):
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))
    b.display(setup, temporal=8, **every)
    b.geometry_changed()
    b.display(setup, temporal=8, **every)
    assert all(frames(b, k) == {1.0} for k in kinds)
    b.display(setup, temporal=8, **every)
    b.init_orig_list(8, 16)
    b.rotate_bunny(0.0)
    b.display(setup, temporal=8, **every)
    assert all(frames(b, k) == {1.0} for k in kinds)
