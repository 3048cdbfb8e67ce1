"""Interleaved sample sets: ugrt_trace_dda_any_area_sets, its _thru form, scenes.area_sample_sets
and Renderer.display(..., area_sets=, area_filter=, area_filter_cos=, area_filter_plane=).

The walk has no restatement of its own: the expected words are test_area_light.cpu_mask once per set (oc_trace_any on
the explicit rays), selected per pixel by sets_select of tests/area_sets_ref.c; the gather and the shading behind the
frames are that file's (tests/test_filter_visibility.py checks it).  The frames underneath are those of
tests/test_area_light.py."""
import ctypes as C

import numpy as np
import pytest

import test_ambient as AM
import test_area_light as TA
import test_lights as TL
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_reflect_shadows as RS
import test_refract as RFR
from test_ambient import AO  # noqa: F401  (fixtures)
from test_area_light import AR  # noqa: F401
from test_filter_visibility import SR, open_of  # noqa: F401
from test_reflect_shadows import REFS, SYN  # noqa: F401
from test_refract import RF  # noqa: F401

bits, scene, SIZES = RD.bits, RD.scene, RD.SIZES
CALLS = ("ugrt_trace_dda_any_area_sets", "ugrt_trace_dda_any_area_sets_thru")
BAYER = [0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5]
S_SETS, SETS, R_FRAME = 8, 16, 2  # the frames: area=8, area_sets=16, area_filter=2
DEPTH = TA.DEPTH
SYN_N = TA.SYN_N


# ---------------------------------------------------------------------------------------------------------------- CPU


def test_library_prototypes_and_context_name_the_calls(ugrt):
    lib = C.CDLL(ugrt.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in ugrt.PROTOTYPES, name
    for name in ("trace_dda_any_area_sets", "trace_dda_any_area_sets_thru"):
        assert hasattr(ugrt.Context, name), name
    assert (ugrt.MAX_AREA_SET_TILE, ugrt.MAX_AREA_SET_POINTS) == (4, 512)
    assert ugrt.lib.ugrt_version() == 105


@pytest.mark.parametrize("axis", TA.AXES)
def test_area_sample_sets(ugrt, axis):
    centre, radius = np.float64([1.5, -2.0, 3.25]), 0.75
    assert ugrt.scenes.AREA_SET_RANK == {1: (0,), 4: (0, 2, 3, 1), 16: tuple(BAYER)}
    a = np.float64(axis) / np.linalg.norm(np.float64(axis))
    for S in (1, 4, 8, 32):
        for sets in (1, 4, 16):
            pos = ugrt.scenes.area_sample_sets(S, sets, centre, axis, radius)
            assert pos.dtype == np.float32 and pos.shape == (sets, S, 3)
            np.testing.assert_array_equal(bits(pos[0]), bits(ugrt.scenes.area_samples(S, centre, axis, radius)))
            rel = pos.astype(np.float64) - centre
            assert (np.abs(rel @ a) <= 1e-5 * radius).all()
            r = np.sqrt((rel * rel).sum(2))
            np.testing.assert_allclose(r, np.tile(radius * np.sqrt((np.arange(S) + 0.5) / S), (sets, 1)), rtol=0, atol=1e-5 * radius)
            for j in range(sets):
                for k in range(j):
                    assert np.abs(pos[j] - pos[k]).max() > 1e-3 * radius, (S, sets, j, k)
            # set k is set 0 turned by 2 pi rank[k] / sets about the axis (B = a x T: counter-clockwise seen along -a)
            rank = ugrt.scenes.AREA_SET_RANK[sets]
            for k in range(sets):
                phi = 2.0 * np.pi * rank[k] / sets
                turned = rel[0] * np.cos(phi) + np.cross(a, rel[0]) * np.sin(phi)
                np.testing.assert_allclose(rel[k], turned, rtol=0, atol=1e-6)
    for bad in (0, 2, 3, 8, 17, None):
        with pytest.raises(ValueError):
            ugrt.scenes.area_sample_sets(4, bad, centre, axis, radius)


def _fake(ugrt):
    r = TA._fake_frame_renderer(ugrt)
    r.__dict__.update(area_vis="avis", _area_set_tables={})
    r._ensure_area_filter_buffers = lambda: None
    r._upload_area_sets = lambda table: ("table", table)
    return r


def test_the_new_keywords_are_checked_before_anything_runs(ugrt):
    rmod = RLT._rmod(ugrt)
    chk = rmod.check_area_filter
    assert chk(0) == (1, 0, None, None) and chk(8) == (1, 0, None, None)
    assert chk(8, 16, 2, 0.9, None) == (16, 2, float(np.float32(0.9)), None)
    assert chk(8, np.int64(4), np.int32(8), 1, 0) == (4, 8, 1.0, 0.0)
    assert chk(8, 1, 0, "junk", "junk") == (1, 0, None, None)  # (not looked at without a gather)
    for bad in (0, 2, 3, 8, 17, 16.0, True, "4", None):
        with pytest.raises(ValueError):
            chk(8, bad)
    for bad in (-1, 9, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            chk(8, 1, bad)
    for bad in (None, "x", True, float("nan")):
        with pytest.raises(ValueError):
            chk(8, 1, 2, bad)
    for bad in (-1e-9, float("nan"), "x", True):
        with pytest.raises(ValueError):
            chk(8, 1, 2, 0.9, bad)
    for kw in (dict(area_sets=4), dict(area_filter=1), dict(area_sets=16, area_filter=2)):
        with pytest.raises(ValueError):
            chk(0, **kw)
    s = scene(ugrt, "hall")
    area = dict(area=8, area_radius=1.0)
    for kw in (dict(area_sets=16), dict(area_filter=2), dict(area_sets=3, **area), dict(area_filter=9, **area),
               dict(area_filter=2, area_filter_plane=-1.0, **area), dict(area_filter=2, area_filter_cos=None, **area),
               dict(area_sets=16, area=8), dict(area_sets=16, shadows=False, **area)):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(TL.setup_for(ugrt, s), **kw)
        assert r.ctx.calls == [], kw
    for kw in (dict(area_sets=16, **area), dict(area_filter=2, **area)):
        r = _fake(ugrt)
        with pytest.raises(ValueError):
            r.display(TL.setup_for(ugrt, s, TL.lights_for(s, 2)), **kw)
        assert r.ctx.calls == []
        r = _fake(ugrt)
        r.aux = object()  # a two-stream renderer
        with pytest.raises(ValueError):
            r.display(TL.setup_for(ugrt, s), **kw)
        assert r.ctx.calls == []
        br = object.__new__(ugrt.BandedRenderer)
        with pytest.raises(ValueError):
            br.display(TL.setup_for(ugrt, s), **kw)
    for kw in (dict(area_sets=16), dict(area_filter=2)):  # without area, too
        br = object.__new__(ugrt.BandedRenderer)
        with pytest.raises(ValueError):
            br.display(TL.setup_for(ugrt, s), **kw)


def _plain(c):
    return c[:1] + tuple(x for x in c[1:] if isinstance(x, (str, int, float)))


def test_recorded_call_lists(ugrt):
    """With the defaults every frame is call for call what it was (the four frame kinds of test_area_light, with and
    without area); area_sets=16 swaps only the walk; area_filter=2 swaps only shade_area for the two new calls."""
    s = RFR.scene(ugrt, "glass")
    setup = ugrt.FrameSetup.from_scene(s)
    reflect = dict(reflect=True, bounces=DEPTH, reflect_shadows=True)
    kinds = (dict(), dict(ao=4, ao_radius=1.0), reflect, dict(shade=False), dict(refract=True, **reflect))
    defaults = dict(area_sets=1, area_filter=0, area_filter_cos=0.9, area_filter_plane=None)
    hard = {0: TA.CAMERA_PASS + TA.HARD + ["shade_simple", "shade_add_shadows"],
            1: TA.CAMERA_PASS + TA.HARD + ["grid_build_uniform", "ao_rays", "trace_dda_any_hemi", "shade_simple",
                                           "shade_add_shadows", "shade_ao"],
            2: TA.CAMERA_PASS + TA.HARD + ["reflect_rays", "grid_build_uniform"] + TA.LEVELS
            + ["shade_reflect_depth_occluded", "shade_add_shadows"],
            3: TA.CAMERA_PASS + TA.HARD}
    for j, kw in enumerate(kinds):
        for area in (dict(), dict(area=5, area_radius=0.5)):
            a, b = _fake(ugrt), _fake(ugrt)
            a.display(setup, **area, **kw)
            b.display(setup, **area, **defaults, **kw)
            assert [_plain(c) for c in a.ctx.calls] == [_plain(c) for c in b.ctx.calls], (kw, area)
            if not area and j in hard:
                assert TA._names(a) == hard[j], kw
            assert not {"trace_dda_any_area_sets", "trace_dda_any_area_sets_thru", "filter_visibility", "shade_area_vis"} \
                & set(TA._names(a))
    eye = np.asarray(setup.light_camera["eye"], np.float64)
    axis = np.asarray(setup.light_camera["look"], np.float64) - eye
    for kw in kinds:
        base, sets, filt, both = _fake(ugrt), _fake(ugrt), _fake(ugrt), _fake(ugrt)
        base.display(setup, area=8, area_radius=0.5, **kw)
        sets.display(setup, area=8, area_radius=0.5, area_sets=16, **kw)
        filt.display(setup, area=8, area_radius=0.5, area_filter=2, **kw)
        both.display(setup, area=8, area_radius=0.5, area_sets=16, area_filter=2, area_filter_cos=0.5, area_filter_plane=0.25, **kw)
        if not kw.get("shade", True):
            assert TA._names(sets) == TA._names(filt) == TA._names(both) == TA._names(base) == TA.CAMERA_PASS
            continue
        old = "trace_dda_any_area_thru" if kw.get("refract") else "trace_dda_any_area"
        new = old.replace("_area", "_area_sets")
        # area_sets: the walk alone
        assert TA._names(sets) == [new if n == old else n for n in TA._names(base)]
        for cb, cs in zip(base.ctx.calls, sets.ctx.calls):
            if cb[0] != old:
                assert _plain(cb) == _plain(cs)
                continue
            assert cs[1:8] == cb[1:8] == ("value", "span", "offset", "v", "f", "aorays", "aoact")
            assert cs[8:11] == (8, 4, 4) and cs[11][0] == "table" and cs[12] == "amask"
            np.testing.assert_array_equal(bits(cs[11][1]), bits(ugrt.scenes.area_sample_sets(8, 16, eye, axis, 0.5)))
            assert cs[13:] == cb[10:] == (("mi", "tr", 3) if kw.get("refract") else ())
        # area_filter: shade_area alone
        at = TA._names(base).index("shade_area")
        want = TA._names(base)[:at] + ["filter_visibility", "shade_area_vis"] + TA._names(base)[at + 1:]
        assert TA._names(filt) == want
        assert [_plain(c) for c in filt.ctx.calls[:at]] == [_plain(c) for c in base.ctx.calls[:at]]
        assert [_plain(c) for c in filt.ctx.calls[at + 2:]] == [_plain(c) for c in base.ctx.calls[at + 1:]]
        plane = float(np.float32(0.01))  # (the fake's box is the unit cube)
        assert filt.ctx.calls[at] == ("filter_visibility", "amask", 8, "aorays", "aoact", 2, float(np.float32(0.9)), plane, "avis")
        assert filt.ctx.calls[at + 1] == ("shade_area_vis", "img", "avis", 8)
        # both
        assert TA._names(both) == [new if n == old else n for n in want]
        assert both.ctx.calls[at] == ("filter_visibility", "amask", 8, "aorays", "aoact", 2, 0.5, 0.25, "avis")
    # the table is uploaded once per (S, sets, radius, light)
    r, uploads = _fake(ugrt), []
    r._upload_area_sets = lambda table: uploads.append(table) or len(uploads)
    for kw in (dict(area=8, area_sets=16), dict(area=8, area_sets=16), dict(area=8, area_sets=4), dict(area=4, area_sets=16),
               dict(area=8, area_sets=16), dict(area=8, area_sets=16, area_radius=0.25)):
        r.display(setup, **dict(dict(area_radius=0.5), **kw))
    assert [u.shape for u in uploads] == [(16, 8, 3), (4, 8, 3), (16, 4, 3), (16, 8, 3)]
    walks = [c for c in r.ctx.calls if c[0] == "trace_dda_any_area_sets"]
    assert [w[11] for w in walks] == [1, 1, 2, 3, 1, 4]


_SETS = {}


def cpu_sets(O, REFS, AO, AR, SR, ugrt, name, RF=None, S=S_SETS, sets=SETS, share=None):
    """The CPU side of a frame with interleaved sets: test_area_light.cpu_area's origins and radius, the table of
    scenes.area_sample_sets, the mask of every set ("per_set" [sets, N]: the see-through walk on glass) and the
    per-pixel selection ("mask").  share: the radius as a share of the scene's largest extent instead of cpu_area's.
    Computed once per key and shared: nobody writes to it."""
    key = (name, S, sets, share)
    if key in _SETS:
        return _SETS[key]
    a = TA.cpu_area(O, REFS, AO, AR, ugrt, name, RF)
    s, N, W, H = a["scene"], a["N"], a["W"], a["H"]
    verts, faces = TA._f32(s["verts"]).reshape(-1), TA._i32(s["faces"]).reshape(-1)
    lc = ugrt.FrameSetup.from_scene(s).light_camera
    eye = np.asarray(lc["eye"], np.float64)
    radius = a["radius"] if share is None else float(np.float32(share * TA.extent(s)))
    table = ugrt.scenes.area_sample_sets(S, sets, eye, np.asarray(lc["look"], np.float64) - eye, radius)
    grid = a["base"]["thru"] if name == "glass" else a["base"]["ugrid"]
    per_set = np.stack([TA.cpu_mask(REFS[1], AR, grid, verts, faces, a["orays"], a["oactive"], table[k], 0, N, N)
                        for k in range(sets)])
    tile = {1: (1, 1), 4: (2, 2), 16: (4, 4)}[sets]
    out = dict(a=a, table=table, per_set=per_set, tile=tile, mask=SR.select(per_set, tile[0], tile[1], W, H), radius=radius)
    _SETS[key] = out
    return out


def share(per_set, S):
    """The lit share of a pixel over all of per_set's samples."""
    return sum(open_of(m, S).astype(np.float64) for m in per_set) / (S * len(per_set))


def _errors(O, REFS, AO, AR, SR, ugrt, name, part=None):
    rmod = RLT._rmod(ugrt)
    c = cpu_sets(O, REFS, AO, AR, SR, ugrt, name, share=part)
    a = c["a"]
    W, H = a["W"], a["H"]
    truth = share(cpu_sets(O, REFS, AO, AR, SR, ugrt, name, S=32, share=part)["per_set"], 32)  # 16 turns x 32 samples
    hit = a["oactive"] != 0
    pen = hit & (truth > 0) & (truth < 1)
    v = TA._f32(a["scene"]["verts"]).reshape(-1, 3)
    plane = rmod.default_filter_plane(v.min(0), v.max(0))
    assert plane == float(np.float32(0.01 * TA.extent(a["scene"])))
    out = {}
    for what, mask, R in (("fixed", c["per_set"][0], 0), ("interleaved", c["mask"], 0), ("interleaved, gather", c["mask"], R_FRAME),
                          ("fixed, gather", c["per_set"][0], R_FRAME)):
        vis = SR.filter(mask, S_SETS, a["orays"], a["oactive"], R, 0.9, plane, W, H).astype(np.float64)
        out[what] = float(np.abs(vis[0::2][pen] / (S_SETS * vis[1::2][pen]) - truth[pen]).mean())
    return c, int(pen.sum()), out


def test_interleaved_sets_with_the_gather_halve_the_error_on_crash(ugrt, O, REFS, AO, AR, SR):
    """crash 256 x 144, radius 10 % of the extent (2.8), S = 8, 16 sets: every set index is used by at least 1000 hit
    pixels, the fixed and the interleaved masks differ on at least 1000 pixels, and the mean absolute error of the lit
    share over the penumbra of the 16 x 32-sample truth is, for interleaved sets with the gather of radius 2, below half
    of that of the fixed 8 samples unfiltered (measured: 0.0253 against 0.0703, a ratio of 0.36, DESIGN.md section 6.8;
    the cap of 0.5 leaves room for rounding differences of the sets)."""
    c, npen, err = _errors(O, REFS, AO, AR, SR, ugrt, "crash")
    a = c["a"]
    W, H = a["W"], a["H"]
    assert (W, H) == (256, 144) and abs(a["radius"] - 2.8) < 0.05
    hit = (a["oactive"] != 0).reshape(H, W)
    used = [int(hit[j // 4::4, j % 4::4].sum()) for j in range(16)]
    differ = int((c["mask"] != c["per_set"][0]).sum())
    print("crash: %d penumbra pixels; hit pixels per set %s; fixed and interleaved masks differ on %d pixels; errors %s; ratio %.3f"
          % (npen, used, differ, {k: round(v, 4) for k, v in err.items()}, err["interleaved, gather"] / err["fixed"]))
    assert min(used) >= 1000, used
    assert differ >= 1000
    assert not c["mask"][a["oactive"] == 0].any() and not (c["mask"] >> np.uint32(S_SETS)).any()
    assert err["interleaved, gather"] < 0.5 * err["fixed"], err


def test_the_halls_figures_are_printed_where_the_gather_loses(ugrt, O, REFS, AO, AR, SR):
    """hall 256 x 256 at 10 % and at 2 % of the extent: the penumbra is narrow against the gather there; the figures are
    those of DESIGN.md section 6.8 and nothing is claimed of them but that they are errors of a share."""
    for part, least in ((None, 1000), (0.02, 500)):
        c, npen, err = _errors(O, REFS, AO, AR, SR, ugrt, "hall", part)
        print("hall, radius %.2f: %d penumbra pixels; errors %s" % (c["radius"], npen, {k: round(v, 4) for k, v in err.items()}))
        assert npen >= least and all(0.0 < e < 0.5 for e in err.values()), err


# ------------------------------------------------------------------------------------------------- the synthetic rays


def syn_table(ugrt, S, K, k):
    """K sets of S samples around TA.SYN_SETS[k]: the first K of the 16 turned sets (set j is the same for every K)."""
    centre, radius = TA.SYN_SETS[k]
    return np.ascontiguousarray(ugrt.scenes.area_sample_sets(S, 16, centre, TA.SYN_AXIS, radius)[:K])


_SYN_PER_SET = {}


def syn_per_set(O, REFS, AR, SYN, ugrt, S, K, k, kind="plain"):
    """[K, SYN_N] CPU masks of the sets of syn_table (whole frame), cached per set."""
    sc = SYN if kind == "plain" else RFR.syn_glass(O)
    orays, oactive = TA.syn_origins(kind != "plain")
    grid = sc["thru"] if kind == "glass_thru" else sc["grid"]
    table = syn_table(ugrt, S, K, k)
    for j in range(K):
        if (S, k, j, kind) not in _SYN_PER_SET:
            _SYN_PER_SET[(S, k, j, kind)] = TA.cpu_mask(REFS[1], AR, grid, sc["verts"], sc["faces"], orays, oactive, table[j], 0,
                                                       SYN_N, SYN_N)
    return np.stack([_SYN_PER_SET[(S, k, j, kind)] for j in range(K)])


def syn_want(SR, per_set, tile, rows=None):
    r0, r1 = (0, 64) if rows is None else (8 * rows[0], 8 * rows[1])
    return SR.select(per_set, tile[0], tile[1], 64, 64, r0, r1, fill=0xFFFFFFFF)


WALK_CASES = [(5, (4, 4)), (32, (4, 4)), (32, (2, 2)), (8, (1, 1)), (8, (2, 2)), (8, (4, 4)), (8, (3, 2))]


def test_synthetic_selections_are_not_vacuous(ugrt, O, REFS, AR, SR, SYN):
    """CPU: on the 64 x 64 image of the 4096 synthetic origins the per-pixel selection differs from every single set's
    mask on at least 100 pixels, for every case and both placements; plain and see-through selections differ."""
    for S, tile in WALK_CASES:
        K = tile[0] * tile[1]
        for k in range(len(TA.SYN_SETS)):
            per = syn_per_set(O, REFS, AR, SYN, ugrt, S, K, k)
            want = syn_want(SR, per, tile)
            if K == 1:
                np.testing.assert_array_equal(want, per[0])
                continue
            differ = [int((want != per[j]).sum()) for j in range(K)]
            assert min(differ) >= 100, (S, tile, k, differ)
            x, y = np.arange(SYN_N) % 64, np.arange(SYN_N) // 64
            j = (y % tile[1]) * tile[0] + x % tile[0]
            np.testing.assert_array_equal(want, per[j, np.arange(SYN_N)])
    for k in range(len(TA.SYN_SETS)):
        plain = syn_want(SR, syn_per_set(O, REFS, AR, SYN, ugrt, 8, 16, k, "glass_plain"), (4, 4))
        thru = syn_want(SR, syn_per_set(O, REFS, AR, SYN, ugrt, 8, 16, k, "glass_thru"), (4, 4))
        assert not (thru & ~plain).any() and int((plain != thru).sum()) >= 500


# ---------------------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


_words = AM._words


def _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, torch, thru=None):
    mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)  # 0xFFFFFFFF
    S = table.shape[1]
    d_table = ctx.upload(table.reshape(-1))
    if thru is None:
        ctx.trace_dda_any_area_sets(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, S, tile[0], tile[1], d_table, mask)
    else:
        ctx.trace_dda_any_area_sets_thru(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, S, tile[0], tile[1], d_table,
                                         mask, *thru)
    ctx.synchronize()
    return _words(mask)


@pytest.mark.gpu
@pytest.mark.parametrize("S,tile", WALK_CASES)
def test_synthetic_sets_walk(ugrt, O, REFS, AR, SR, SYN, torch, S, tile):
    """The any-hit scene's 4096 origins as a 64 x 64 image, both placements of the samples, the mask pre-filled with
    ones: equal to the CPU masks of the sets selected per pixel, to ugrt_trace_dda_any_area per set selected per pixel,
    and to ugrt_trace_dda_any on the explicit rays of every (set, sample) selected per pixel; 1 x 1 is
    ugrt_trace_dda_any_area's words."""
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = TA.syn_origins()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    K = tile[0] * tile[1]
    for k in range(len(TA.SYN_SETS)):
        what = "S %d tile %r placement %d" % (S, tile, k)
        table = syn_table(ugrt, S, K, k)
        want = syn_want(SR, syn_per_set(O, REFS, AR, SYN, ugrt, S, K, k), tile)
        got = _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, torch)
        np.testing.assert_array_equal(got, want, err_msg=what)
        assert not got[oactive == 0].any() and (S == 32 or not (got >> np.uint32(S)).any())
        by_area = np.stack([TA._area(ctx, grid, dv, df, d_orays, d_oactive, table[j], torch) for j in range(K)])
        np.testing.assert_array_equal(got, syn_want(SR, by_area, tile), err_msg=what)
        if K == 1:
            np.testing.assert_array_equal(got, by_area[0], err_msg=what)
        by_ray = np.zeros((K, SYN_N), np.uint32)
        for j in range(K):
            for s in range(S):
                occ = torch.full((SYN_N,), -7, dtype=torch.int32, device=ctx.device)
                rays = AR.expand(orays, oactive, table[j, s], 0, SYN_N, SYN_N)
                ctx.trace_dda_any(grid[0], grid[1], grid[2], dv, df, ctx.upload(rays), d_oactive, 1.0, occ)
                by_ray[j] |= occ.cpu().numpy().astype(np.uint32) << np.uint32(s)
        np.testing.assert_array_equal(got, syn_want(SR, by_ray, tile), err_msg=what)


@pytest.mark.gpu
def test_synthetic_see_through_sets_walk(ugrt, O, REFS, AR, SR, SYN, torch):
    """syn_glass (every third face see-through), S = 8, 4 x 4 and 3 x 2, any_coop 1, 8 and 2^30: equal to the CPU masks on
    the filtered grid selected per pixel, and with transmit all zero to the plain call's words."""
    G = RFR.syn_glass(O)
    ctx, dv, df, grid = RS._syn_context(ugrt, G)
    orays, oactive = TA.syn_origins(True)
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    d_mat, d_tr, d_zero = ctx.upload(G["matidx"]), ctx.upload(RFR.SYN_TRANSMIT), ctx.upload(np.zeros(2, np.float32))
    for tile in ((4, 4), (3, 2)):
        K = tile[0] * tile[1]
        for k in range(len(TA.SYN_SETS)):
            table = syn_table(ugrt, 8, K, k)
            want = syn_want(SR, syn_per_set(O, REFS, AR, SYN, ugrt, 8, K, k, "glass_thru"), tile)
            plain = syn_want(SR, syn_per_set(O, REFS, AR, SYN, ugrt, 8, K, k, "glass_plain"), tile)
            assert int((want != plain).sum()) >= 500
            for coop in (1, 8, 1 << 30):
                ctx.set_option("any_coop", coop)
                what = "tile %r placement %d any_coop %d" % (tile, k, coop)
                got = _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, torch, (d_mat, d_tr, 2))
                np.testing.assert_array_equal(got, want, err_msg=what)
                opaque = _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, torch, (d_mat, d_zero, 2))
                np.testing.assert_array_equal(opaque, plain, err_msg=what)
                np.testing.assert_array_equal(opaque, _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, torch), err_msg=what)
            ctx.set_option("any_coop", -1)


@pytest.mark.gpu
def test_launch_shapes_change_no_word(ugrt, O, REFS, AR, SR, SYN, torch):
    """any_rays_per_wave 1, 7, 32, 64 x any_coop 1, 8, 2^30, dda_blocks = 1 (every later group comes from the ticket: each
    workgroup still copies the table once) and a band context, whose sets are those of the full image's coordinates
    (its first row is row 16) and whose other pixels keep their words; a table that is not 16-byte aligned."""
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = TA.syn_origins()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    for S, tile in ((8, (4, 4)), (5, (3, 2)), (32, (4, 4))):
        K = tile[0] * tile[1]
        table = syn_table(ugrt, S, K, 0)
        per = syn_per_set(O, REFS, AR, SYN, ugrt, S, K, 0)
        want = syn_want(SR, per, tile)
        for rpw in (1, 7, 32, 64):
            for coop in (1, 8, 1 << 30):
                ctx.set_option("any_rays_per_wave", rpw)
                ctx.set_option("any_coop", coop)
                got = _sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, torch)
                np.testing.assert_array_equal(got, want, err_msg="S %d, rays per wave %d, coop %d" % (S, rpw, coop))
        ctx.set_option("any_rays_per_wave", -1)
        ctx.set_option("any_coop", -1)
        ctx.set_option("dda_blocks", 1)
        np.testing.assert_array_equal(_sets(ctx, grid, dv, df, d_orays, d_oactive, table, tile, torch), want)
        ctx.set_option("dda_blocks", -1)
        # the table one float into an allocation: the copy's single-float path
        shifted = ctx.upload(np.concatenate([np.zeros(1, np.float32), table.reshape(-1)]))[1:]
        assert shifted.data_ptr() % 16 == 4
        mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda_any_area_sets(grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, S, tile[0], tile[1], shifted, mask)
        ctx.synchronize()
        np.testing.assert_array_equal(_words(mask), want)
        band, bv, bf, bgrid = RS._syn_context(ugrt, SYN, (2, 5))
        p0, n = band.p0, band.npix
        assert (p0, n) == (1024, 1536)
        got = _sets(band, bgrid, bv, bf, band.upload(orays), band.upload(oactive), table, tile, torch)
        np.testing.assert_array_equal(got, syn_want(SR, per, tile, (2, 5)))
        assert (got[:p0] == 0xFFFFFFFF).all() and (got[p0 + n:] == 0xFFFFFFFF).all()
        np.testing.assert_array_equal(got[p0:p0 + n], want[p0:p0 + n])


@pytest.mark.gpu
def test_the_walk_leaves_the_shared_dda_state_alone(ugrt, O, REFS, AO, AR, SR, torch):
    """hall: a ugrt_trace_dda before and after a launch over sample sets gives identical hits, and the split walks'
    figures stay what they were (test_area_light's test of the plain area walk)."""
    c = cpu_sets(O, REFS, AO, AR, SR, ugrt, "hall")
    a = c["a"]
    s, N = a["scene"], a["N"]
    W, H = SIZES["hall"]
    ctx, r = RD.make(ugrt, s, W, H)
    ctx.set_option("dda_split", 1)
    ctx.set_option("dda_split_load", 50)
    r.display(RD.setup_for(ugrt, s), shadows=True, reflect=True)
    g = ctx.grid_ptrs(ugrt.GRID_UNIFORM)[:3]

    def level1():
        ht = torch.full((N,), 5.0, device=ctx.device)
        hid = torch.full((N,), 5, dtype=torch.int32, device=ctx.device)
        ctx.trace_dda(g[0], g[1], g[2], r.d_verts, r.d_faces, r.rays, r.active, ht, hid)
        ctx.synchronize()
        return ht, hid

    level1()
    ht0, hid0 = level1()
    before = ctx.stats_dda_split()
    mask = torch.full((N,), -1, dtype=torch.int32, device=ctx.device)
    ctx.trace_dda_any_area_sets(g[0], g[1], g[2], r.d_verts, r.d_faces, ctx.upload(a["orays"]), ctx.upload(a["oactive"]),
                                S_SETS, 4, 4, ctx.upload(c["table"].reshape(-1)), mask)
    ctx.synchronize()
    np.testing.assert_array_equal(_words(mask), c["mask"])
    assert ctx.stats_dda_split() == before
    ht1, hid1 = level1()
    assert torch.equal(hid0, hid1) and torch.equal(ht0.view(torch.int32), ht1.view(torch.int32))
    np.testing.assert_array_equal(hid1.cpu().numpy(), a["base"]["levels"][0]["hit_id"])
    assert ctx.stats_dda_split() == before


@pytest.mark.gpu
def test_bad_arguments_enqueue_nothing_and_leave_the_context_usable(ugrt, O, REFS, AR, SR, SYN, torch):
    fresh = ugrt.Context(64, 64, light_grid=(16, 16), uniform_dims=RS.SYN_DIMS)
    z = torch.zeros(6 * SYN_N, dtype=torch.int32, device=fresh.device)
    for call, extra in ((fresh.trace_dda_any_area_sets, ()), (fresh.trace_dda_any_area_sets_thru, (z, z, 2))):
        with pytest.raises(ugrt.UgrtError) as e:  # no uniform grid yet: ugrt_trace_dda's error
            call(z, z, z, z, z, z, z, 4, 2, 2, z, z, *extra)
        assert e.value.code == ugrt.UGRT_EINVAL and b"build the uniform grid first" in ugrt.lib.ugrt_last_error()
    ctx, dv, df, grid = RS._syn_context(ugrt, SYN)
    orays, oactive = TA.syn_origins()
    d_orays, d_oactive = ctx.upload(orays), ctx.upload(oactive)
    mask = torch.full((SYN_N,), -1, dtype=torch.int32, device=ctx.device)
    d_mat = ctx.upload(np.zeros(len(SYN["faces"]), np.int32))
    d_tr = ctx.upload(np.zeros(2, np.float32))
    table = syn_table(ugrt, 8, 16, 0)
    d_table = ctx.upload(np.concatenate([table.reshape(-1), np.zeros(3 * 512, np.float32)]))
    args = [grid[0], grid[1], grid[2], dv, df, d_orays, d_oactive, 8, 4, 4, d_table, mask]
    targs = args + [d_mat, d_tr, 2]

    def fails(fn, a, word):
        with pytest.raises(ugrt.UgrtError) as e:
            fn(*a)
        assert e.value.code == ugrt.UGRT_EINVAL and word in ugrt.lib.ugrt_last_error(), ugrt.lib.ugrt_last_error()

    for fn, a in ((ctx.trace_dda_any_area_sets, args), (ctx.trace_dda_any_area_sets_thru, targs)):
        for bad in (0, 33, -1):
            fails(fn, a[:7] + [bad] + a[8:], b"num_samples")
        for bad in (0, 5, -1):
            fails(fn, a[:8] + [bad] + a[9:], b"set_w")
            fails(fn, a[:9] + [bad] + a[10:], b"set_h")
    ctx.synchronize()
    assert (_words(mask) == 0xFFFFFFFF).all()
    mask.fill_(-1)
    for fn, a in ((ctx.trace_dda_any_area_sets, args), (ctx.trace_dda_any_area_sets_thru, targs)):
        for h in (0, 1, 2, 3, 4, 5, 6, 10, 11):
            fails(fn, a[:h] + [None] + a[h + 1:], b"null")
    for h in (12, 13):
        fails(ctx.trace_dda_any_area_sets_thru, targs[:h] + [None] + targs[h + 1:], b"null")
    ctx.synchronize()
    assert (_words(mask) == 0xFFFFFFFF).all()  # nothing was enqueued
    want = syn_want(SR, syn_per_set(O, REFS, AR, SYN, ugrt, 8, 16, 0), (4, 4))
    np.testing.assert_array_equal(_sets(ctx, grid, dv, df, d_orays, d_oactive, table, (4, 4), torch), want)
    ctx.trace_dda_any_area_sets(*(args[:7] + [32, 4, 4] + args[10:]))  # 512 points, the most a call takes, are accepted
    ctx.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hall", "crash", "glass"])
def test_frames_with_sets_and_the_gather_equal_the_cpu_frames(ugrt, O, REFS, AO, AR, SR, RF, torch, name):
    """Plain, with ao = 16, reflections of depth 3 with reflect_shadows, that with ao = 16 (hall, crash); the refract
    frame of depth 3 with reflect_shadows (glass: the see-through walk), all with area=8, area_sets=16, area_filter=2:
    area_mask is the per-pixel selection of the sets' CPU masks, area_vis the checker's gather over the CPU G-buffer,
    the image the frame's shading without add_shadows, then sets_shade, then ao_shade, byte for byte; a default frame
    before and behind it is the CPU frame."""
    rmod = RLT._rmod(ugrt)
    c = cpu_sets(O, REFS, AO, AR, SR, ugrt, name, RF)
    a = c["a"]
    s, N, W, H = a["scene"], a["N"], a["W"], a["H"]
    setup = ugrt.FrameSetup.from_scene(s)
    v = TA._f32(s["verts"]).reshape(-1, 3)
    plane = rmod.default_filter_plane(v.min(0), v.max(0))
    vis = SR.filter(c["mask"], S_SETS, a["orays"], a["oactive"], R_FRAME, 0.9, plane, W, H)
    # the gather does mix shares (glass: the see-through mask is non-zero on about a hundred pixels only, section 6.7)
    assert int((vis[0::2] != open_of(c["mask"], S_SETS) * vis[1::2]).sum()) > 100
    for what, kw, w_plain, w_hard, w_ids, amb in TA._frames(O, REFS, AO, AR, RF, ugrt, name):
        ctx, r = RFR.make(ugrt, s) if name == "glass" else RD.make(ugrt, s, W, H)
        ao_kw = dict(ao=AM.S_FRAME, ao_radius=amb["radius"]) if amb else {}
        hard = AO.shade(w_hard, amb["mask"], AM.S_FRAME, 0, N) if amb else w_hard
        r.display(setup, **kw, **ao_kw)
        ctx.synchronize()
        assert r.area_mask is None and r.area_vis is None
        np.testing.assert_array_equal(r.image.cpu().numpy(), hard, err_msg=what)
        r.display(setup, area=S_SETS, area_radius=a["radius"], area_sets=SETS, area_filter=R_FRAME, **kw, **ao_kw)
        ctx.synchronize()
        np.testing.assert_array_equal(_words(r.area_mask), c["mask"], err_msg=what)
        np.testing.assert_array_equal(r.ao_active.cpu().numpy(), a["oactive"], err_msg=what)
        np.testing.assert_array_equal(bits(r.ao_rays.cpu().numpy()), bits(a["orays"]), err_msg=what)
        np.testing.assert_array_equal(_words(r.area_vis), vis, err_msg=what)
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        shaded = SR.shade(w_plain, vis, S_SETS, 0, N)
        plain_area = AR.shade(w_plain, c["per_set"][0], S_SETS, 0, N)
        if amb:
            np.testing.assert_array_equal(_words(r.ao_mask), amb["mask"], err_msg=what)
            shaded = AO.shade(shaded, amb["mask"], AM.S_FRAME, 0, N)
            plain_area = AO.shade(plain_area, amb["mask"], AM.S_FRAME, 0, N)
        np.testing.assert_array_equal(r.image.cpu().numpy(), shaded, err_msg=what)
        assert int((shaded != hard).sum()) > 1000 and int((shaded != plain_area).sum()) > 100, what
        assert len(r._area_set_tables) == 1
        r.display(setup, **kw, **ao_kw)
        ctx.synchronize()
        np.testing.assert_array_equal(r.image.cpu().numpy(), hard, err_msg=what + ", behind a frame with sets")
        np.testing.assert_array_equal(r.intersect_id.cpu().numpy(), w_ids, err_msg=what)
        np.testing.assert_array_equal(r.is_shadowed.cpu().numpy(), a["base"]["is_shadowed"], err_msg=what)
