"""Renderer.display() on every legal combination of its effects against CPU frames.

tests/frame_ref.py holds legal() -- the display() docstring restated without a check_* -- and cpu_display(), which strings
the suite's checkers into a whole frame.  Here:

  CPU  legality: the product of every effect's {off, on, on with sets and a filter} with seven bases, shadows and the three
       renderer kinds raises ValueError before anything is enqueued exactly where legal() says no;
       call order: on the legal part the recorded call names are those of predicted() below;
       the composer returns the images and words of the files that pin a combination already;
       sharpness: the figures below, on the CPU alone.
  GPU  every legal frame of the matrix, a temporal chain whose masks come from the CPU walk over the frame's rotated
       table, and one renderer walked through a mixed sequence against a fresh one per step.

Scenes: scenes.glossy() at 128 x 128 (three reflecting floor strips with the scene's own spreads, posts that cast shadows)
for every base without glass, scenes.glass(scale=0.1) at 128 x 128 with spread 0.1 on its mirror panel for the refract base:
one scene does not meet the floors below -- the glass scene's only reflecting material, the mirror panel, fills 1 326 pixels,
glossy and ao both change 94 of them and no shadow falls on it.

Sharpness, printed by test_the_scenes_are_sharp (pixels of 16 384 whose bytes BOTH effects of a pair change, and pixels
that differ when two neighbouring byte passes run in the other order, per chain of passes that holds the two side by side;
each at least 200).  The radii are shares of the scene's largest extent, SHARES below: 5 % (ao) and 10 % (area) on glossy, twice
that and more on glass, where at 5 % and 10 % area and ao the other way round changed 109 pixels:

    glass   area     ao       both change                           1650
    glass   area     ao       swapped in area ao                     224
    glass   area     gi       both change                           1954
    glass   area     gi       swapped in area gi ao                  422
    glass   gi       ao       both change                           7638
    glass   gi       ao       swapped in area gi ao                 7622
    glass   gi       ao       swapped in shadows gi ao              7622
    glass   shadows  ao       swapped in shadows ao                  599
    glass   shadows  gi       swapped in shadows gi ao              1550
    glossy  aa       ao       both change                           1369
    glossy  aa       ao       swapped in shadows aa ao              2178
    glossy  area     ao       both change                           1572
    glossy  area     ao       swapped in area ao                     828
    glossy  area     gi       both change                           2724
    glossy  area     gi       swapped in area gi ao                 3107
    glossy  area     gi       swapped in glossy area gi ao          3119
    glossy  gi       ao       both change                           2699
    glossy  gi       ao       swapped in area gi ao                 2597
    glossy  gi       ao       swapped in glossy area gi ao          2599
    glossy  gi       ao       swapped in glossy shadows gi ao       2612
    glossy  gi       ao       swapped in shadows gi ao              2598
    glossy  glossy   ao       both change                            836
    glossy  glossy   area     both change                            736
    glossy  glossy   area     swapped in glossy area gi ao           808
    glossy  glossy   gi       both change                           8385
    glossy  glossy   shadows  swapped in glossy shadows ao           491
    glossy  glossy   shadows  swapped in glossy shadows gi ao        491
    glossy  shadows  aa       swapped in shadows aa ao              1587
    glossy  shadows  ao       swapped in glossy shadows ao           410
    glossy  shadows  ao       swapped in shadows ao                  410
    glossy  shadows  gi       swapped in glossy shadows gi ao       1957
    glossy  shadows  gi       swapped in shadows gi ao              1957

Single-fault edits of renderer.py, one at a time, on an MI355X (nothing of them is committed).  "new": the GPU tests of this
file that fail, of 17; "existing": the failing ones among the 107 frame-level and recorded-call tests of test_glossy,
test_indirect, test_area_light, test_area_sets, test_ambient, test_ambient_sets, test_antialias, test_temporal, test_refract and
test_frame_paths (in brackets: those of them that run on the GPU).  Without an edit: 0 and 0.

    area_pass: have_rays forced True                          new 10   existing 14 (9)
    gi_pass: have_rays constant False                         new 10   existing  3 (0)
    gi_pass: have_rays constant True                          new 12   existing  5 (4)
    area shading and gi_shade swapped                         new  9   existing  3 (1)
    aa_resolve moved behind ao_shade                          new  5   existing  5 (4)
    glossy_shade moved behind shade_add_shadows               new  4   existing  3 (2)
    shade_frame given shadows, not shadows and not area       new  5   existing  4 (0)
    glossy_shade's filter given f.ao_active, not f.active     new  6   existing  3 (2)
    _temporal_table given frame + 1                           new  4   existing  1 (0)
    the line _temporal_live = False dropped                   new  2   existing  1 (0)
    _ao_set_tables keyed by S alone                           new  2   existing  3 (2)

The two edits that change no byte (an ao_rays launch too many, a shade_add_shadows over flags that are all 0) are caught on
the GPU by the bracket counts of _frame; the CPU test of the call order catches them as well (it catches the first seven of the eleven).

Measured on an MI355X (seconds per test, with the CPU frames computed in the same process):

    test_every_legal_frame_equals_the_cpu_frame         0.34 (plain-shadows, 57 frames; 1.15 more to compile the checkers once),
                                                        at most 0.2 for each of the nine others
    ..._under_several_lights_equals_the_cpu_frame       0.1
    test_temporal_sequences_equal_the_cpu_chain         at most 0.2 for each of the four
    test_a_long_lived_renderer_equals_a_fresh_one       1.20 (rebuild), 0.76 (static_geometry): 129 display calls each, a fresh
                                                        renderer per call
    the whole file, CPU tests included                  12
"""
import itertools

import numpy as np
import pytest

import frame_ref as FR
import test_ambient as AM
import test_antialias as TAA
import test_ambient_sets as TAS
import test_area_light as TA
import test_area_sets as TS
import test_glossy as TG
import test_indirect as TI
import test_lights as TL
import test_refract as RFR
import test_temporal as TT
from test_ambient import AO  # noqa: F401  (fixtures)
from test_ambient_sets import ASR  # noqa: F401
from test_antialias import AA  # noqa: F401
from test_area_light import AR  # noqa: F401
from test_filter_visibility import SR  # noqa: F401
from test_glossy import GL  # noqa: F401
from test_indirect import IR  # noqa: F401
from test_lights import LT  # noqa: F401
from test_reflect_lights import RL  # noqa: F401
from test_reflect_shadows import REFS  # noqa: F401
from test_refract import RF  # noqa: F401
from test_temporal import TR  # noqa: F401

legal, cpu_display, device_frame, differences = FR.legal, FR.cpu_display, FR.device_frame, FR.differences
W = H = 128
N = W * H
FLOOR = 200


@pytest.fixture(scope="session")
def K(ugrt, O, REFS, RF, AO, AR, SR, ASR, IR, GL, AA, TR, LT, RL):
    return FR.Checkers(ugrt, O, REFS, RF, AO, AR, SR, ASR, IR, GL, AA, TR, LT, RL)


_F = {}


def frames(K, name):
    """The composer's Frames of a scene, made once and shared: nobody writes to what it caches."""
    if name not in _F:
        if name == "glossy":
            # the scene's light stands above the posts and their shadows are short: this one stands low beside the room, so that
            # the posts' shadows cross the reflecting strips (the floor of glossy_apply and shade_add_shadows the other way round)
            s = K.ugrt.scenes.glossy()
            light = dict(s["light_camera"], eye=(4.0, 0.0, 5.0), look=(8.0, 3.0, 0.0), up=(0.0, 0.0, 1.0))
            _F[name] = FR.Frames(K, s, W, H, s["spread"], K.ugrt.FrameSetup(s["cameras"]["ref"], light, (4.0, 0.0, 4.5)))
        else:
            s = RFR.scene(K.ugrt, "glass")
            _F[name] = FR.Frames(K, s, W, H, np.float32([0, 0, 0, 0, 0, 0, 0, 0, 0.1]))
        _F[name].shares = SHARES[name]
    return _F[name]


# ----------------------------------------------------------------------------------------------------------- the matrix

BASES = {"plain": dict(), "plain2": dict(frame_cnt=2), "reflect1": dict(reflect=True, bounces=1),
         "reflect3": dict(reflect=True, bounces=3, reflect_shadows=True),
         "refract3": dict(reflect=True, refract=True, bounces=3, reflect_shadows=True)}
MULTI = {"lights": dict(), "reflect_lights": dict(reflect=True, bounces=3, reflect_shadows=True, reflect_lights=True)}
SCENE_OF = {"refract3": "glass"}
AXES = (("area", (dict(), dict(area=5), dict(area=8, area_sets=16, area_filter=2))),
        ("ao", (dict(), dict(ao=8), dict(ao=8, ao_sets=16, ao_filter=1))),
        ("gi", (dict(), dict(gi=8), TI.GI_FRAME)),
        ("glossy", (dict(), TG.GLOSSY_FRAME)),
        ("aa", (dict(), dict(aa=4, aa_sets=16))))


SHARES = {"glossy": (0.05, 0.10), "glass": (0.10, 0.25)}  # (ao_radius, area_radius) as shares of the scene's largest extent


def radii(F):
    ao, area = getattr(F, "shares", SHARES["glossy"])
    return dict(ao_radius=float(np.float32(ao * F.extent)), area_radius=float(np.float32(area * F.extent)))


def with_radii(F, kw):
    r = radii(F)
    return dict(kw, **{n: r[n] for n in ("ao_radius", "area_radius") if kw.get(n[:-7])})


def bare(kw):
    """The keywords legal() looks at."""
    return {n: v for n, v in kw.items() if n in FR.DEFAULTS}


def matrix(base, shadows, lights=False):
    """The legal frames of a base: every choice of the axes legal() admits, in a fixed order."""
    out = []
    for choice in itertools.product(*[values for _, values in AXES]):
        kw = dict(base, shadows=shadows)
        for part in choice:
            kw.update(part)
        if legal(dict(bare(kw), lights=lights)):
            out.append(kw)
    return out


def test_the_matrix_has_the_frames_it_claims():
    sizes = {(b, sh): len(matrix(BASES[b], sh)) for b in BASES for sh in (True, False)}
    assert sizes == {("plain", True): 57, ("plain", False): 21, ("plain2", True): 54, ("plain2", False): 18,
                     ("reflect1", True): 27, ("reflect1", False): 9, ("reflect3", True): 27, ("reflect3", False): 9,
                     ("refract3", True): 27, ("refract3", False): 9}
    assert sum(sizes.values()) == 258
    for b in MULTI:
        for sh in (True, False):  # under setup.lights only ao composes
            assert [sorted(set(kw) - set(MULTI[b]) - {"shadows"}) for kw in matrix(MULTI[b], sh, lights=True)] \
                == [[], ["ao"], ["ao", "ao_filter", "ao_sets"]]


# ------------------------------------------------------------------------------------------------------------- legality


def _fake(ugrt):
    """test_temporal's recording renderer with the names the glossy and the anti-aliased frames read besides."""
    r = TT._fake(ugrt)
    r.__dict__.update(glossy_sum="glsum", glossy_acc="glacc", _glossy_tables={}, d_spread="spread", aa_edge="aaedge",
                      aa_sum="aasum", _aa_set_tables={})
    r._ensure_glossy_buffers = lambda gather: None
    r._upload_glossy_points = lambda table: ("gltable", table)
    r._ensure_aa_buffers = lambda: None
    return r


ON = dict(area=(dict(), dict(area=5, area_radius=0.5), dict(area=8, area_radius=0.5, area_sets=16, area_filter=2)),
          ao=(dict(), dict(ao=8, ao_radius=1.0), dict(ao=8, ao_radius=1.0, ao_sets=16, ao_filter=1)),
          gi=(dict(), dict(gi=8), dict(TI.GI_FRAME)),
          glossy=(dict(), dict(glossy=8), dict(TG.GLOSSY_FRAME)),
          aa=(dict(), dict(aa=4), dict(aa=4, aa_sets=16)),
          temporal=(dict(), dict(temporal=8)))
LEGALITY_BASES = dict(BASES, **MULTI)
# Counted by hand from the docstring.  plain with shadows: 81 + 6 (aa with ao alone) and under temporal 26 + 4; without
# shadows (no area) 27 + 6 and 8 + 4; frame_cnt 2 (no aa) 81 + 26 and 27 + 8; each of the three bases with levels (no glossy,
# no aa) 27 + 26 and 9 + 8; each of the two bases under several lights 3 + 3 (ao alone): 117 + 45 + 107 + 35 + 210 + 12
LEGAL_ONE = [486 * 14 - 526, 526]


def _setups(ugrt):
    s = TL.scene(ugrt, "hall")
    return TL.setup_for(ugrt, s), TL.setup_for(ugrt, s, TL.lights_for(s, 2))


def test_display_raises_exactly_where_legal_says_no(ugrt):
    """486 effect choices x 7 bases x shadows x 3 renderer kinds.  The one-stream renderer: ValueError with nothing
    enqueued, or a frame.  The two-stream renderer and the banded one are never constructed here, so for them the test is
    weaker: an illegal frame raises ValueError (the two-stream one with nothing enqueued; the banded one has no recording
    context to look at), a legal one does not -- it fails later with an AttributeError, on the streams it does not have.
    BandedRenderer.display has no reflect_lights keyword at all: asked for it, it raises TypeError."""
    single, multi = _setups(ugrt)
    counts = {kind: [0, 0] for kind in FR.KINDS}
    for base_name, base in LEGALITY_BASES.items():
        setup = multi if base_name in MULTI else single
        for shadows in (True, False):
            for choice in itertools.product(*ON.values()):
                kw = dict(base, shadows=shadows)
                for part in choice:
                    kw.update(part)
                for kind in FR.KINDS:
                    ok = legal(dict(bare(kw), lights=base_name in MULTI), kind)
                    counts[kind][ok] += 1
                    what = (base_name, kind, kw, FR.why_not(dict(bare(kw), lights=base_name in MULTI), kind))
                    if kind == "banded":
                        r = object.__new__(ugrt.BandedRenderer)
                        if kw.get("reflect_lights"):  # BandedRenderer.display has no such keyword: TypeError, not ValueError
                            assert not ok
                            with pytest.raises(TypeError):
                                r.display(setup, **kw)
                            continue
                        kw_b = dict(kw, reflect=kw.get("reflect", False))
                    else:
                        r = _fake(ugrt)
                        if kind == "two":
                            r.aux = object()
                        kw_b = kw
                    try:
                        r.display(setup, **kw_b)
                        raised = False
                    except ValueError:
                        raised = True
                    except (AttributeError, TypeError):
                        assert kind != "one", what
                        raised = False
                    assert raised == (not ok), what
                    if kind != "banded" and raised:
                        assert r.ctx.calls == [] and r.cleared == [], what
    print(counts)
    # the two-stream and the banded frames take the five single-light bases, with and without shadows, and no effect
    assert counts["two"] == counts["banded"] == [486 * 14 - 10, 10]
    assert counts["one"] == LEGAL_ONE


def test_every_rule_quotes_the_docstring(ugrt):
    """legal()'s exclusions are the docstring's: each rule's words stand in display()'s docstring."""
    doc = " ".join(ugrt.Renderer.display.__doc__.split())
    for name, words, _ in FR.RULES:
        assert " ".join(words.split()) in doc, name
    order = ("the shading call; glossy_apply; shade_add_shadows, or with area shade_area / shade_area_vis in its place; "
             "gi_apply; aa_resolve; shade_ao / shade_ao_vis")
    assert order in doc


def test_the_design_table_is_what_legal_says():
    import os

    text = open(os.path.join(TG.RD.ROOT, "DESIGN.md")).read()
    for row in FR.table_rows():
        assert row in text, row


# ----------------------------------------------------------------------------------------------------------- call order

CAMERA = ["set_light_position", "upload_camera", "grid_build_perspective", "trace_primary"]
HARD = TA.HARD


def _levels(kw, lights):
    any_hit = "trace_dda_any_lights" if lights else "trace_dda_any"
    thru = "_thru" if kw.get("refract") else ""
    out = []
    for j in range(kw.get("bounces", 1)):
        if j:
            out.append("refract_rays_next" if kw.get("refract") else "reflect_rays_next")
        out.append("trace_dda")
        if kw.get("reflect_shadows"):
            out += ["occlusion_rays", any_hit + thru]
    return out


def predicted(kw, num_lights=0):
    """The call names of a legal one-stream frame: camera pass, shadow stage, the effects' rays and walks, the shading
    call, the applies."""
    g = lambda n: kw.get(n, FR.DEFAULTS.get(n))
    shadows, shade, t = g("shadows"), kw.get("shade", True), g("temporal")
    names = list(CAMERA)
    if num_lights:
        names += (["upload_camera"] + (HARD if shadows else [])) * num_lights
        if not shade:
            return names
        if g("reflect"):
            names += ["reflect_rays", "grid_build_uniform"] + _levels(kw, True)
        elif g("ao"):
            names += ["grid_build_uniform"]
    else:
        names += ["upload_camera"] + (HARD if shadows and not g("area") else [])
        if not shade:
            return names
        if g("aa"):
            names.append("aa_edges")
        if g("reflect"):
            names += ["refract_rays" if g("refract") else "reflect_rays", "grid_build_uniform"] + _levels(kw, False)
        elif g("glossy"):
            names += ["reflect_rays", "grid_build_uniform", "ao_rays", "glossy_gather"]
        elif g("ao") or g("area") or g("gi") or g("aa"):
            names.append("grid_build_uniform")
    rays = ["ao_rays"] if not g("glossy") else []
    if g("area"):
        names += rays + ["trace_dda_any_area" + ("_sets" if t or g("area_sets") > 1 else "") + ("_thru" if g("refract") else "")]
        rays = []
    if g("ao"):
        names += rays + ["trace_dda_any_hemi" + ("_sets" if t or g("ao_sets") > 1 else "")]
        rays = []
    if g("gi"):
        names += rays + ["gi_gather"]
    if g("aa"):
        names.append("aa_gather")
    if num_lights:
        names.append("shade_reflect_lights" if g("reflect") else "shade_lights")
    elif g("reflect"):
        names.append("shade_reflect_depth_occluded" if g("reflect_shadows") else "shade_reflect" if g("bounces") == 1
                     else "shade_reflect_depth")
    else:
        names.append("shade_spotlight" if g("frame_cnt") >= 2 else "shade_simple")
    if g("glossy"):
        names += (["gi_filter"] if g("glossy_filter") else []) + ["glossy_apply"]
    if shadows and not g("area") and not num_lights:
        names.append("shade_add_shadows")
    if g("area"):
        names += ["filter_visibility", "temporal_visibility", "shade_area_vis"] if t else \
            ["filter_visibility", "shade_area_vis"] if g("area_filter") else ["shade_area"]
    if g("gi"):
        names += ["gi_filter", "temporal_gi", "gi_apply"] if t else (["gi_filter"] if g("gi_filter") else []) + ["gi_apply"]
    if g("aa"):
        names.append("aa_resolve")
    if g("ao"):
        names += ["filter_visibility", "temporal_visibility", "shade_ao_vis"] if t else \
            ["filter_visibility", "shade_ao_vis"] if g("ao_filter") else ["shade_ao"]
    return names


def test_a_legal_frame_enqueues_the_predicted_calls(ugrt):
    """Every legal frame of the legality product on the recording renderer, with shade=False as well: the call names are
    predicted()'s; ao_rays is enqueued once in a frame with any of ao, area, gi and glossy and never elsewhere;
    grid_build_uniform once in a frame that walks the uniform grid and never elsewhere."""
    single, multi = _setups(ugrt)
    seen = 0
    for base_name, base in LEGALITY_BASES.items():
        setup, L = (multi, 2) if base_name in MULTI else (single, 0)
        for shadows in (True, False):
            for choice in itertools.product(*ON.values()):
                kw = dict(base, shadows=shadows)
                for part in choice:
                    kw.update(part)
                if not legal(dict(bare(kw), lights=bool(L))):
                    continue
                seen += 1
                r = _fake(ugrt)
                r.display(setup, **kw)
                names = TA._names(r)
                assert names == predicted(kw, L), (base_name, kw, names)
                effects = any(kw.get(n) for n in ("ao", "area", "gi", "glossy"))
                assert names.count("ao_rays") == (1 if effects else 0), (base_name, kw)
                walks = effects or kw.get("aa") or kw.get("reflect")
                assert names.count("grid_build_uniform") == (1 if walks else 0), (base_name, kw)
                r = _fake(ugrt)
                r.display(setup, shade=False, **kw)
                assert TA._names(r) == predicted(dict(kw, shade=False), L), (base_name, kw)
    assert seen > 500


# ------------------------------------------------------------------------------------------ the composer is not a second truth


def test_the_composer_returns_the_glossy_files_frames(ugrt, O, REFS, AO, GL, IR, K):
    """glossy + ao, glossy + gi and glossy alone on scenes.glossy(): test_glossy's own CPU frames."""
    c = TG.cpu_scene(O, REFS, AO, ugrt, "glossy")
    g = TG.cpu_glossy(O, GL, IR, ugrt, c)
    F = frames(K, "glossy")
    n, radius = c["N"], radii(F)["ao_radius"]
    mask = AM.cpu_mask(REFS[1], AO, c["ugrid"], c["scene"]["verts"], c["scene"]["faces"], c["orays"], c["oactive"],
                       ugrt.scenes.ao_directions(8), radius, 0, n, n)
    gi = TI.cpu_gi(IR, ugrt, c, g["image"], c["plain"]["mat_ids"], c["lcam"], S=8, sets=1, filt=0)
    for kw, image in ((dict(), g["image"]), (dict(ao=8, ao_radius=radius), AO.shade(g["image"], mask, 8, 0, n)),
                      (dict(gi=8), gi["image_gi"])):
        got = cpu_display(F, c["setup"], **TG.GLOSSY_FRAME, **kw)
        np.testing.assert_array_equal(got["image"], image)
        np.testing.assert_array_equal(got["glossy_sum"], g["sums"])
        np.testing.assert_array_equal(got["glossy_acc"], g["acc"])
        np.testing.assert_array_equal(got["intersect_id"], c["plain"]["mat_ids"])
        np.testing.assert_array_equal(got["levels"][0]["active"], c["active"])
        np.testing.assert_array_equal(got["ao_active"], c["oactive"])
        if "gi" in kw:
            np.testing.assert_array_equal(got["gi_sum"], gi["sums"])
        if "ao" in kw:
            np.testing.assert_array_equal(got["ao_mask"], mask)
    np.testing.assert_array_equal(cpu_display(F, c["setup"])["image"], c["plain"]["image"])
    np.testing.assert_array_equal(cpu_display(F, c["setup"], reflect=True, bounces=1, reflect_shadows=True)["image"], c["mirror"])


def test_the_composer_returns_the_other_files_frames(ugrt, O, REFS, AO, AR, SR, ASR, IR, AA, RF, K):
    """aa, with and without shadows, and aa + ao on the glass scene at 128 x 128 (test_antialias' frame and cpu_aa); gi
    alone and gi + ao on the Cornell box (test_indirect.cornell and cpu_gi).  The combinations under temporal that a file
    pins one effect at a time have no CPU frame to return: test_temporal's checker is handed the device's masks."""
    F = frames(K, "glass")
    for shadows in (True, False):
        f = TAA.frame(O, ugrt, "glass", W, H, shadows=shadows)
        edge, sums, image = TAA.cpu_aa(AA, ugrt, f, 4, 16, shadows)
        got = cpu_display(F, shadows=shadows, aa=4, aa_sets=16)
        np.testing.assert_array_equal(got["aa_edge"], edge)
        np.testing.assert_array_equal(got["aa_sum"], sums)
        np.testing.assert_array_equal(got["image"], image)
        np.testing.assert_array_equal(cpu_display(F, shadows=shadows)["image"], f["image"])
    radius = radii(F)["ao_radius"]
    P = FR.primary(F, F.setup)
    mask = AM.cpu_mask(REFS[1], AO, f["ugrid"], F.verts, F.faces, P["orays"], P["oactive"], ugrt.scenes.ao_directions(8), radius,
                       0, N, N)
    edge, sums, image = TAA.cpu_aa(AA, ugrt, TAA.frame(O, ugrt, "glass", W, H), 4, 16, True)
    np.testing.assert_array_equal(cpu_display(F, aa=4, aa_sets=16, ao=8, ao_radius=radius)["image"], AO.shade(image, mask, 8, 0, N))
    c = TI.cornell(O, IR, AO, ugrt)
    FC = FR.Frames(K, c["scene"], c["W"], c["H"])
    got = cpu_display(FC, c["setup"], **TI.GI_FRAME)
    np.testing.assert_array_equal(got["gi_sum"], c["sums"])
    np.testing.assert_array_equal(got["gi_acc"], c["acc"])
    np.testing.assert_array_equal(got["image"], c["image_gi"])
    rc = float(np.float32(0.05 * FC.extent))
    cmask = AM.cpu_mask(REFS[1], AO, c["ugrid"], FC.verts, FC.faces, c["orays"], c["oactive"], ugrt.scenes.ao_directions(8), rc,
                        0, c["N"], c["N"])
    np.testing.assert_array_equal(cpu_display(FC, c["setup"], ao=8, ao_radius=rc, **TI.GI_FRAME)["image"],
                                  AO.shade(c["image_gi"], cmask, 8, 0, c["N"]))


def _assert_levels(got, want, occluded):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        what = "level %d" % (j + 1)
        np.testing.assert_array_equal(g["active"], w["active"], err_msg=what)
        np.testing.assert_array_equal(FR.bits(g["rays"]), FR.bits(w["rays"]), err_msg=what)
        np.testing.assert_array_equal(g["hit_id"], w["hit_id"], err_msg=what)
        np.testing.assert_array_equal(FR.bits(g["hit_t"]), FR.bits(w["hit_t"]), err_msg=what)
        if occluded:
            np.testing.assert_array_equal(g["occluded"], w["occluded"], err_msg=what)


def _assert_area_frames(ugrt, O, REFS, AO, AR, SR, RF, F, name):
    """test_area_light's and test_area_sets' frames of a scene (TA._frames: plain, plain + ao, reflect 3, reflect 3 + ao; glass:
    the refract frame), as their GPU tests state them: the frame itself with its levels, the frame under area=16 with
    cpu_area's mask, and under area=8, area_sets=16, area_filter=2 with cpu_sets' selection and the checker's gather."""
    a = TA.cpu_area(O, REFS, AO, AR, ugrt, name, RF)
    c = TS.cpu_sets(O, REFS, AO, AR, SR, ugrt, name, RF)
    n, base = a["N"], a["base"]
    vis = SR.filter(c["mask"], TS.S_SETS, a["orays"], a["oactive"], TS.R_FRAME, 0.9, F.plane, a["W"], a["H"])
    for what, kw, w_plain, w_hard, w_ids, amb in TA._frames(O, REFS, AO, AR, RF, ugrt, name):
        ao_kw = dict(ao=AM.S_FRAME, ao_radius=amb["radius"]) if amb else {}
        under_ao = (lambda img, amb=amb: AO.shade(img, amb["mask"], AM.S_FRAME, 0, n)) if amb else (lambda img: img)
        got = cpu_display(F, **kw, **ao_kw)
        np.testing.assert_array_equal(got["image"], under_ao(w_hard), err_msg=what)
        np.testing.assert_array_equal(got["intersect_id"], w_ids, err_msg=what)
        np.testing.assert_array_equal(got["is_shadowed"], base["is_shadowed"], err_msg=what)
        if kw.get("reflect"):
            _assert_levels(got["levels"], base["levels"][:kw["bounces"]], True)
        if amb:
            np.testing.assert_array_equal(got["ao_mask"], amb["mask"], err_msg=what)
        got = cpu_display(F, area=TA.S_FRAME, area_radius=a["radius"], **kw, **ao_kw)
        np.testing.assert_array_equal(got["area_mask"], a["mask"], err_msg=what)
        np.testing.assert_array_equal(got["ao_active"], a["oactive"], err_msg=what)
        np.testing.assert_array_equal(FR.bits(got["ao_rays"]), FR.bits(a["orays"]), err_msg=what)
        np.testing.assert_array_equal(got["intersect_id"], w_ids, err_msg=what)
        np.testing.assert_array_equal(got["image"], under_ao(AR.shade(w_plain, a["mask"], TA.S_FRAME, 0, n)), err_msg=what)
        got = cpu_display(F, area=TS.S_SETS, area_radius=c["radius"], area_sets=TS.SETS, area_filter=TS.R_FRAME, **kw, **ao_kw)
        np.testing.assert_array_equal(got["area_mask"], c["mask"], err_msg=what)
        np.testing.assert_array_equal(got["area_vis"], vis, err_msg=what)
        np.testing.assert_array_equal(got["image"], under_ao(SR.shade(w_plain, vis, TS.S_SETS, 0, n)), err_msg=what)
    return a, c, vis


def test_the_composer_returns_the_crash_frames_of_the_area_ambient_and_indirect_files(ugrt, O, REFS, AO, AR, SR, ASR, IR, LT, RL, K):
    """crash at 256 x 144, the scene and size of the files' own frame tests, from their own CPU-frame functions:
    test_area_light.cpu_area and test_area_sets.cpu_sets over TA._frames (area + ao with one set and with sets and a filter,
    on the plain frame and on the reflections of depth 3 with their shadows); test_ambient_sets.cpu_ambient_sets over
    AM._frames (plain, reflect 3, three lights, reflections under three lights) and beside the area light's sets;
    test_indirect's crash frames (gi on the plain frame, on the reflect frame with and without ao, and behind an area
    light) from RS.cpu_frame, cpu_gi and AO.shade."""
    name = "crash"
    Wc, Hc = TG.RD.SIZES[name]
    s = TG.RD.scene(ugrt, name)
    F = FR.Frames(K, s, Wc, Hc)
    n = Wc * Hc
    a, c, vis = _assert_area_frames(ugrt, O, REFS, AO, AR, SR, None, F, name)
    base = a["base"]
    # ao over direction sets with the gather
    cs = TAS.cpu_ambient_sets(O, REFS, AO, SR, ugrt, name)
    avis = SR.filter(cs["mask"], TAS.S_SETS, a["orays"], a["oactive"], TAS.R_FRAME, 0.9, F.plane, Wc, Hc)
    new = dict(ao=TAS.S_SETS, ao_radius=cs["radius"], ao_sets=TAS.SETS, ao_filter=TAS.R_FRAME)
    lights = TL.lights_for(s, 3)
    for what, kw, with_lights, w_img, w_ids in AM._frames(O, REFS, LT, RL, ugrt, name):
        setup = TL.setup_for(ugrt, s, lights if with_lights else None)
        got = cpu_display(F, setup, **kw)
        np.testing.assert_array_equal(got["image"], w_img, err_msg=what)
        np.testing.assert_array_equal(got["intersect_id"], w_ids, err_msg=what)
        got = cpu_display(F, setup, **new, **kw)
        np.testing.assert_array_equal(got["ao_mask"], cs["mask"], err_msg=what)
        np.testing.assert_array_equal(got["ao_vis"], avis, err_msg=what)
        np.testing.assert_array_equal(got["intersect_id"], w_ids, err_msg=what)
        np.testing.assert_array_equal(got["image"], ASR.shade(w_img, avis, TAS.S_SETS, 0, n), err_msg=what)
        got = cpu_display(F, setup, ao=TAS.S_SETS, ao_radius=cs["radius"], **kw)
        np.testing.assert_array_equal(got["ao_mask"], cs["per_set"][0], err_msg=what)
        np.testing.assert_array_equal(got["image"], AO.shade(w_img, cs["per_set"][0], TAS.S_SETS, 0, n), err_msg=what)
    plain = TL.cpu_frame(O, ugrt, name, Wc, Hc)
    got = cpu_display(F, area=TS.S_SETS, area_radius=c["radius"], area_sets=TS.SETS, area_filter=TS.R_FRAME, **new)
    np.testing.assert_array_equal(got["area_vis"], vis)
    np.testing.assert_array_equal(got["ao_vis"], avis)
    np.testing.assert_array_equal(got["image"], ASR.shade(SR.shade(plain["image_unshadowed"], vis, TS.S_SETS, 0, n), avis, TAS.S_SETS, 0, n))
    # the indirect light
    amb = AM.cpu_ambient(O, REFS, AO, ugrt, name)
    ci = dict(scene=s, setup=TL.setup_for(ugrt, s), W=Wc, H=Hc, N=n, ugrid=base["ugrid"], orays=amb["orays"], oactive=amb["oactive"])
    reflect = dict(shadows=True, reflect=True, bounces=AM.DEPTH, reflect_shadows=True)
    for what, kw, w_img, w_ids, last in (
            ("plain", dict(shadows=True), plain["image"], plain["mat_ids"], None),
            ("reflect", reflect, base["image_occluded"], base["mat_ids_occluded"], None),
            ("reflect, ao", dict(reflect, ao=AM.S_FRAME, ao_radius=amb["radius"]), base["image_occluded"], base["mat_ids_occluded"],
             lambda img: AO.shade(img, amb["mask"], AM.S_FRAME, 0, n)),
            ("plain, area", dict(shadows=True, area=TA.S_FRAME, area_radius=a["radius"]),
             AR.shade(plain["image_unshadowed"], a["mask"], TA.S_FRAME, 0, n), plain["mat_ids"], None)):
        g = TI.cpu_gi(IR, ugrt, ci, w_img, w_ids, base["lcam"])
        got = cpu_display(F, **TI.GI_FRAME, **kw)
        np.testing.assert_array_equal(got["gi_sum"], g["sums"], err_msg=what)
        np.testing.assert_array_equal(got["gi_acc"], g["acc"], err_msg=what)
        np.testing.assert_array_equal(got["intersect_id"], w_ids, err_msg=what)
        np.testing.assert_array_equal(got["image"], g["image_gi"] if last is None else last(g["image_gi"]), err_msg=what)


def test_the_composer_returns_the_refract_files_frames(ugrt, O, REFS, RF, AO, AR, SR, K):
    """glass at 256 x 256: test_refract.cpu_frame at depth 4 (the levels through glass, the frame without and with
    reflect_shadows and its see-through flags, and under ao = 8), and the refract frame of depth 3 under an area light
    from test_area_light.cpu_area and test_area_sets.cpu_sets (the walk that sees through glass)."""
    s = RFR.scene(ugrt, "glass")
    F = FR.Frames(K, s, RFR.W, RFR.H)
    n = RFR.N
    want = RFR.cpu_frame(O, RF, REFS, ugrt, "glass", 4)
    kw = dict(shadows=True, reflect=True, refract=True, bounces=4)
    got = cpu_display(F, **kw)
    _assert_levels(got["levels"], want["levels"], False)
    np.testing.assert_array_equal(got["image"], want["image_depth"])
    np.testing.assert_array_equal(got["intersect_id"], want["mat_ids_depth"])
    np.testing.assert_array_equal(got["is_shadowed"], want["is_shadowed"])
    pr = want["primary"]
    radius = float(np.float32(0.05 * F.extent))
    orays, oactive = AO.rays(want["cam_pos"], pr["t"], pr["dir"], pr["id"], F.verts, F.faces, RFR.EPS, 0, n, n)
    mask = AM.cpu_mask(REFS[1], AO, want["ugrid"], F.verts, F.faces, orays, oactive, ugrt.scenes.ao_directions(RFR.AO_S), radius, 0, n, n)
    got = cpu_display(F, ao=RFR.AO_S, ao_radius=radius, **kw)
    np.testing.assert_array_equal(got["ao_mask"], mask)
    np.testing.assert_array_equal(got["image"], AO.shade(want["image_depth"], mask, RFR.AO_S, 0, n))
    got = cpu_display(F, reflect_shadows=True, **kw)
    _assert_levels(got["levels"], want["levels"], True)
    np.testing.assert_array_equal(got["image"], want["image_occluded"])
    np.testing.assert_array_equal(got["intersect_id"], want["mat_ids_occluded"])
    _assert_area_frames(ugrt, O, REFS, AO, AR, SR, RF, F, "glass")


# ------------------------------------------------------------------------------------------------------------ sharpness

PAIR_KW = dict(glossy=TG.GLOSSY_FRAME, area=dict(area=8, area_sets=16, area_filter=2), gi=TI.GI_FRAME, aa=dict(aa=4, aa_sets=16),
               ao=dict(ao=8, ao_sets=16, ao_filter=1))


def _changed(a, b):
    return (a.reshape(-1, 3) != b.reshape(-1, 3)).any(1)


def _passes(F, kw):
    """The byte passes of a frame one by one, as functions over an image, in the frame's order: (name, pass)."""
    kw = with_radii(F, kw)
    d = cpu_display(F, **kw)
    K, s, ids = F.K, F.scene, d["intersect_id"]
    P = FR.primary(F, F.setup)
    out = []
    if kw.get("glossy"):
        out.append(("glossy", lambda img: K.GL.apply(img, d["glossy_acc"], kw["glossy"], ids, s["reflect"], 0, N)))
    if kw.get("area"):
        out.append(("area", lambda img: K.SR.shade(img, d["area_vis"], kw["area"], 0, N)))
    else:
        def shadows(img):
            img = img.copy()
            K.O.add_shadows(img, P["hard"], 0, N)
            return img
        out.append(("shadows", shadows))
    if kw.get("gi"):
        out.append(("gi", lambda img: K.IR.apply(img, d["gi_acc"], kw["gi"], 1.0, ids, s["mat_list"], 0, N)))
    if kw.get("aa"):
        out.append(("aa", lambda img: K.AA.resolve(img, d["aa_sum"], kw["aa"], 0, N)))
    if kw.get("ao"):
        out.append(("ao", lambda img: K.ASR.shade(img, d["ao_vis"], kw["ao"], 0, N)))
    return out, d


def test_the_scenes_are_sharp(K):
    """Per scene and per pair of effects that can be on together: the pixels whose bytes both change (each against the
    frame without it) number at least FLOOR; and for each two neighbouring byte passes of a frame, running them in the
    other order changes at least FLOOR pixels.  The figures are printed and stand in the module's docstring."""
    figures = {}
    for scene, base in (("glossy", dict()), ("glass", BASES["refract3"])):
        F = frames(K, scene)
        shaded, _ = FR.shading_call(F, F.setup, dict(FR.DEFAULTS, **base))
        for a, b in itertools.combinations(FR.EFFECTS, 2):
            kw = dict(base, **PAIR_KW[a], **PAIR_KW[b])
            if not legal(bare(kw)):
                continue
            both = cpu_display(F, **with_radii(F, kw))["image"]
            without_a = cpu_display(F, **with_radii(F, dict(base, **PAIR_KW[b])))["image"]
            without_b = cpu_display(F, **with_radii(F, dict(base, **PAIR_KW[a])))["image"]
            figures[(scene, a, b, "both change")] = int((_changed(both, without_a) & _changed(both, without_b)).sum())
        # neighbouring passes the other way round, on every frame that holds them: a figure per chain of passes
        on = PAIR_KW
        chains = [dict(base, **on["area"], **on["gi"], **on["ao"]), dict(base, **on["gi"], **on["ao"]), dict(base, **on["ao"]),
                  dict(base, **on["area"], **on["ao"])]
        if scene == "glossy":
            chains += [dict(on["glossy"], **on["gi"], **on["ao"]), dict(on["glossy"], **on["area"], **on["gi"], **on["ao"]),
                       dict(on["glossy"], **on["ao"]), dict(on["aa"], **on["ao"])]
        for kw in chains:
            passes, d = _passes(F, kw)
            chain = " ".join(name for name, _ in passes)
            img = shaded
            for name, p in passes:
                img = p(img)
            np.testing.assert_array_equal(img, d["image"])  # the passes one by one are the frame
            for i in range(len(passes) - 1):
                order = passes[:i] + [passes[i + 1], passes[i]] + passes[i + 2:]
                img = shaded
                for name, p in order:
                    img = p(img)
                figures[(scene, passes[i][0], passes[i + 1][0], "swapped in " + chain)] = int(_changed(img, d["image"]).sum())
    for key in sorted(figures):
        print("%-7s %-8s %-8s %-36s %5d" % (key + (figures[key],)))
    assert min(figures.values()) >= FLOOR, {k: v for k, v in figures.items() if v < FLOOR}
    pairs = {k[:3] for k in figures if k[3].startswith("swapped")}
    every = {("shadows", "gi"), ("shadows", "ao"), ("area", "gi"), ("area", "ao"), ("gi", "ao")}
    assert pairs == {("glass",) + p for p in every} | {("glossy",) + p for p in every | {
        ("glossy", "shadows"), ("glossy", "area"), ("shadows", "aa"), ("aa", "ao")}}


# ------------------------------------------------------------------------------------------------------------------ GPU


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available()
    return torch


def _compare(F, r, ctx, setup, kw, what, chain=None, cpu=True, only=None):
    ctx.synchronize()
    got = device_frame(r, setup, **kw)
    if cpu:
        bad = differences(cpu_display(F, setup, chain=chain, **kw), got, only)
        assert not bad, (what, kw, bad)
    return got


# the calls that open one "reflect_gen" bracket each, and those that open one "shade" bracket each (the feature files pin that)
RAY_CALLS = {"reflect_rays", "refract_rays", "reflect_rays_next", "refract_rays_next", "occlusion_rays", "ao_rays"}
SHADE_CALLS = {"shade_simple", "shade_spotlight", "shade_reflect", "shade_reflect_depth", "shade_reflect_depth_occluded", "shade_lights",
               "shade_reflect_lights", "shade_add_shadows", "shade_ao", "shade_ao_vis", "shade_area", "shade_area_vis", "gi_apply",
               "aa_resolve", "aa_edges", "glossy_apply", "filter_visibility", "gi_filter", "temporal_visibility", "temporal_gi"}
STALE = ("ao_rays", "ao_active", "ao_mask", "ao_vis", "area_mask", "area_vis", "gi_sum", "gi_acc", "glossy_sum", "glossy_acc", "aa_edge",
         "aa_sum")


def _frame(F, r, ctx, setup, kw, what, num_lights=0):
    """One frame of the matrix.  Before it, whatever an earlier frame left in the effects' buffers is overwritten (NaN
    origins, no active pixel, all-ones words), so that a frame which skips a call of its own does not find an equal frame's
    values there; behind it, the whole dict is the CPU's and the frame opened as many ray-generator and shading brackets
    as predicted() names such calls."""
    for name in STALE:
        buf = getattr(r, name, None)
        if buf is not None:
            buf.fill_(float("nan") if name == "ao_rays" else 0 if name == "ao_active" else -1)
    ctx.prof_reset()
    r.display(setup, **kw)
    _compare(F, r, ctx, setup, kw, what)
    names, prof = predicted(kw, num_lights), ctx.prof_get()
    assert prof["reflect_gen"][1] == sum(n in RAY_CALLS for n in names), (what, kw, prof["reflect_gen"])
    assert prof["shade"][1] == sum(n in SHADE_CALLS for n in names), (what, kw, prof["shade"])


@pytest.mark.gpu
@pytest.mark.parametrize("shadows", [True, False], ids=["shadows", "no_shadows"])
@pytest.mark.parametrize("base", list(BASES))
def test_every_legal_frame_equals_the_cpu_frame(K, torch, base, shadows):
    """One fresh renderer per parameter walks the base's legal frames in matrix()'s order: after each, every entry of
    cpu_display's dict is the device's, bit for bit."""
    F = frames(K, SCENE_OF.get(base, "glossy"))
    ctx, r = F.make()
    ctx.prof_enable(True, stages=("shade", "reflect_gen"))
    todo = matrix(BASES[base], shadows)
    assert len(todo) >= 9
    for kw in todo:
        _frame(F, r, ctx, F.setup, with_radii(F, kw), base)


@pytest.mark.gpu
def test_every_legal_frame_under_several_lights_equals_the_cpu_frame(K, torch):
    """setup.lights and reflect_lights (depth 3, reflect_shadows) under three lights x the three ao values x shadows."""
    F = frames(K, "glossy")
    setup = K.ugrt.FrameSetup.from_scene(F.scene, lights=TL.lights_for(F.scene, 3))
    ctx, r = F.make()
    ctx.prof_enable(True, stages=("shade", "reflect_gen"))
    for base in MULTI:
        for shadows in (True, False):
            for kw in matrix(MULTI[base], shadows, lights=True):
                _frame(F, r, ctx, setup, with_radii(F, kw), base, 3)


SEQUENCES = {
    "plain, ao + aa": ("glossy", dict(ao=4, ao_sets=16, ao_filter=1, aa=4, aa_sets=16)),
    "plain, ao + area + gi": ("glossy", dict(TT.FRAMES["ao"], **TT.FRAMES["area"], **TT.FRAMES["gi"])),
    "reflect1, area + gi": ("glossy", dict(BASES["reflect1"], **TT.FRAMES["area"], **TT.FRAMES["gi"])),
    "refract3, area + ao": ("glass", dict(BASES["refract3"], **TT.FRAMES["area"], **TT.FRAMES["ao"])),
}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(SEQUENCES))
def test_temporal_sequences_equal_the_cpu_chain(K, torch, which):
    """Three frames under test_temporal._moved's camera.  Every mask is the CPU walk over scenes.temporal_sets' table of
    that frame; the gathers' sums, the histories, the output pairs and the image follow from them on the CPU alone."""
    scene, kw = SEQUENCES[which]
    F = frames(K, scene)
    kw = with_radii(F, dict(kw, temporal=8))
    ctx, r = F.make()
    chain = FR.Chain()
    step = np.float64([0.004, -0.003, 0.002]) * F.extent
    for f in range(3):
        setup = TT._moved(K.ugrt, F.setup, f, step)
        r.display(setup, **kw)
        got = _compare(F, r, ctx, setup, kw, "%s, frame %d" % (which, f), chain=chain)
        assert set(got["history"]) == {n for n in ("ao", "area", "gi") if kw.get(n)}
    assert all(n == 3 for n in chain.n.values())


def _walk(F, rng):
    """The steps of the long-lived renderer's walk: ("display", setup name, keywords) and ("call", name)."""
    on = {n: with_radii(F, kw) for n, kw in PAIR_KW.items()}
    steps = []

    def show(kw, setup="s0"):
        if not steps or steps[-1] != ("display", setup, kw):
            steps.append(("display", setup, kw))

    # every effect goes off -> on and on -> off behind every other effect
    for a, b in itertools.permutations(FR.EFFECTS, 2):
        both = dict(on[a], **on[b])
        show(on[b])
        show(both if legal(bare(both)) else on[a])
        show(on[b])
    # every S, sets, filter and radius changes while its effect stays on (and another effect beside it)
    beside = dict(ao=on["gi"], area=on["ao"], gi=on["area"], glossy=on["ao"], aa=on["ao"])
    for e, changes in (("ao", (dict(ao=5), dict(ao_sets=4), dict(ao_filter=2), dict(ao_radius=on["ao"]["ao_radius"] * 2))),
                       ("area", (dict(area=5), dict(area_sets=4), dict(area_filter=1), dict(area_radius=on["area"]["area_radius"] / 2))),
                       ("gi", (dict(gi=5), dict(gi_sets=4), dict(gi_filter=1), dict(gi_radius=F.extent / 4))),
                       ("glossy", (dict(glossy=5), dict(glossy_sets=4), dict(glossy_filter=1), dict(glossy_radius=F.extent / 4))),
                       ("aa", (dict(aa=8), dict(aa_sets=4)))):
        show(dict(on[e], **beside[e]))
        for change in changes:
            show(dict(on[e], **beside[e], **change))
            show(dict(on[e], **beside[e]))
    every = dict(on["glossy"], **on["area"], **on["gi"], **on["ao"])
    show(every)
    show(every, "light")      # a light move
    show(every, "camera")     # a camera move
    show(every)
    steps.append(("display", "s0", dict(every, shade=False)))
    show(every)
    steps.append(("raises", "s0", dict(every, aa=4)))
    show(every)
    # temporal entered, left and entered again; the bases with levels in between
    t = dict(on["area"], **on["gi"], **on["ao"], temporal=8)
    for setup in ("s0", "camera", "s0"):
        show(t, setup)
    show(dict(on["ao"], **BASES["reflect3"]))
    for setup in ("s0", "camera"):
        show(dict(t, **BASES["reflect1"]), setup)
    show(dict(on["area"], **on["gi"], **BASES["refract3"]))
    show(every)
    steps.append(("call", "rotate_bunny", None))
    show(every)
    show(t)
    show(t, "camera")
    steps.append(("call", "geometry_changed", None))
    show(t)
    show(every)
    # seeded picks from the matrix, so that no two runs of frames above are all there is
    pool = [with_radii(F, kw) for b in ("plain", "reflect3") for sh in (True, False) for kw in matrix(BASES[b], sh)]
    for i in rng.choice(len(pool), 8, replace=False):
        show(pool[i])
    return steps


@pytest.mark.gpu
@pytest.mark.parametrize("static", [False, True], ids=["rebuild", "static_geometry"])
def test_a_long_lived_renderer_equals_a_fresh_one(K, torch, static):
    """One renderer (with and without FLAG_STATIC_GEOMETRY) through _walk's steps.  After each display the whole frame
    equals a fresh renderer's for the same geometry, setup and keywords (a temporal run is replayed on the fresh renderer
    from its first frame), and, while the geometry is the scene's, the CPU frame where the step is not a temporal one."""
    ugrt = K.ugrt
    F = frames(K, "glossy")
    flags = ugrt.FLAG_STATIC_GEOMETRY if static else 0
    s0 = F.setup
    ext = F.extent
    setups = dict(s0=s0, camera=TT._moved(ugrt, s0, 1, np.float64([0.004, -0.003, 0.002]) * ext),
                  light=ugrt.FrameSetup(s0.camera, dict(s0.light_camera, eye=tuple(np.float64(s0.light_camera["eye"]) + 0.05 * ext)),
                                        tuple(np.float64(s0.shading_light) + 0.05 * ext)))
    ctx, r = F.make(flags)
    r.init_orig_list(8, 16)
    moved = False
    run = []  # the temporal run that is going on: its (setup name, keywords)
    steps = _walk(F, np.random.RandomState(2024))
    shown = 0
    for i, (what, name, kw) in enumerate(steps):
        if what == "call":
            if name == "rotate_bunny":
                r.rotate_bunny(0.05)
            else:
                r.d_verts[3 * 16:3 * 24] += 0.01 * ext
                r.geometry_changed()
            moved, run = True, []
            continue
        if what == "raises":
            with pytest.raises(ValueError):
                r.display(setups[name], **kw)
            continue
        r.display(setups[name], **kw)
        shown += 1
        temporal = bool(kw.get("temporal")) and kw.get("shade", True)
        run = run + [(name, kw)] if temporal else []
        fctx, fresh = F.make(flags)
        if moved:
            fresh.d_verts.copy_(r.d_verts)
            fresh.geometry_changed()
        for n2, kw2 in (run or [(name, kw)]):
            fresh.display(setups[n2], **kw2)
        ctx.synchronize()
        fctx.synchronize()
        if not kw.get("shade", True):
            for n in ("intersect_id", "is_shadowed"):
                assert torch.equal(getattr(r, n), getattr(fresh, n)), (i, kw)
            continue
        got = device_frame(r, setups[name], **{n: v for n, v in kw.items() if n in FR.DEFAULTS or n in FR.MORE})
        want = device_frame(fresh, setups[name], **{n: v for n, v in kw.items() if n in FR.DEFAULTS or n in FR.MORE})
        bad = differences(want, got)
        assert not bad, (i, name, kw, bad)
        if not moved and not temporal and name == "s0":
            bad = differences(cpu_display(F, setups[name], **kw), got)
            assert not bad, (i, name, kw, bad, "against the CPU frame")
    assert shown >= 60
