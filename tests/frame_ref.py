"""The CPU composer of Renderer.display(): which keyword sets are legal, and everything a legal frame leaves behind.

legal() restates the display() docstring and DESIGN.md sections 6.1-6.14; it calls no check_*.  Every rule carries the
words of the docstring it comes from (RULES), which tests/test_frame_matrix.py looks up in the docstring.

cpu_display() strings the checkers the suite already has (the oracle and the plain-C restatements next to it) into one
frame, in the order DESIGN.md section 6.14 gives the byte passes:

    the shading call -> glossy_apply -> shade_add_shadows | shade_area | shade_area_vis -> gi_apply -> aa_resolve ->
    shade_ao | shade_ao_vis

The words of an effect (masks, gathered sums) depend on the primary hits and on the effect's own parameters only, so they
are computed once per (camera, light, effect parameters, refract) and shared; the composition on top is byte passes.
Nothing here reads the device: a Chain carries a temporal sequence's histories from frame to frame on the CPU."""
import numpy as np

import test_ambient as AM
import test_area_light as TA
import test_reflect_depth as RD
import test_reflect_lights as RLT
import test_refract as RFR

_f32, _i32, bits, LG, UD = RD._f32, RD._i32, RD.bits, RD.LG, RD.UD
EPS = 1e-3
COS = float(np.float32(0.9))
INF = float("inf")
TILE = {1: (1, 1), 4: (2, 2), 16: (4, 4)}
KINDS = ("one", "two", "banded")  # Renderer, a two-stream Renderer, BandedRenderer

# what legal() looks at, with display()'s defaults; "lights": the setup carries FrameSetup.lights
DEFAULTS = dict(lights=False, frame_cnt=1, shadows=True, reflect=False, bounces=1, reflect_shadows=False, reflect_lights=False,
                refract=False, ao=0, ao_sets=1, ao_filter=0, area=0, area_sets=1, area_filter=0, gi=0, gi_sets=1, gi_filter=0,
                aa=0, aa_sets=1, temporal=0, glossy=0, glossy_sets=1, glossy_filter=0)

# (name, the docstring's words, the keyword sets the rule excludes)
RULES = (
    ("reflect_shadows needs reflect", "reflect_shadows (needs reflect=True)",
     lambda k, kind: k["reflect_shadows"] and not k["reflect"]),
    ("refract needs reflect", "refract (needs reflect=True",
     lambda k, kind: k["refract"] and not k["reflect"]),
    ("reflect_lights needs reflect and lights", "reflect_lights (one-stream renderer; needs reflect=True and setup.lights)",
     lambda k, kind: k["reflect_lights"] and not (k["reflect"] and k["lights"] and kind == "one")),
    ("lights", "setup.lights (one-stream renderer, reflect=False)",
     lambda k, kind: k["lights"] and (kind != "one" or (k["reflect"] and not k["reflect_lights"]))),
    ("ao", "ao (one-stream renderer, every frame above",
     lambda k, kind: k["ao"] and kind != "one"),
    ("ao_sets", "ao_sets (needs ao > 0",
     lambda k, kind: k["ao_sets"] != 1 and not k["ao"]),
    ("ao_filter", "ao_filter (needs ao > 0",
     lambda k, kind: k["ao_filter"] and not k["ao"]),
    ("area", "area (one-stream renderer, single-light frames, needs shadows=True",
     lambda k, kind: k["area"] and (kind != "one" or k["lights"] or not k["shadows"])),
    ("area_sets", "area_sets (needs area > 0",
     lambda k, kind: k["area_sets"] != 1 and not k["area"]),
    ("area_filter", "area_filter (needs area > 0",
     lambda k, kind: k["area_filter"] and not k["area"]),
    ("gi", "gi (one-stream renderer, single-light frames, plain or reflect, with or without refract; ao and area compose",
     lambda k, kind: k["gi"] and (kind != "one" or k["lights"])),
    ("gi_sets, gi_filter", "gi_sets and gi_filter (need gi > 0",
     lambda k, kind: (k["gi_sets"] != 1 or k["gi_filter"]) and not k["gi"]),
    ("aa", "aa (one-stream renderer, the single-light plain frame: reflect=False, frame_cnt < 2, no setup.lights, area or gi",
     lambda k, kind: k["aa"] and (kind != "one" or k["reflect"] or k["frame_cnt"] >= 2 or k["lights"] or k["area"] or k["gi"])),
    ("aa_sets", "aa_sets (needs aa > 0",
     lambda k, kind: k["aa_sets"] != 1 and not k["aa"]),
    ("temporal", "temporal (one-stream renderer, single-light frames, plain, reflect or refract; needs ao, area or gi",
     lambda k, kind: k["temporal"] and (kind != "one" or k["lights"] or not (k["ao"] or k["area"] or k["gi"]))),
    ("glossy", "glossy (one-stream renderer, single-light frames with reflect=False; ao, area and gi compose; no aa, no temporal",
     lambda k, kind: k["glossy"] and (kind != "one" or k["lights"] or k["reflect"] or k["aa"] or k["temporal"])),
    ("glossy_sets, glossy_filter", "glossy_sets and glossy_filter (need glossy > 0",
     lambda k, kind: (k["glossy_sets"] != 1 or k["glossy_filter"]) and not k["glossy"]),
)


def why_not(kw, renderer_kind="one"):
    """The name of the first rule of RULES that excludes the keyword set, or None: the frame is legal."""
    assert renderer_kind in KINDS and not set(kw) - set(DEFAULTS), (renderer_kind, set(kw) - set(DEFAULTS))
    k = dict(DEFAULTS, **kw)
    for name, _, excludes in RULES:
        if excludes(k, renderer_kind):
            return name
    return None


def legal(kw, renderer_kind="one"):
    """True where display() of a Renderer ("one"), of a two-stream Renderer ("two") or of a BandedRenderer ("banded")
    takes the keyword set; kw: keywords of DEFAULTS ("lights": the setup carries FrameSetup.lights)."""
    return why_not(kw, renderer_kind) is None


# the effects in the order of their byte passes, and which pairs can be on together on a one-stream single-light frame
EFFECTS = ("glossy", "area", "gi", "aa", "ao")


def table_rows():
    """The "what composes with what" table of DESIGN.md section 6.14 as text lines, from legal()."""
    frames = (("plain", dict()), ("plain, frame_cnt 2", dict(frame_cnt=2)), ("shadows=False", dict(shadows=False)),
              ("reflect", dict(reflect=True)), ("reflect + refract", dict(reflect=True, refract=True)),
              ("setup.lights", dict(lights=True)), ("reflect_lights", dict(lights=True, reflect=True, reflect_lights=True)),
              ("two-stream", "two"), ("banded", "banded"))
    cols = EFFECTS + ("temporal",)
    on = dict(glossy=dict(glossy=8), area=dict(area=8), gi=dict(gi=8), aa=dict(aa=4), ao=dict(ao=8), temporal=dict(temporal=8, ao=8))
    mark = lambda ok: "yes" if ok else "-"
    rows = ["| with | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    for name, base in frames:
        kind, base = (base, {}) if isinstance(base, str) else ("one", base)
        rows.append("| %s | " % name + " | ".join(mark(legal(dict(base, **on[c]), kind)) for c in cols) + " |")
    for a in cols:
        rows.append("| %s | " % a + " | ".join(mark(legal(dict(on[a], **on[c]))) for c in cols) + " |")
    return rows


# ------------------------------------------------------------------------------------------------------- the composer


class Checkers:
    """The suite's checkers in one place: the oracle and the restatements' fixtures, by the names the test modules use."""

    def __init__(self, ugrt, O, REFS, RF, AO, AR, SR, ASR, IR, GL, AA, TR, LT, RL):
        self.ugrt, self.O, self.REF, self.OC, self.RF, self.AO, self.AR, self.SR, self.ASR = ugrt, O, REFS[0], REFS[1], RF, AO, AR, SR, ASR
        self.IR, self.GL, self.AA, self.TR, self.LT, self.RL = IR, GL, AA, TR, LT, RL
        self.rmod = RLT._rmod(ugrt)


class Frames:
    """F of cpu_display: a scene at W x H, the spreads of its materials, and the caches of everything computed for it."""

    def __init__(self, K, scene, W, H, spread=None, setup=None):
        s = dict(scene)
        m = len(np.asarray(s["reflect"]))
        s.setdefault("transmit", np.zeros(m, np.float32))
        s.setdefault("ior", np.ones(m, np.float32))
        s["continue"] = np.where(s["transmit"] > 0, s["transmit"], s["reflect"]).astype(np.float32)
        self.K, self.scene, self.W, self.H, self.N = K, s, W, H, W * H
        self.spread = np.zeros(m, np.float32) if spread is None else np.asarray(spread, np.float32)
        self.verts, self.faces = _f32(s["verts"]).reshape(-1), _i32(s["faces"]).reshape(-1)
        v3 = self.verts.reshape(-1, 3)
        self.bbmin, self.bbmax = v3.min(0), v3.max(0)
        self.plane = K.rmod.default_filter_plane(self.bbmin, self.bbmax)
        self.extent = float((self.bbmax - self.bbmin).max())
        self.ugrid = K.O.grid_uniform(s["faces"], s["verts"], self.bbmin, self.bbmax, UD)
        self.thru = RFR.filtered_grid(self.ugrid, RFR.see_through(s))
        self.setup = K.ugrt.FrameSetup.from_scene(s) if setup is None else setup
        self.cache = {}

    def make(self, flags=0):
        """(context, a fresh one-stream Renderer) of the scene, as the frames' test modules make theirs."""
        u, s = self.K.ugrt, self.scene
        ctx = u.Context(self.W, self.H, light_grid=LG, flags=u.FLAG_SHADOW_ALL_CHUNKS | flags, uniform_dims=UD)
        return ctx, u.Renderer(ctx, s["verts"], s["faces"], s["matidx"], s["mat_list"], s["reflect"], s["transmit"], s["ior"],
                               spread=self.spread)

    def once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]


def _cam_key(params):
    return tuple((k, tuple(np.float64(params[k]).reshape(-1))) for k in ("eye", "look", "up", "near", "far"))


def _setup_key(setup):
    lights = getattr(setup, "lights", None)
    return (_cam_key(setup.camera), _cam_key(setup.light_camera), tuple(np.float64(setup.shading_light)), float(setup.fovy),
            None if lights is None else tuple((_cam_key(p), tuple(np.float64(pos))) for p, pos in lights))


def primary(F, setup):
    """The camera pass and the shadow stage(s) of a setup: the oracle's plain frame (every chunk traced), {o', n} of the
    primary hits, the light's point, and with setup.lights per light its camera block, position and flags."""
    def make():
        K, s, W, H, N = F.K, F.scene, F.W, F.H, F.N
        O = K.O
        want = O.frame(s, setup, W, H, light_grid=LG, all_chunks=True, shadows=True)
        pr = want["primary"]
        cam_pos = want["cam"].worldori[:3].copy()
        orays, oactive = K.AO.rays(cam_pos, pr["t"], pr["dir"], pr["id"], F.verts, F.faces, EPS, 0, N, N)
        p = dict(pr=pr, cam=want["cam"], lcam=want["lcam"], cam_pos=cam_pos, light=want["lcam"].worldori[:3].copy(),
                 hard=want["is_shadowed"], untouched=pr["shadowed"].copy(), orays=orays, oactive=oactive,
                 cc=np.array(K.rmod.make_camera(setup.camera, setup.fovy, float(np.float32(W) / np.float32(H))).camcoords, np.float32))
        if getattr(setup, "lights", None) is not None:
            aspect, (lx, ly) = float(np.float32(W) / np.float32(H)), LG
            per = []
            for params, pos in setup.lights:
                lcam = O.cam_from(params, setup.fovy, aspect)
                d_map = O.map_rays(lcam.cc, pr["t"], pr["dir"], cam_pos, lx, ly, 0, N)
                lgrid = O.grid_spherical(lcam.cc, F.faces, F.verts, lx, ly)
                prefix, nchunks = O.process_rays(d_map, N, lx * ly + 1, N // 64 + lx * ly + 2)
                flags = np.zeros(N, np.int32)
                O.trace_shadow(lcam.cc, lgrid, lx * ly, F.verts, F.faces, pr["t"], pr["dir"], flags, d_map, prefix, cam_pos, nchunks,
                               (W // 8) * (H // 8), N, strict=False)
                per.append(dict(cc=lcam.cc.copy(), pos=pos, flags=flags, eye=lcam.worldori[:3].copy()))
            p["lights"] = per
        return p
    return F.once(("primary", _setup_key(setup)), make)


def levels(F, setup, refract, depth, occluded):
    """The reflection levels 1..depth of a frame (a refract frame: through glass), with `occluded` every level's flags
    towards the light camera's eye (a refract frame: through the grid without the glass), or under setup.lights towards
    every light's eye, [L, N] per level."""
    def make():
        K, s, N, P = F.K, F.scene, F.N, primary(F, setup)
        pr, out = P["pr"], []
        mats = (s["matidx"], s["reflect"], s["transmit"], s["ior"])
        for j in range(depth):
            if j == 0 and refract:
                rays, active, _ = K.RF.refract_rays(P["cam_pos"], pr["t"], pr["dir"], pr["id"], *mats, F.verts, F.faces, EPS, 0, N, N)
            elif j == 0:
                rays, active = K.O.reflect_rays(P["cam_pos"], pr["t"], pr["dir"], pr["id"], s["matidx"], s["reflect"], F.verts,
                                                F.faces, EPS, 0, N, N)
            elif refract:
                lv = out[-1]
                rays, active, _ = K.RF.refract_rays_next(lv["rays"], lv["active"], lv["hit_t"], lv["hit_id"], *mats, F.verts,
                                                         F.faces, EPS, 0, N, N)
            else:
                lv = out[-1]
                rays, active = K.REF.reflect_rays_next(lv["rays"], lv["active"], lv["hit_t"], lv["hit_id"], s["matidx"],
                                                       s["reflect"], F.verts, F.faces, EPS, 0, N, N)
            hit_t, hit_id, _ = K.O.trace_dda(F.ugrid, F.verts, F.faces, rays, active, 0, N, N)
            lv = dict(rays=rays, active=active, hit_t=hit_t, hit_id=hit_id)
            if occluded:
                grid = F.thru if refract else F.ugrid
                eyes = [lt["eye"] for lt in P["lights"]] if "lights" in P else [P["light"]]
                flags = []
                for eye in eyes:
                    o_r, o_a = K.OC.occlusion_rays(rays, active, hit_t, hit_id, F.verts, F.faces, eye, EPS, 0, N, N)
                    flags.append(K.OC.trace_any(grid, F.verts, F.faces, o_r, o_a, 1.0, 0, N, N))
                lv["occluded"] = np.stack(flags) if "lights" in P else flags[0]
            out.append(lv)
        return out
    return F.once(("levels", _setup_key(setup), refract, depth, occluded), make)


def shading_call(F, setup, k):
    """(image, material ids) behind the frame's shading call, before any other pass: shade_simple | shade_spotlight |
    shade_reflect | shade_reflect_depth | shade_reflect_depth_occluded | shade_lights | shade_reflect_lights, with the
    light camera's block current (the last light's under setup.lights), shadows or not."""
    key = ("shaded", _setup_key(setup), k["frame_cnt"] >= 2, k["shadows"] and k["lights"], k["reflect"], k["refract"], k["bounces"],
           k["reflect_shadows"], k["reflect_lights"])

    def make():
        K, s, N, P = F.K, F.scene, F.N, primary(F, setup)
        pr = P["pr"]
        front = (pr["normal"], pr["t"], pr["dir"], pr["id"], P["cam_pos"], s["matidx"], s["mat_list"])
        weights = s["continue"] if k["refract"] else s["reflect"]
        if k["reflect"]:
            lv = levels(F, setup, k["refract"], k["bounces"], k["reflect_shadows"])
            stack = {n: np.concatenate([l[n] for l in lv]) for n in ("rays", "active", "hit_t", "hit_id")}
            chain = (weights, F.verts, F.faces, k["bounces"], stack["rays"], stack["active"], stack["hit_t"], stack["hit_id"])
        if k["reflect_lights"]:
            per = P["lights"]
            flags = np.stack([lt["flags"] for lt in per]) if k["shadows"] else None
            occluded = np.stack([l["occluded"] for l in lv]) if k["reflect_shadows"] else None
            return K.RL.shade(per[-1]["cc"], *front, *chain, [lt["pos"] for lt in per], flags, occluded, 0, N, N)
        if k["lights"]:
            per = P["lights"]
            flags = np.stack([lt["flags"] for lt in per]) if k["shadows"] else None
            return K.LT.shade_lights(per[-1]["cc"], *front, [lt["pos"] for lt in per], flags, 0, N, N)
        cc = P["lcam"].cc
        if k["reflect"] and k["reflect_shadows"]:
            return K.OC.shade_depth_occluded(cc, setup.shading_light, *front, *chain, np.concatenate([l["occluded"] for l in lv]), 0, N, N)
        if k["reflect"] and k["bounces"] > 1:
            return K.REF.shade_depth(cc, setup.shading_light, *front, *chain, 0, N, N)
        img, ids = np.zeros(3 * N, np.uint8), pr["id"].copy()
        if k["reflect"]:
            K.O.shade_reflect(cc, setup.shading_light, img, pr["normal"], pr["t"], pr["dir"], ids, P["cam_pos"], s["matidx"],
                              s["mat_list"], weights, F.verts, F.faces, lv[0]["rays"], lv[0]["active"], lv[0]["hit_t"],
                              lv[0]["hit_id"], 0, N)
        else:
            K.O.shade(cc, setup.shading_light, img, pr["normal"], pr["t"], pr["dir"], ids, P["cam_pos"], s["matidx"], s["mat_list"],
                      0, N, spot=k["frame_cnt"] >= 2)
        return img, ids
    return F.once(key, make)


def _set_mask(F, setup, kind, row, limit, thru):
    """One set's mask word per pixel: the hemisphere walk along the directions `row` up to `limit` ("ao"), or the walk
    towards the points `row` of the light's disk ("area"; thru: through the grid without the glass)."""
    def make():
        K, P, N = F.K, primary(F, setup), F.N
        if kind == "ao":
            return AM.cpu_mask(K.OC, K.AO, F.ugrid, F.verts, F.faces, P["orays"], P["oactive"], row, limit, 0, N, N)
        return TA.cpu_mask(K.OC, K.AR, F.thru if thru else F.ugrid, F.verts, F.faces, P["orays"], P["oactive"], row, 0, N, N)
    return F.once((kind + " set", _setup_key(setup), bits(_f32(row)).tobytes(), limit, thru), make)


def sets_mask(F, setup, kind, table, limit=None, thru=False):
    """The mask of a walk over the sets of `table` [sets, S, 3]: every set's mask, selected per pixel of the tile."""
    per_set = np.stack([_set_mask(F, setup, kind, row, limit, thru) for row in table])
    tile = TILE[len(table)]
    return per_set[0] if len(table) == 1 else F.K.SR.select(per_set, tile[0], tile[1], F.W, F.H)


def area_table(F, setup, S, sets, radius):
    lc = setup.light_camera
    eye = np.asarray(lc["eye"], np.float64)
    axis = np.asarray(lc["look"], np.float64) - eye
    sc = F.K.ugrt.scenes
    return sc.area_samples(S, eye, axis, radius)[None] if sets == 1 else sc.area_sample_sets(S, sets, eye, axis, radius)


def ao_table(F, S, sets):
    sc = F.K.ugrt.scenes
    return sc.ao_directions(S)[None] if sets == 1 else sc.ao_direction_sets(S, sets)


def gi_sums(F, setup, S, sets, table, radius, shadows):
    def make():
        K, s, P, N = F.K, F.scene, primary(F, setup), F.N
        return K.IR.gather(F.ugrid, F.verts, F.faces, P["orays"], P["oactive"], S, TILE[sets], table, F.W, radius, s["matidx"],
                           s["mat_list"], P["lcam"].cc, setup.shading_light, P["light"] if shadows else None, EPS, 0, N, N)
    return F.once(("gi", _setup_key(setup), S, sets, bits(_f32(table)).tobytes(), radius, shadows), make)


def glossy_sums(F, setup, S, sets, radius, shadows):
    """(level 1's rays, their flags, the lobe's sums)."""
    def make():
        K, s, P, N = F.K, F.scene, primary(F, setup), F.N
        lv = levels(F, setup, False, 1, False)[0]
        sums = K.GL.gather(F.ugrid, F.verts, F.faces, lv["rays"], lv["active"], P["orays"], P["pr"]["id"], s["matidx"], F.spread, S,
                           TILE[sets], K.ugrt.scenes.glossy_point_sets(S, sets), F.W, radius, s["mat_list"], P["lcam"].cc,
                           setup.shading_light, P["light"] if shadows else None, EPS, 0, N, N)
        return lv["rays"], lv["active"], sums
    return F.once(("glossy", _setup_key(setup), S, sets, radius, shadows), make)


def aa_words(F, setup, S, sets, with_shadows, cos=COS):
    """(edge flags, sums) of the anti-aliasing; with_shadows: the frame has a shadow stage and aa_shadows is on."""
    def make():
        K, s, P = F.K, F.scene, primary(F, setup)
        edge = K.AA.edges(P["pr"], P["cam_pos"], s["matidx"], P["hard"] if with_shadows else None, cos, F.plane, F.W, F.H, 0, F.N)
        sums = K.AA.gather(F.ugrid, s["verts"], s["faces"], P["cam"], False, F.W, F.H, edge, S, TILE[sets],
                           K.ugrt.scenes.aa_offset_sets(S, sets), s["matidx"], s["mat_list"], P["lcam"].cc, setup.shading_light,
                           P["light"] if with_shadows else None, EPS, 0, F.N)
        return edge, sums
    return F.once(("aa", _setup_key(setup), S, sets, with_shadows, cos), make)


class Chain:
    """A temporal sequence on the CPU: the G-buffer and eye of the frame before, and per effect its history and the number
    of frames it has seen.  It follows an uninterrupted sequence whose effects and parameters stay what they are."""

    def __init__(self):
        self.prev = None  # (orays, oactive, the eye's block)
        self.hist, self.n, self.key = {}, {}, {}

    def blend(self, F, name, P, key, sums, S, tp):
        """One effect's temporal call: (history, output words) from this frame's gathered sums."""
        assert self.key.setdefault(name, key) == key, "a Chain follows one set of parameters"
        C_, CW = (3, 4) if name == "gi" else (1, 2)
        N = F.N
        prev = self.prev if self.prev is not None else (np.zeros(6 * N, np.float32), np.zeros(N, np.int32), P["cc"])
        hist, out, _ = F.K.TR.blend(C_, sums, S, P["orays"], P["oactive"], prev[2], prev[0], prev[1],
                                    self.hist.get(name, np.zeros(CW * N, np.float32)), tp[0], tp[1], tp[2], F.W, F.H)
        self.hist[name] = hist
        self.n[name] = self.n.get(name, 0) + 1
        return hist, out


# every keyword cpu_display takes besides legal()'s, with display()'s defaults
MORE = dict(ao_radius=None, area_radius=None, gi_radius=None, gi_gain=1.0, gi_shadows=True, aa_shadows=True, glossy_radius=None,
            glossy_shadows=True, temporal_cos=0.9, temporal_plane=None)


def cpu_display(F, setup=None, chain=None, **kw):
    """Everything display(setup, **kw) on a fresh one-stream Renderer of F leaves behind, by the renderer's attribute names:
    image, intersect_id, is_shadowed and the arrays of every effect that is on; "levels" (per level rays, active, hit_t,
    hit_id and, with reflect_shadows, occluded); "shadowed_lights" under setup.lights; under temporal (chain: the
    sequence's Chain, which this call advances) the gathers' sums, ao_tvis / area_tvis / gi_tacc and "history" per
    effect."""
    setup = F.setup if setup is None else setup
    k = dict(DEFAULTS, **MORE)
    assert not set(kw) - set(k), set(kw) - set(k)
    k.update(kw, lights=getattr(setup, "lights", None) is not None)
    assert legal({n: k[n] for n in DEFAULTS}), why_not({n: k[n] for n in DEFAULTS})
    K, s, N, W, H = F.K, F.scene, F.N, F.W, F.H
    P = primary(F, setup)
    out = {}
    tp = None
    if k["temporal"]:
        assert chain is not None
        tp = (k["temporal"], float(np.float32(k["temporal_cos"])), F.plane if k["temporal_plane"] is None else k["temporal_plane"])
    hard = k["shadows"] and not k["area"]
    img, ids = shading_call(F, setup, k)
    img = img.copy()
    out["intersect_id"] = ids
    if k["lights"]:
        out["is_shadowed"] = P["untouched"]
        if k["shadows"]:
            out["shadowed_lights"] = np.stack([lt["flags"] for lt in P["lights"]])
    else:
        out["is_shadowed"] = P["hard"] if hard else P["untouched"]
    if k["reflect"]:
        out["levels"] = levels(F, setup, k["refract"], k["bounces"], k["reflect_shadows"])
    if k["ao"] or k["area"] or k["gi"] or k["glossy"]:
        out["ao_rays"], out["ao_active"] = P["orays"], P["oactive"]
    # -- glossy_apply, directly behind the shading call
    if k["glossy"]:
        S = k["glossy"]
        rays, active, sums = glossy_sums(F, setup, S, k["glossy_sets"], INF if k["glossy_radius"] is None else k["glossy_radius"],
                                         k["glossy_shadows"])
        out["levels"] = [dict(rays=rays, active=active)]
        out["glossy_sum"] = acc = sums
        if k["glossy_filter"]:
            out["glossy_acc"] = acc = K.IR.filter(sums, P["orays"], active, k["glossy_filter"], COS, F.plane, W, 0, H)
        img = K.GL.apply(img, acc, S, ids, s["reflect"], 0, N)
    # -- the shadows, or the area light in their place
    if hard and not k["lights"]:
        K.O.add_shadows(img, P["hard"], 0, N)
    if k["area"]:
        S = k["area"]
        n = chain.n.get("area", 0) if tp else None
        table = area_table(F, setup, S, 16 if tp else k["area_sets"], k["area_radius"])
        if tp:
            table = K.ugrt.scenes.temporal_sets(table, k["area_sets"], n)
        out["area_mask"] = mask = sets_mask(F, setup, "area", table, thru=k["refract"])
        if tp or k["area_filter"]:
            out["area_vis"] = vis = K.SR.filter(mask, S, P["orays"], P["oactive"], k["area_filter"], COS, F.plane, W, H)
            if tp:
                key = (S, k["area_sets"], k["area_radius"], k["area_filter"], _setup_key(setup)[1], tp)
                hist, vis = chain.blend(F, "area", P, key, vis, S, tp)
                out["area_tvis"] = vis
                out.setdefault("history", {})["area"] = hist
            img = K.SR.shade(img, vis, S, 0, N)
        else:
            img = K.AR.shade(img, mask, S, 0, N)
    # -- gi_apply
    if k["gi"]:
        S, radius = k["gi"], INF if k["gi_radius"] is None else k["gi_radius"]
        sc = K.ugrt.scenes
        if tp:
            table = sc.temporal_sets(sc.ao_direction_sets(S, 16), k["gi_sets"], chain.n.get("gi", 0))
        else:
            table = sc.ao_direction_sets(S, k["gi_sets"])
        out["gi_sum"] = acc = gi_sums(F, setup, S, k["gi_sets"], table, radius, k["gi_shadows"])
        if tp or k["gi_filter"]:
            out["gi_acc"] = acc = K.IR.filter(acc, P["orays"], P["oactive"], k["gi_filter"], COS, F.plane, W, 0, H)
        if tp:
            key = (S, k["gi_sets"], radius, k["gi_gain"], k["gi_shadows"], k["gi_filter"], _setup_key(setup)[1:3], tp)
            hist, acc = chain.blend(F, "gi", P, key, acc, S, tp)
            out["gi_tacc"] = acc
            out.setdefault("history", {})["gi"] = hist
        img = K.IR.apply(img, acc, S, k["gi_gain"], ids, s["mat_list"], 0, N)
    # -- aa_resolve
    if k["aa"]:
        out["aa_edge"], out["aa_sum"] = aa_words(F, setup, k["aa"], k["aa_sets"], bool(k["shadows"] and k["aa_shadows"]))
        img = K.AA.resolve(img, out["aa_sum"], k["aa"], 0, N)
    # -- shade_ao, last
    if k["ao"]:
        S = k["ao"]
        sc = K.ugrt.scenes
        if tp:
            table = sc.temporal_sets(sc.ao_direction_sets(S, 16), k["ao_sets"], chain.n.get("ao", 0))
        else:
            table = ao_table(F, S, k["ao_sets"])
        out["ao_mask"] = mask = sets_mask(F, setup, "ao", table, k["ao_radius"])
        if tp or k["ao_filter"]:
            out["ao_vis"] = vis = K.SR.filter(mask, S, P["orays"], P["oactive"], k["ao_filter"], COS, F.plane, W, H)
            if tp:
                key = (S, k["ao_sets"], k["ao_radius"], k["ao_filter"], tp)
                hist, vis = chain.blend(F, "ao", P, key, vis, S, tp)
                out["ao_tvis"] = vis
                out.setdefault("history", {})["ao"] = hist
            img = K.ASR.shade(img, vis, S, 0, N)
        else:
            img = K.AO.shade(img, mask, S, 0, N)
    if tp:
        chain.prev = (P["orays"], P["oactive"], P["cc"])
    out["image"] = img
    return out


def device_frame(r, setup, **kw):
    """What a Renderer holds behind display(setup, **kw), as cpu_display names it, on the host."""
    lights = getattr(setup, "lights", None)
    k = dict(DEFAULTS, **MORE)
    k.update(kw, lights=lights is not None, num_lights=0 if lights is None else len(lights))
    words = lambda t: t.cpu().numpy().view(np.uint32)
    out = dict(image=r.image.cpu().numpy(), intersect_id=r.intersect_id.cpu().numpy(), is_shadowed=r.is_shadowed.cpu().numpy())
    if k["reflect"]:
        out["levels"] = []
        for j in range(k["bounces"]):
            lv = dict(rays=r.rays_levels[j].cpu().numpy(), active=r.active_levels[j].cpu().numpy(),
                      hit_t=r.hit_t_levels[j].cpu().numpy(), hit_id=r.hit_id_levels[j].cpu().numpy())
            if k["reflect_shadows"] and k["reflect_lights"]:
                lv["occluded"] = r.occluded_lights[j].cpu().numpy()
            elif k["reflect_shadows"]:
                lv["occluded"] = r.occluded_levels[j].cpu().numpy()
            out["levels"].append(lv)
    if k["glossy"]:
        out["levels"] = [dict(rays=r.rays.cpu().numpy(), active=r.active.cpu().numpy())]
    if k["num_lights"] and k["shadows"]:
        out["shadowed_lights"] = r.shadowed_lights[:k["num_lights"]].cpu().numpy()
    for name in ("ao_rays", "ao_active"):
        if k["ao"] or k["area"] or k["gi"] or k["glossy"]:
            out[name] = getattr(r, name).cpu().numpy()
    for effect, names in (("ao", ("ao_mask", "ao_vis", "ao_tvis")), ("area", ("area_mask", "area_vis", "area_tvis")),
                          ("gi", ("gi_sum", "gi_acc", "gi_tacc")), ("glossy", ("glossy_sum", "glossy_acc")),
                          ("aa", ("aa_edge", "aa_sum"))):
        if not k[effect]:
            continue
        for name in names:
            if getattr(r, name, None) is not None:
                out[name] = getattr(r, name).cpu().numpy() if name == "aa_edge" else words(getattr(r, name))
        if k["temporal"] and effect in ("ao", "area", "gi"):
            out.setdefault("history", {})[effect] = r.temporal_history(effect).cpu().numpy()
    return out


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(bits(_f32(a)), bits(_f32(b)))
    return a.shape == b.shape and np.array_equal(a.astype(np.int64), b.astype(np.int64))


def differences(want, got, only=None):
    """The entries of `want` (cpu_display's dict, or device_frame's) that `got` does not hold bit for bit, as
    "name: how many elements differ"; only: the entries to look at."""
    bad = []
    for name, w in want.items():
        if only is not None and name not in only:
            continue
        if name not in got:
            bad.append("%s: missing" % name)
        elif name == "levels":
            for j, (lw, lg) in enumerate(zip(w, got[name])):
                bad += ["level %d %s" % (j + 1, n) for n in lw if not _same(lw[n], lg[n])]
            if len(w) != len(got[name]):
                bad.append("levels: %d, not %d" % (len(got[name]), len(w)))
        elif name == "history":
            bad += ["history %s" % n for n in w if n not in got[name] or not _same(w[n], got[name][n])]
        elif not _same(w, got[name]):
            a, b = np.asarray(w).reshape(-1), np.asarray(got[name]).reshape(-1)
            bad.append("%s: %s" % (name, "shape" if a.shape != b.shape else "%d of %d differ" % (int((a != b).sum()), a.size)))
    return bad
