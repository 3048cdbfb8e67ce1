"""display() of the reference (main.cu:59-302) over the C-ABI.

One :class:`Renderer` owns what the reference's ``DecisionData`` (decision_data.h:13-40),
``Model`` device lists (scene.h:24-28) and the image buffer own, as torch tensors, and
sequences one frame exactly in the reference's order:

  updateLightPosition -> camera -> fillCoordinatesData -> build_frustum_grid ->
  FrustumTracer::trace -> per light { light camera -> fillCoordinatesData ->
  getEffectiveRayGridMapping -> build_secondary_frustum_grid -> processData ->
  check_for_shadows } -> simpleShade | spotlight_shade -> add_shadows

(getRayGridMapping + the host max loop, main.cu:172-187, only produce values that
are overwritten with M_PI, so they are dropped: xM = yM = (float)M_PI.)
With ``reflect=True`` the shading step becomes: secondary rays -> uniform grid
build -> 3D-DDA -> shade_reflect (not in the reference).  With
``bounces=D > 1`` the reflected rays are followed D levels deep: (next rays ->
3D-DDA) x (D-1) behind the first bounce, then shade_reflect_depth (DESIGN.md
section 6).  With ``reflect_shadows=True`` the hits of every reflection level are tested against the
light behind the level's 3D-DDA (occlusion rays -> any-hit walk) and the shading darkens the
occluded levels.  With ``FrameSetup.lights`` the per-light part of the sequence runs once
per light and one shading pass averages the lights (one-stream frame, no reflections); with
``reflect_lights=True`` as well, the reflections are rendered under all of them.  With ``ao=S`` every
one-stream frame ends with ambient occlusion: S hemisphere rays per primary hit through the uniform grid, and a last
pass that scales the image by the share of open rays.  With ``refract=True`` a level's ray goes
through a hit whose material transmits instead of being mirrored, and the reflected hits' shadow walk sees through such
materials.  With ``area=S`` the one-stream single-light frame casts soft shadows: S shadow rays
per primary hit towards a disk around the light through the uniform grid in the place of the light-space shadow stage,
and a last pass that darkens the image by the share of occluded samples; with ``area_sets``
the pixels of a tile aim at different sets of S points, and with ``area_filter`` a gather over the pixels of the same
surface averages their shares before that pass; ``ao_sets`` and ``ao_filter`` do the same for the
hemisphere rays of ``ao``, in a walk that keeps a pixel's rays side by side in a wave.  With
``gi=S`` the one-stream single-light frame adds one bounce of indirect diffuse light: S hemisphere rays per primary hit to
their first hit, which is shaded and shadowed, and a pass that adds the mean to the image.  With
``aa=S`` the one-stream single-light plain frame is anti-aliased where it needs it: the pixels on an edge send S sub-pixel
eye rays through the uniform grid and take the mean of their colours.  With ``temporal=N`` the
frames of a sequence give ``ao``, ``area`` and ``gi`` a different sample set each and blend every frame's share into a
running mean over at most N frames, reprojected through the surface point when the camera moves.
With ``glossy=S`` the one-stream single-light frame without ``reflect`` shows its reflecting materials as rough mirrors: S
rays per primary hit in a lobe around the mirror direction, as wide as the material's spread, to their first hit, and a
pass directly behind the shading call that blends the lobe's mean into the image.
With ``smooth=True`` the shading call reads interpolated vertex normals in the place of the triangles' own: the corners'
adjacency once per geometry, the crease-aware corner normals when the vertices move, and one pass per frame that mixes them
at every primary hit.
With ``fresnel=True`` the ``refract`` frame's glass both transmits and reflects: every glass hit sends the two rays, weighted
by Schlick's share at the hit's angle, and one launch walks the whole ray tree of a pixel in the place of the level chain
(DESIGN.md section 6.16).
With ``dof=S`` the one-stream single-light plain frame is seen through a thin lens of radius ``dof_aperture`` focused at
``dof_focus``: the pixels that a circle of confusion reaches send S rays from points of the lens through the uniform grid
and take the mean of their colours.

Each stage is one function below, shared by the four frame paths (one stream, two streams with a helper thread, two
streams from one host thread, one frame in bands); the paths differ only in the context and stream a stage runs on
and in the events that join the streams.
"""
import contextlib

import numpy as np

from . import (FLAG_STATIC_GEOMETRY, GRID_SPHERICAL, GRID_UNIFORM, MAX_AA_SAMPLES, MAX_AO_DIRS, MAX_AREA_SAMPLES,
               MAX_DOF_WINDOW, MAX_FILTER_RADIUS, MAX_FRESNEL_DEPTH, MAX_GLOSSY_SAMPLES, MAX_LIGHTS, MAX_REFLECT_DEPTH, MAX_TEMPORAL_FRAMES,
               MAX_TEXTURE_ANISO, MAX_TEXTURE_DIM, MAX_TEXTURES)
from .host import Camera

PI_F = float(np.float32(np.pi))


def check_bounces(bounces):
    """1..MAX_REFLECT_DEPTH levels of reflection, or ValueError (before anything is enqueued)."""
    if isinstance(bounces, bool) or not isinstance(bounces, (int, np.integer)) or not 1 <= bounces <= MAX_REFLECT_DEPTH:
        raise ValueError("bounces must be an integer in 1..%d, not %r" % (MAX_REFLECT_DEPTH, bounces))
    return int(bounces)


def check_reflect_shadows(reflect_shadows, reflect):
    """A bool, and only with reflect, or ValueError (before anything is enqueued)."""
    if not isinstance(reflect_shadows, (bool, np.bool_)):
        raise ValueError("reflect_shadows must be a bool, not %r" % (reflect_shadows,))
    if reflect_shadows and not reflect:
        raise ValueError("reflect_shadows=True needs reflect=True: it shadows the reflected hits")
    return bool(reflect_shadows)


def check_refract(refract, reflect):
    """A bool, and only with reflect, or ValueError (before anything is enqueued)."""
    if not isinstance(refract, (bool, np.bool_)):
        raise ValueError("refract must be a bool, not %r" % (refract,))
    if refract and not reflect:
        raise ValueError("refract=True needs reflect=True: the transmitted rays are levels of the bounce chain")
    return bool(refract)


def check_fresnel(fresnel, fresnel_cut=0.0, reflect=False, refract=False, bounces=1, lights=None, reflect_lights=False,
                  two_streams=False):
    """The keywords of the Fresnel glass.  fresnel: False (off) or a number in (0, 1], the scale
    of Schlick's share (True: 1.0); fresnel_cut: a number >= 0, the weight at or below which a child ray is dropped
    (needs fresnel).  fresnel needs reflect=True and refract=True, bounces <= MAX_FRESNEL_DEPTH and the one-stream
    Renderer's single-light frame (no setup.lights, no reflect_lights).  ValueError before anything is enqueued; returns
    None (off) or (scale, cut)."""
    num = (int, float, np.integer, np.floating)
    if isinstance(fresnel_cut, (bool, np.bool_)) or not isinstance(fresnel_cut, num) or not float(np.float32(fresnel_cut)) >= 0.0:
        raise ValueError("fresnel_cut must be a number >= 0, not %r" % (fresnel_cut,))
    if fresnel is False or (isinstance(fresnel, np.bool_) and not fresnel):
        if float(fresnel_cut) != 0.0:
            raise ValueError("fresnel_cut needs fresnel: it drops the light children of a glass hit")
        return None
    if fresnel is True or isinstance(fresnel, np.bool_):
        fresnel = 1.0
    if not isinstance(fresnel, num) or not 0.0 < float(np.float32(fresnel)) <= 1.0:
        raise ValueError("fresnel must be False, True or a number in (0, 1], not %r" % (fresnel,))
    if not (reflect and refract):
        raise ValueError("fresnel needs reflect=True and refract=True: it splits the glass hits of the refract frame")
    if bounces > MAX_FRESNEL_DEPTH:
        raise ValueError("fresnel needs bounces <= %d: the 2^bounces leaves of a pixel's ray tree are the lanes of one wave"
                         % MAX_FRESNEL_DEPTH)
    if lights is not None or reflect_lights:
        raise ValueError("fresnel needs a single-light frame: the ray tree under setup.lights is not built")
    if two_streams:
        raise ValueError("fresnel needs the one-stream Renderer: the two-stream and banded frames keep the level chain")
    return float(np.float32(fresnel)), float(np.float32(fresnel_cut))


_CAMERA_KEYS = ("eye", "look", "up", "near", "far")


def _three_floats(v):
    v = tuple(float(x) for x in v)
    if len(v) != 3:
        raise ValueError("three floats expected, not %d" % len(v))
    return v


def check_reflect_lights(reflect_lights, reflect, lights):
    """A bool, and only with reflect and FrameSetup.lights, or ValueError (before anything is enqueued)."""
    if not isinstance(reflect_lights, (bool, np.bool_)):
        raise ValueError("reflect_lights must be a bool, not %r" % (reflect_lights,))
    if reflect_lights and not reflect:
        raise ValueError("reflect_lights=True needs reflect=True: it renders the reflections under every light")
    if reflect_lights and lights is None:
        raise ValueError("reflect_lights=True needs FrameSetup.lights")
    return bool(reflect_lights)


def check_lights(lights, reflect, two_streams, reflect_lights=False):
    """FrameSetup.lights as a list of (light_camera_params, (x, y, z)) with 1..MAX_LIGHTS entries, or ValueError (before
    anything is enqueued).  Not with reflect unless reflect_lights says so (the reflection shading of sections 6.1 and 6.2
    knows one light; DESIGN.md section 6.4 is the frame that knows all) and not in the two-stream or banded frames
    (two_streams: they keep one light grid on a side context); DESIGN.md section 6.3."""
    if reflect and not reflect_lights:
        raise ValueError("lights cannot be combined with reflect=True: the reflection shading knows one light")
    if two_streams:
        raise ValueError("lights need the one-stream Renderer: the two-stream and banded frames keep one light grid")
    try:
        entries = list(lights)
    except TypeError:
        raise ValueError("lights must be a sequence of (light_camera, shading_light) pairs, not %r" % (lights,))
    if not 1 <= len(entries) <= MAX_LIGHTS:
        raise ValueError("lights must hold 1..%d entries, not %d" % (MAX_LIGHTS, len(entries)))
    out = []
    for k, entry in enumerate(entries):
        try:
            params, pos = entry
            if not isinstance(params, dict):
                raise TypeError("the light camera must be a dict")
            for key in ("eye", "look", "up"):
                _three_floats(params[key])
            float(params["near"]), float(params["far"])
            out.append((params, _three_floats(pos)))
        except (TypeError, ValueError, KeyError) as e:
            raise ValueError("lights[%d] is not (dict with %s, three floats): %r" % (k, "/".join(_CAMERA_KEYS), e))
    return out


def check_ao(ao, ao_radius, two_streams=False):
    """ao: an integer 0..MAX_AO_DIRS (0: off, and ao_radius is not looked at); ao > 0 needs a number ao_radius > 0 and the
    one-stream Renderer (two_streams: the two-stream and banded frames keep the uniform grid on a side context), or
    ValueError (before anything is enqueued); DESIGN.md section 6.5.  Returns (ao, radius or None)."""
    if isinstance(ao, (bool, np.bool_)) or not isinstance(ao, (int, np.integer)) or not 0 <= ao <= MAX_AO_DIRS:
        raise ValueError("ao must be an integer in 0..%d, not %r" % (MAX_AO_DIRS, ao))
    if ao == 0:
        return 0, None
    if isinstance(ao_radius, (bool, np.bool_)) or not isinstance(ao_radius, (int, float, np.integer, np.floating)):
        raise ValueError("ao=%d needs ao_radius, a number greater than 0, not %r" % (ao, ao_radius))
    if not float(np.float32(ao_radius)) > 0.0:
        raise ValueError("ao_radius must be greater than 0, not %r" % (ao_radius,))
    if two_streams:
        raise ValueError("ao needs the one-stream Renderer: the two-stream and banded frames keep the uniform grid on a "
                         "side context")
    return int(ao), float(np.float32(ao_radius))


def check_area(area, area_radius, shadows=True, lights=None, two_streams=False):
    """area: an integer 0..MAX_AREA_SAMPLES (0: off, and nothing else is looked at); area > 0 needs a number
    area_radius > 0, shadows=True, a single-light frame (lights: setup.lights) and the one-stream Renderer (two_streams:
    the two-stream and banded frames keep the uniform grid on a side context), or ValueError (before anything is
    enqueued); DESIGN.md section 6.7.  Returns (area, radius or None)."""
    if isinstance(area, (bool, np.bool_)) or not isinstance(area, (int, np.integer)) or not 0 <= area <= MAX_AREA_SAMPLES:
        raise ValueError("area must be an integer in 0..%d, not %r" % (MAX_AREA_SAMPLES, area))
    if area == 0:
        return 0, None
    if isinstance(area_radius, (bool, np.bool_)) or not isinstance(area_radius, (int, float, np.integer, np.floating)):
        raise ValueError("area=%d needs area_radius, a number greater than 0, not %r" % (area, area_radius))
    if not float(np.float32(area_radius)) > 0.0:
        raise ValueError("area_radius must be greater than 0, not %r" % (area_radius,))
    if not shadows:
        raise ValueError("area needs shadows=True: the area light's penumbra takes the place of the hard shadows")
    if lights is not None:
        raise ValueError("area needs a single-light frame: area lights under setup.lights are not built")
    if two_streams:
        raise ValueError("area needs the one-stream Renderer: the two-stream and banded frames keep the uniform grid on "
                         "a side context")
    return int(area), float(np.float32(area_radius))


AREA_SET_TILES = {1: (1, 1), 4: (2, 2), 16: (4, 4)}  # area_sets -> (set_w, set_h)


def default_filter_plane(bbmin, bbmax):
    """area_filter_plane=None: 1 % of the scene's largest extent, as a float32."""
    return float(np.float32(0.01 * float((np.asarray(bbmax, np.float32) - np.asarray(bbmin, np.float32)).max())))


def _check_sets_filter(name, needs, on, sets, radius, cos, plane):
    """check_area_filter and check_ao_filter: the keywords <name>_sets, <name>_filter, <name>_filter_cos and
    <name>_filter_plane of a frame whose `name` keyword is `on`."""
    if isinstance(sets, (bool, np.bool_)) or not isinstance(sets, (int, np.integer)) or int(sets) not in AREA_SET_TILES:
        raise ValueError("%s_sets must be 1, 4 or 16, not %r" % (name, sets))
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) \
            or not 0 <= radius <= MAX_FILTER_RADIUS:
        raise ValueError("%s_filter must be an integer in 0..%d, not %r" % (name, MAX_FILTER_RADIUS, radius))
    if not on and (sets != 1 or radius != 0):
        raise ValueError("%s_sets and %s_filter need %s > 0: they shape %s" % (name, name, name, needs))
    if not radius:
        return int(sets), 0, None, None
    number = (int, float, np.integer, np.floating)
    if isinstance(cos, (bool, np.bool_)) or not isinstance(cos, number) or np.isnan(np.float32(cos)):
        raise ValueError("%s_filter_cos must be a number, not %r" % (name, cos))
    if plane is not None:
        if isinstance(plane, (bool, np.bool_)) or not isinstance(plane, number) or not float(np.float32(plane)) >= 0.0:
            raise ValueError("%s_filter_plane must be None or a number not below 0, not %r" % (name, plane))
        plane = float(np.float32(plane))
    return int(sets), int(radius), float(np.float32(cos)), plane


def check_area_filter(area, area_sets=1, area_filter=0, area_filter_cos=0.9, area_filter_plane=None):
    """The interleaved sample sets and the gather of an area light, checked in check_area's
    manner behind it (area: what check_area returned).  area_sets: 1, 4 or 16 (tiles of 1 x 1, 2 x 2, 4 x 4 pixels);
    area_filter: an integer radius 0..MAX_FILTER_RADIUS (0: no gather); a value of either that is not its default needs
    area > 0.  area_filter_cos: a number (no NaN); area_filter_plane: None (default_filter_plane) or a number >= 0; the
    two are looked at with area_filter > 0 only.  ValueError before anything is enqueued.  Returns
    (area_sets, area_filter, cos or None, plane or None)."""
    return _check_sets_filter("area", "the area light's samples and penumbra", area, area_sets, area_filter, area_filter_cos,
                              area_filter_plane)


def check_ao_filter(ao, ao_sets=1, ao_filter=0, ao_filter_cos=0.9, ao_filter_plane=None):
    """The interleaved direction sets and the gather of ambient occlusion: check_area_filter's
    rules for ao_sets, ao_filter, ao_filter_cos and ao_filter_plane, behind check_ao (ao: what check_ao returned).
    Returns (ao_sets, ao_filter, cos or None, plane or None)."""
    return _check_sets_filter("ao", "the hemisphere's rays and their shading", ao, ao_sets, ao_filter, ao_filter_cos,
                              ao_filter_plane)


def check_gi(gi, gi_radius=None, gi_gain=1.0, gi_shadows=True, gi_sets=1, gi_filter=0, gi_filter_cos=0.9,
             gi_filter_plane=None, lights=None, reflect_lights=False, two_streams=False):
    """The keywords of the indirect diffuse light.  gi: check_ao's rule, an integer
    0..MAX_AO_DIRS (0: off, and every other gi_* keyword must be at its default); gi_radius: None (+inf: the whole grid) or
    a number greater than 0; gi_gain: a number not below 0; gi_shadows: a bool; gi_sets, gi_filter, gi_filter_cos and
    gi_filter_plane: check_ao_filter's rules.  gi > 0 needs a single-light frame (lights: setup.lights; reflect_lights)
    and the one-stream Renderer, where check_area asks for them.  ValueError before anything is enqueued.  Returns None
    (off) or (gi, radius, gain, shadows, gi_sets, gi_filter, cos or None, plane or None)."""
    if isinstance(gi, (bool, np.bool_)) or not isinstance(gi, (int, np.integer)) or not 0 <= gi <= MAX_AO_DIRS:
        raise ValueError("gi must be an integer in 0..%d, not %r" % (MAX_AO_DIRS, gi))
    number = (int, float, np.integer, np.floating)
    if gi_radius is not None:
        if isinstance(gi_radius, (bool, np.bool_)) or not isinstance(gi_radius, number) \
                or not float(np.float32(gi_radius)) > 0.0:
            raise ValueError("gi_radius must be None or a number greater than 0, not %r" % (gi_radius,))
    if isinstance(gi_gain, (bool, np.bool_)) or not isinstance(gi_gain, number) or not float(np.float32(gi_gain)) >= 0.0:
        raise ValueError("gi_gain must be a number not below 0, not %r" % (gi_gain,))
    if not isinstance(gi_shadows, (bool, np.bool_)):
        raise ValueError("gi_shadows must be True or False, not %r" % (gi_shadows,))
    sets = _check_sets_filter("gi", "the indirect light's rays and its gather", gi, gi_sets, gi_filter, gi_filter_cos,
                              gi_filter_plane)
    if gi == 0:
        if gi_radius is not None or float(gi_gain) != 1.0 or not gi_shadows:
            raise ValueError("gi_radius, gi_gain and gi_shadows need gi > 0: they shape the indirect light")
        return None
    if lights is not None or reflect_lights:
        raise ValueError("gi needs a single-light frame: the indirect light under setup.lights is not built")
    if two_streams:
        raise ValueError("gi needs the one-stream Renderer: the two-stream and banded frames keep the uniform grid on a "
                         "side context")
    radius = float("inf") if gi_radius is None else float(np.float32(gi_radius))
    return (int(gi), radius, float(np.float32(gi_gain)), bool(gi_shadows)) + sets


def check_aa(aa, aa_sets=1, aa_cos=0.9, aa_plane=None, aa_shadows=True, reflect=False, frame_cnt=1, lights=None, area=0,
             gi=0, reflect_lights=False, two_streams=False):
    """The keywords of the adaptive anti-aliasing.  aa: an integer 0..MAX_AA_SAMPLES (0: off, and
    every other aa_* keyword must be at its default); aa_sets: 1, 4 or 16; aa_cos: a number (no NaN); aa_plane: None
    (default_filter_plane) or a number (no NaN); aa_shadows: a bool.  aa > 0 needs the one-stream Renderer's single-light
    plain frame: reflect=False, frame_cnt < 2, no setup.lights, no area, no gi (ao composes).  ValueError before anything
    is enqueued.  Returns None (off) or (aa, aa_sets, cos, plane or None, shadows)."""
    if isinstance(aa, (bool, np.bool_)) or not isinstance(aa, (int, np.integer)) or not 0 <= aa <= MAX_AA_SAMPLES:
        raise ValueError("aa must be an integer in 0..%d, not %r" % (MAX_AA_SAMPLES, aa))
    if isinstance(aa_sets, (bool, np.bool_)) or not isinstance(aa_sets, (int, np.integer)) or int(aa_sets) not in AREA_SET_TILES:
        raise ValueError("aa_sets must be 1, 4 or 16, not %r" % (aa_sets,))
    number = (int, float, np.integer, np.floating)
    if isinstance(aa_cos, (bool, np.bool_)) or not isinstance(aa_cos, number) or np.isnan(np.float32(aa_cos)):
        raise ValueError("aa_cos must be a number, not %r" % (aa_cos,))
    if aa_plane is not None:
        if isinstance(aa_plane, (bool, np.bool_)) or not isinstance(aa_plane, number) or np.isnan(np.float32(aa_plane)):
            raise ValueError("aa_plane must be None or a number, not %r" % (aa_plane,))
        aa_plane = float(np.float32(aa_plane))
    if not isinstance(aa_shadows, (bool, np.bool_)):
        raise ValueError("aa_shadows must be True or False, not %r" % (aa_shadows,))
    if aa == 0:
        if aa_sets != 1 or float(np.float32(aa_cos)) != float(np.float32(0.9)) or aa_plane is not None or not aa_shadows:
            raise ValueError("aa_sets, aa_cos, aa_plane and aa_shadows need aa > 0: they shape the anti-aliasing")
        return None
    if reflect or reflect_lights:
        raise ValueError("aa needs reflect=False: edges seen in mirrors are not supersampled")
    if isinstance(frame_cnt, (bool, np.bool_)) or not isinstance(frame_cnt, (int, np.integer)) or frame_cnt >= 2:
        raise ValueError("aa needs frame_cnt < 2: the samples are shaded as the plain frame shades, not under the spot light")
    if lights is not None:
        raise ValueError("aa needs a single-light frame: the samples under setup.lights are not built")
    if area:
        raise ValueError("aa needs area=0: the samples are not shaded under an area light")
    if gi:
        raise ValueError("aa needs gi=0: the samples gather no indirect light")
    if two_streams:
        raise ValueError("aa needs the one-stream Renderer: the two-stream and banded frames keep the uniform grid on a "
                         "side context")
    return int(aa), int(aa_sets), float(np.float32(aa_cos)), aa_plane, bool(aa_shadows)


def check_dof(dof, dof_aperture=0.0, dof_focus=None, dof_sets=1, dof_min=0.5, dof_window=4, dof_shadows=True, aa=0,
              reflect=False, refract=False, fresnel=False, glossy=0, gi=0, area=0, smooth=False, temporal=0, frame_cnt=1,
              lights=None, reflect_lights=False, two_streams=False):
    """The keywords of the depth of field.  dof: an integer 0..MAX_AA_SAMPLES (0: off, and every
    other dof_* keyword must be at its default); dof_aperture: the lens radius, a finite number >= 0; dof_focus: None (the
    distance to the camera's look-at point) or a finite number > 0; dof_sets: 1, 4 or 16; dof_min: a finite number > 0,
    the smallest circle of confusion in pixels that is traced; dof_window: an integer 0..MAX_DOF_WINDOW, how far a
    neighbour's circle is followed; dof_shadows: a bool.  dof > 0 needs the one-stream Renderer's single-light plain frame
    with frame_cnt < 2 and no aa, reflect, refract, fresnel, glossy, gi, area, smooth or temporal.  ValueError before
    anything is enqueued.  Returns None (off) or (dof, dof_sets, aperture, focus or None, min, window, shadows)."""
    number = (int, float, np.integer, np.floating)

    def real(v):
        return not isinstance(v, (bool, np.bool_)) and isinstance(v, number) and bool(np.isfinite(np.float32(v)))

    if isinstance(dof, (bool, np.bool_)) or not isinstance(dof, (int, np.integer)) or not 0 <= dof <= MAX_AA_SAMPLES:
        raise ValueError("dof must be an integer in 0..%d, not %r" % (MAX_AA_SAMPLES, dof))
    if not real(dof_aperture) or float(np.float32(dof_aperture)) < 0:
        raise ValueError("dof_aperture must be a finite number >= 0, not %r" % (dof_aperture,))
    if dof_focus is not None and (not real(dof_focus) or not float(np.float32(dof_focus)) > 0):
        raise ValueError("dof_focus must be None or a finite number > 0, not %r" % (dof_focus,))
    if isinstance(dof_sets, (bool, np.bool_)) or not isinstance(dof_sets, (int, np.integer)) or int(dof_sets) not in AREA_SET_TILES:
        raise ValueError("dof_sets must be 1, 4 or 16, not %r" % (dof_sets,))
    if not real(dof_min) or not float(np.float32(dof_min)) > 0:
        raise ValueError("dof_min must be a finite number > 0, not %r" % (dof_min,))
    if isinstance(dof_window, (bool, np.bool_)) or not isinstance(dof_window, (int, np.integer)) or \
            not 0 <= dof_window <= MAX_DOF_WINDOW:
        raise ValueError("dof_window must be an integer in 0..%d, not %r" % (MAX_DOF_WINDOW, dof_window))
    if not isinstance(dof_shadows, (bool, np.bool_)):
        raise ValueError("dof_shadows must be True or False, not %r" % (dof_shadows,))
    if dof == 0:
        if float(np.float32(dof_aperture)) != 0.0 or dof_focus is not None or dof_sets != 1 or \
                float(np.float32(dof_min)) != 0.5 or dof_window != 4 or not dof_shadows:
            raise ValueError("dof_aperture, dof_focus, dof_sets, dof_min, dof_window and dof_shadows need dof > 0: they shape "
                             "the depth of field")
        return None
    if aa:
        raise ValueError("dof needs aa=0: the lens samples already carry sub-pixel offsets")
    if reflect or refract or fresnel or reflect_lights:
        raise ValueError("dof needs reflect=False, refract=False and fresnel=False: the lens samples send no secondary rays")
    if glossy:
        raise ValueError("dof needs glossy=0: the lens samples send no lobe")
    if gi:
        raise ValueError("dof needs gi=0: the lens samples gather no indirect light")
    if area:
        raise ValueError("dof needs area=0: the lens samples are not shaded under an area light")
    if smooth:
        raise ValueError("dof needs smooth=False: the lens samples shade with the flat normal")
    if temporal:
        raise ValueError("dof needs temporal=0: the lens samples are not accumulated over frames")
    if isinstance(frame_cnt, (bool, np.bool_)) or not isinstance(frame_cnt, (int, np.integer)) or frame_cnt >= 2:
        raise ValueError("dof needs frame_cnt < 2: the samples are shaded as the plain frame shades, not under the spot light")
    if lights is not None:
        raise ValueError("dof needs a single-light frame: the samples under setup.lights are not built")
    if two_streams:
        raise ValueError("dof needs the one-stream Renderer: the two-stream and banded frames keep the uniform grid on a "
                         "side context")
    return (int(dof), int(dof_sets), float(np.float32(dof_aperture)), None if dof_focus is None else float(np.float32(dof_focus)),
            float(np.float32(dof_min)), int(dof_window), bool(dof_shadows))


def check_temporal(temporal, temporal_cos=0.9, temporal_plane=None, effects=False, lights=None, reflect_lights=False,
                   two_streams=False):
    """The keywords of the temporal accumulation.  temporal: 0 (off, and the other two must be at
    their defaults) or an integer 2..MAX_TEMPORAL_FRAMES, the most frames a running mean spans; temporal_cos: a number (no
    NaN); temporal_plane: None (default_filter_plane) or a number not below 0.  temporal > 0 needs one of ao, area and gi
    (effects), a single-light frame (lights: setup.lights; reflect_lights) and the one-stream Renderer.  ValueError before
    anything is enqueued.  Returns None (off) or (temporal, cos, plane or None)."""
    if isinstance(temporal, (bool, np.bool_)) or not isinstance(temporal, (int, np.integer)) \
            or not (temporal == 0 or 2 <= temporal <= MAX_TEMPORAL_FRAMES):
        raise ValueError("temporal must be 0 or an integer in 2..%d, not %r" % (MAX_TEMPORAL_FRAMES, temporal))
    number = (int, float, np.integer, np.floating)
    if isinstance(temporal_cos, (bool, np.bool_)) or not isinstance(temporal_cos, number) or np.isnan(np.float32(temporal_cos)):
        raise ValueError("temporal_cos must be a number, not %r" % (temporal_cos,))
    if temporal_plane is not None:
        if isinstance(temporal_plane, (bool, np.bool_)) or not isinstance(temporal_plane, number) \
                or not float(np.float32(temporal_plane)) >= 0.0:
            raise ValueError("temporal_plane must be None or a number not below 0, not %r" % (temporal_plane,))
        temporal_plane = float(np.float32(temporal_plane))
    if temporal == 0:
        if float(np.float32(temporal_cos)) != float(np.float32(0.9)) or temporal_plane is not None:
            raise ValueError("temporal_cos and temporal_plane need temporal > 0: they shape the accumulation")
        return None
    if not effects:
        raise ValueError("temporal needs ao, area or gi: it averages their samples over the frames")
    if lights is not None or reflect_lights:
        raise ValueError("temporal needs a single-light frame: the accumulation under setup.lights is not built")
    if two_streams:
        raise ValueError("temporal needs the one-stream Renderer: the two-stream and banded frames keep the uniform grid "
                         "on a side context")
    return int(temporal), float(np.float32(temporal_cos)), temporal_plane


def check_glossy(glossy, glossy_sets=1, glossy_filter=0, glossy_filter_cos=0.9, glossy_filter_plane=None, glossy_radius=None,
                 glossy_shadows=True, reflect=False, refract=False, aa=0, temporal=0, lights=None, reflect_lights=False,
                 two_streams=False):
    """The keywords of the glossy reflections.  glossy: an integer 0..MAX_GLOSSY_SAMPLES (0: off,
    and every other glossy_* keyword must be at its default); glossy_sets, glossy_filter, glossy_filter_cos and
    glossy_filter_plane: check_ao_filter's rules; glossy_radius: None (+inf: the whole grid) or a number greater than 0;
    glossy_shadows: a bool.  glossy > 0 needs the one-stream Renderer's single-light frame with reflect=False (ao, area
    and gi compose): no reflect, refract, aa, temporal (the reprojection follows the primary hit, and a reflection moves
    with the eye), setup.lights or reflect_lights.  ValueError before anything is enqueued.  Returns None (off) or
    (glossy, radius, shadows, glossy_sets, glossy_filter, cos or None, plane or None)."""
    if isinstance(glossy, (bool, np.bool_)) or not isinstance(glossy, (int, np.integer)) \
            or not 0 <= glossy <= MAX_GLOSSY_SAMPLES:
        raise ValueError("glossy must be an integer in 0..%d, not %r" % (MAX_GLOSSY_SAMPLES, glossy))
    if glossy_radius is not None:
        if isinstance(glossy_radius, (bool, np.bool_)) or not isinstance(glossy_radius, (int, float, np.integer, np.floating)) \
                or not float(np.float32(glossy_radius)) > 0.0:
            raise ValueError("glossy_radius must be None or a number greater than 0, not %r" % (glossy_radius,))
    if not isinstance(glossy_shadows, (bool, np.bool_)):
        raise ValueError("glossy_shadows must be True or False, not %r" % (glossy_shadows,))
    sets = _check_sets_filter("glossy", "the lobe's rays and its gather", glossy, glossy_sets, glossy_filter, glossy_filter_cos,
                              glossy_filter_plane)
    if glossy == 0:
        if glossy_radius is not None or not glossy_shadows:
            raise ValueError("glossy_radius and glossy_shadows need glossy > 0: they shape the lobe's rays")
        return None
    if reflect or refract or reflect_lights:
        raise ValueError("glossy needs reflect=False: lobes on the levels of the bounce chain are not built")
    if aa:
        raise ValueError("glossy needs aa=0: the sub-pixel samples send no lobe")
    if temporal:
        raise ValueError("glossy needs temporal=0: the reprojection follows the primary hit, and a reflection moves with the eye")
    if lights is not None:
        raise ValueError("glossy needs a single-light frame: the lobe's hits under setup.lights are not built")
    if two_streams:
        raise ValueError("glossy needs the one-stream Renderer: the two-stream and banded frames keep the uniform grid on a "
                         "side context")
    radius = float("inf") if glossy_radius is None else float(np.float32(glossy_radius))
    return (int(glossy), radius, bool(glossy_shadows)) + sets


def check_smooth(smooth, smooth_cos=0.5, smooth_signed=False, reflect=False, refract=False, glossy=0, aa=0,
                 reflect_lights=False, two_streams=False):
    """The keywords of smooth shading.  smooth: a bool (False: off, and the other two must be at
    their defaults); smooth_cos: a number (no NaN), the cosine of the crease angle -- a face's normal counts at a corner
    where it lies within it of the corner's own face's (<= -1: every face, > 1: none but its own); smooth_signed: a bool,
    True leaves the normals' signs as they are where the primary tracer folds its normals into the positive octant.
    smooth needs the one-stream Renderer and no reflect, refract, glossy, aa or reflect_lights.  ValueError before
    anything is enqueued.  Returns None (off) or (cos, signed)."""
    if not isinstance(smooth, (bool, np.bool_)):
        raise ValueError("smooth must be True or False, not %r" % (smooth,))
    number = (int, float, np.integer, np.floating)
    if isinstance(smooth_cos, (bool, np.bool_)) or not isinstance(smooth_cos, number) or np.isnan(np.float32(smooth_cos)):
        raise ValueError("smooth_cos must be a number, not %r" % (smooth_cos,))
    if not isinstance(smooth_signed, (bool, np.bool_)):
        raise ValueError("smooth_signed must be True or False, not %r" % (smooth_signed,))
    if not smooth:
        if float(np.float32(smooth_cos)) != 0.5 or smooth_signed:
            raise ValueError("smooth_cos and smooth_signed need smooth=True: they shape the vertex normals")
        return None
    if reflect or refract or reflect_lights:
        raise ValueError("smooth needs reflect=False: the reflected and refracted rays leave along the flat normal")
    if glossy:
        raise ValueError("smooth needs glossy=0: the lobe stands around the flat normal's mirror direction")
    if aa:
        raise ValueError("smooth needs aa=0: the sub-pixel samples shade with the flat normal")
    if two_streams:
        raise ValueError("smooth needs the one-stream Renderer: the two-stream and banded frames are not built")
    return float(np.float32(smooth_cos)), bool(smooth_signed)


# -- the stages of a frame.  Each enqueues on the context c it is given, with the frame arrays of f (a Renderer or a
# BandedRenderer) and the arrays of b that belong to one context (the Renderer itself, or one band).


def camera_pass(c, f, b, setup, cam):
    """updateLightPosition (per_frame_funcs.h:6), d_cam_position <- worldori (main.cu:128), fillCoordinatesData,
    build_frustum_grid, FrustumTracer::trace."""
    c.set_light_position(setup.shading_light)
    b._upload_cam_pos(cam.worldori)
    c.upload_camera(cam.camcoords)
    c.grid_build_perspective(f.d_faces, f.d_verts, f.F)
    # (no lists: the trace goes through the grid as the build left it, ugrt_trace_primary_grid; asking for the grid's
    # lists would make the build merge its wide triangles into every cell first)
    c.trace_primary(None, None, None, f.normal, f.t, f.dir, f.is_shadowed, f.intersect_id, f.d_verts, f.d_faces)


def use_light_camera(c, lcam):
    """dd_camcoords is the light's from here on, shadows or not: the light grid build and the shading kernels read it
    (main.cu:158-170)."""
    c.upload_camera(lcam.camcoords)


def build_grid(c, f, which, shards=None):
    """build_secondary_frustum_grid (GRID_SPHERICAL) or the uniform grid (GRID_UNIFORM) over f's triangles.
    shards (parallel.GridShards; one-stream frames only): this rank bins its window of the triangle list, the shards
    are exchanged and merged."""
    if shards is None:
        if which == GRID_SPHERICAL:
            c.grid_build_spherical(f.d_faces, f.d_verts, f.F, PI_F, PI_F)
        else:
            c.grid_build_uniform(f.d_faces, f.d_verts, f.F, f.bbmin, f.bbmax)
        return
    from .parallel import face_window

    c.set_face_window(*face_window(shards.rank, shards.world, f.F))
    try:
        build_grid(c, f, which)
        value, key, span, offset, gi = c.grid_arrays(which)
        ks, vs, sps, counts = shards.exchange(key, value, span, gi.total_refs)
        if shards.world == 1:  # the parts must not be the context's own arrays
            ks, vs, sps = [ks[0].clone()], [vs[0].clone()], [sps[0].clone()]
        c.grid_merge_shards(which, ks, vs, sps, counts)
        f._shard_parts = (ks, vs, sps)  # alive until the merge has run
    finally:
        c.set_face_window(0, -1)  # whatever happened: later builds bin every triangle again


# The one-stream frame builds the light grid between the ray mapping and the sort (the reference's order), the
# two-stream frames on the side stream: so these are two stages, and the shadow trace is given the grid's pointers.
def map_rays(c, f, b):
    """getEffectiveRayGridMapping."""
    c.map_rays_to_light(f.t, f.dir, b._d_map, b.cam_pos, PI_F, PI_F)


def sort_rays(c, b):
    """processData, deferred: the chunk count stays on the device until num_chunks is read."""
    b._num_chunks = c.sort_rays(b._d_map, b._prefix, deferred=True)


def trace_shadows(c, f, b, light_grid, is_shadowed=None):
    """check_for_shadows through the light grid; light_grid: its grid_ptrs().  is_shadowed: the flags the pass sets
    (it only ever sets them, and skips the rays whose flag is set), f.is_shadowed unless given."""
    lvalue, lspan, loffset, _ = light_grid
    c.trace_shadow(lvalue, f.d_verts, f.d_faces, lspan, loffset, f.t, f.dir,
                   f.is_shadowed if is_shadowed is None else is_shadowed, b._d_map, b._prefix, b.cam_pos, b._num_chunks)


def check_textures(textures, texture_aniso=8, texture_bias=0, reflect=False, refract=False, fresnel=False, glossy=0, gi=0,
                   aa=0, dof=0, frame_cnt=1, reflect_lights=False, two_streams=False):
    """The keywords of texture mapping.  textures: a bool (False: off, and the other two must be
    at their defaults); texture_aniso: an int in 1..MAX_TEXTURE_ANISO, the most taps along a footprint's longer axis (1:
    isotropic trilinear); texture_bias: an int in -16..16 added to every pixel's level.  Returns None (off) or (texture_aniso,
    texture_bias).  textures needs the one-stream Renderer and no reflect, refract, fresnel, glossy, gi, aa, dof or
    reflect_lights: their kernels and ugrt_gi_apply read a hit's colour from its material's Kd (frame_cnt is taken and
    not looked at: the spotlight frame composes).  ValueError before anything is enqueued."""
    if not isinstance(textures, (bool, np.bool_)):
        raise ValueError("textures must be True or False, not %r" % (textures,))
    for name, v, lo, hi in (("texture_aniso", texture_aniso, 1, MAX_TEXTURE_ANISO), ("texture_bias", texture_bias, -16, 16)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d..%d, not %r" % (name, lo, hi, v))
    if not textures:
        if texture_aniso != 8 or texture_bias != 0:
            raise ValueError("texture_aniso and texture_bias need textures=True: they shape the texture's filter")
        return None
    if reflect or refract or fresnel or reflect_lights:
        raise ValueError("textures needs reflect=False: the levels' hits are shaded from their materials' Kd")
    for name, v in (("glossy", glossy), ("gi", gi), ("aa", aa), ("dof", dof)):
        if v:
            raise ValueError("textures needs %s=0: the gather's hits and ugrt_gi_apply are shaded from the materials' Kd" % name)
    if two_streams:
        raise ValueError("textures needs the one-stream Renderer: the two-stream and banded frames are not built")
    return int(texture_aniso), int(texture_bias)


def texture_pass(c, f, cam_pos, tex):
    """The albedo of a textured frame into f.albedo, directly behind the camera pass: the ids are
    the triangles' and the context's camera is the eye's, whose rays through the neighbouring pixels give the footprint
    (the light's camera block replaces it for the rest of the frame).  Returns the buffer the shading call reads in the
    place of the materials' Kd."""
    st = f._tex
    c.texture_albedo(f.t, f.dir, f.intersect_id, cam_pos, f.d_verts, f.d_faces, st["uvs"], st["num_uvs"], st["uv_faces"],
                     f.d_matidx, f.d_matlist, f.num_materials, st["mat_texture"], st["mat_texture_host"], tex[0], tex[1],
                     f.albedo)
    return f.albedo


def smooth_pass(c, f, cam_pos, signed):
    """The shading normals of a smooth frame into f.snormal, directly before the shading call
    (the ids are the triangles' still): the corner normals mixed at every primary hit, f.normal's words elsewhere.  Returns
    the buffer the shading call reads in the place of f.normal; f.normal itself is left to the frame's other stages."""
    c.smooth_normals(f.t, f.dir, f.intersect_id, cam_pos, f.d_verts, f.d_faces, f.corner_normals, f.normal, not signed,
                     f.snormal)
    return f.snormal


def shade_lights(c, f, cam_pos, lights, shadows, normal=None, albedo=None):
    """The Lambertian shading of every light and its shadows, averaged, in one pass.  normal: the
    normals the pass reads (smooth_pass'), f.normal unless given.  albedo (texture_pass'): the pixels' Kd in the place of
    their materials'."""
    if albedo is not None:
        c.texture_shade_lights(f.image, f.normal if normal is None else normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx,
                              f.d_matlist, f.num_materials, [pos for _, pos in lights], f.shadowed_lights if shadows else None,
                              albedo)
        return
    c.shade_lights(f.image, f.normal if normal is None else normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx,
                   f.d_matlist, f.num_materials,
                   [pos for _, pos in lights], f.shadowed_lights if shadows else None)


def refracts(f):
    """This frame's display(..., refract=) as the stages read it (a frame that never heard of it: False)."""
    return getattr(f, "refract", False)


def see_through(f):
    """What an any-hit walk is given to see through glass: (mat_idx, transmit, num_materials) in a refract frame, else
    None."""
    return (f.d_matidx, f.d_transmit, f.num_materials) if refracts(f) else None


def any_hit(c, name, thru, *args):
    """The context's any-hit call `name`, or with thru (see_through) its _thru twin, which takes thru's three behind."""
    getattr(c, name if thru is None else name + "_thru")(*args, *(thru or ()))


def level_weights(f):
    """What the shading calls are given as d_reflect: how much of a level's colour comes from the next level.  In a
    refract frame that is a glass material's transmit (f.d_continue), otherwise its reflect."""
    return f.d_continue if refracts(f) else f.d_reflect


def shade_reflect_lights(c, f, cam_pos, lights, bounces, shadows, reflect_shadows):
    """The reflection levels blended under every light, its shadows and its occluded levels, averaged, in one pass
    (DESIGN.md section 6.4)."""
    c.shade_reflect_lights(f.image, f.normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx, f.d_matlist,
                           level_weights(f), f.num_materials, f.d_verts, f.d_faces, bounces, f.rays_levels, f.active_levels,
                           f.hit_t_levels, f.hit_id_levels, [pos for _, pos in lights],
                           f.shadowed_lights if shadows else None, f.occluded_lights if reflect_shadows else None)


def reflect_rays(c, f, cam_pos):
    """Level 1's secondary rays from the primary hits (a refract frame: through glass, mirrored elsewhere)."""
    if refracts(f):
        c.refract_rays(cam_pos, f.t, f.dir, f.intersect_id, f.d_matidx, f.d_reflect, f.d_transmit, f.d_ior,
                       f.num_materials, f.d_verts, f.d_faces, f.reflect_eps, f.rays, f.active)
        return
    c.reflect_rays(cam_pos, f.t, f.dir, f.intersect_id, f.d_matidx, f.d_reflect, f.num_materials, f.d_verts,
                   f.d_faces, f.reflect_eps, f.rays, f.active)


def trace_reflections(c, f, bounces, shadow_light=None, shadow_lights=None):
    """3D-DDA of level 1 through c's uniform grid, then levels 2..bounces (next rays -> 3D-DDA) behind it with no
    host wait (a level without an active ray costs the DDA's prepare kernel and an empty persistent launch).
    shadow_light (reflect_shadows: the light camera's eye, three host floats): behind every level's 3D-DDA its hits'
    occlusion rays towards that point and the any-hit walk up to it (t < 1) into f.occluded_levels.
    shadow_lights (reflect_lights with reflect_shadows: the eyes of the L light cameras): the occlusion rays ONCE per
    level (towards the first eye; only their origins are used) and one any-hit launch towards all L eyes into level j's
    [L, N] layers of f.occluded_lights.
    A refract frame (f.refract) generates the levels with the refract calls and walks the occlusion rays with the any-hit
    calls that see through glass."""
    uvalue, uspan, uoffset, _ = c.grid_ptrs(GRID_UNIFORM)
    rays, active, hit_t, hit_id = f.rays, f.active, f.hit_t, f.hit_id
    for j in range(bounces):
        if j:
            nrays, nactive = f.rays_levels[j], f.active_levels[j]
            if refracts(f):
                c.refract_rays_next(rays, active, hit_t, hit_id, f.d_matidx, f.d_reflect, f.d_transmit, f.d_ior,
                                    f.num_materials, f.d_verts, f.d_faces, f.reflect_eps, nrays, nactive)
            else:
                c.reflect_rays_next(rays, active, hit_t, hit_id, f.d_matidx, f.d_reflect, f.num_materials, f.d_verts,
                                    f.d_faces, f.reflect_eps, nrays, nactive)
            rays, active, hit_t, hit_id = nrays, nactive, f.hit_t_levels[j], f.hit_id_levels[j]
        c.trace_dda(uvalue, uspan, uoffset, f.d_verts, f.d_faces, rays, active, hit_t, hit_id)
        if shadow_light is not None:
            c.occlusion_rays(rays, active, hit_t, hit_id, f.d_verts, f.d_faces, shadow_light, f.reflect_eps,
                             f.occlusion_rays, f.occlusion_active)
            any_hit(c, "trace_dda_any", see_through(f), uvalue, uspan, uoffset, f.d_verts, f.d_faces, f.occlusion_rays,
                    f.occlusion_active, 1.0, f.occluded_levels[j])
        if shadow_lights is not None:
            c.occlusion_rays(rays, active, hit_t, hit_id, f.d_verts, f.d_faces, shadow_lights[0], f.reflect_eps,
                             f.occlusion_rays, f.occlusion_active)
            any_hit(c, "trace_dda_any_lights", see_through(f), uvalue, uspan, uoffset, f.d_verts, f.d_faces,
                    f.occlusion_rays, f.occlusion_active, shadow_lights, f.occluded_lights[j])


def fresnel_pass(c, f, cam_pos, bounces, fresnel, shadow_light=None):
    """The ray tree of every pixel with a level-1 ray, in the place of trace_reflections: one
    fresnel_gather through c's uniform grid into f.f_acc.  fresnel: check_fresnel's (scale, cut); shadow_light
    (reflect_shadows): the light camera's eye."""
    uvalue, uspan, uoffset, _ = c.grid_ptrs(GRID_UNIFORM)
    c.fresnel_gather(uvalue, uspan, uoffset, f.d_verts, f.d_faces, f.rays, f.active, f.normal, f.t, f.dir, f.intersect_id,
                     cam_pos, f.d_matidx, f.d_matlist, f.d_reflect, f.d_transmit, f.d_ior, f.num_materials, bounces,
                     fresnel[0], fresnel[1], shadow_light, f.reflect_eps, f.f_acc)


def ao_pass(c, f, cam_pos, dirs, radius, sets=None, have_rays=False):
    """Ambient occlusion's rays and walk: {origin, normal} of every primary hit, then the any-hit
    walk along the hemisphere directions `dirs` up to `radius` through c's uniform grid into f.ao_mask.  sets
    ((table, (set_w, set_h), gather)) with a table: the device table of a direction set per pixel
    of the tile, and the walk is the pixel-major one over direction sets.  have_rays: glossy_pass or area_pass of this frame
    wrote the rays already.  Runs behind the uniform grid's build and before the shading call that rewrites the ids."""
    uvalue, uspan, uoffset, _ = c.grid_ptrs(GRID_UNIFORM)
    if not have_rays:
        c.ao_rays(cam_pos, f.t, f.dir, f.intersect_id, f.d_verts, f.d_faces, f.reflect_eps, f.ao_rays, f.ao_active)
    if sets is not None and sets[0] is not None:
        c.trace_dda_any_hemi_sets(uvalue, uspan, uoffset, f.d_verts, f.d_faces, f.ao_rays, f.ao_active, len(dirs), sets[1][0],
                                  sets[1][1], sets[0], radius, f.ao_mask)
    else:
        c.trace_dda_any_hemi(uvalue, uspan, uoffset, f.d_verts, f.d_faces, f.ao_rays, f.ao_active, dirs, radius, f.ao_mask)


def ao_shade(c, f, dirs, radius, sets=None):
    """Ambient occlusion's last pass over the image (ao_pass' arguments): shade_ao, or with a gather ((radius, cos, plane),
    DESIGN.md section 6.9) filter_visibility over f.ao_mask into f.ao_vis and shade_ao_vis."""
    if sets is not None and sets[2] is not None:
        c.filter_visibility(f.ao_mask, len(dirs), f.ao_rays, f.ao_active, sets[2][0], sets[2][1], sets[2][2], f.ao_vis)
        c.shade_ao_vis(f.image, f.ao_vis, len(dirs))
    else:
        c.shade_ao(f.image, f.ao_mask, len(dirs))


def gi_pass(c, f, cam_pos, gi, shadow_light, have_rays):
    """The indirect light's gather: {origin, normal} of every primary hit (ao_rays, into the AO
    buffers, unless glossy_pass, area_pass or ao_pass of this frame wrote them: have_rays), then the closest-hit hemisphere
    walk through c's uniform grid into f.gi_sum.  gi: Renderer._gi_stage's (S, (set_w, set_h), table, radius, gain, gather, shadows);
    shadow_light: the point the hits are shadowed from, or None.  Runs behind the uniform grid's build and before the
    shading call that rewrites the ids."""
    uvalue, uspan, uoffset, _ = c.grid_ptrs(GRID_UNIFORM)
    if not have_rays:
        c.ao_rays(cam_pos, f.t, f.dir, f.intersect_id, f.d_verts, f.d_faces, f.reflect_eps, f.ao_rays, f.ao_active)
    c.gi_gather(uvalue, uspan, uoffset, f.d_verts, f.d_faces, f.ao_rays, f.ao_active, gi[0], gi[1][0], gi[1][1], gi[2], gi[3],
                f.d_matidx, f.d_matlist, f.num_materials, shadow_light, f.reflect_eps, f.gi_sum)


def gi_shade(c, f, gi):
    """The indirect light onto the image, behind the frame's own shading (gi_pass' gi): with a gather ((radius, cos,
    plane)) gi_filter over f.gi_sum into f.gi_acc, then gi_apply."""
    acc = f.gi_sum
    if gi[5] is not None:
        c.gi_filter(f.gi_sum, f.ao_rays, f.ao_active, gi[5][0], gi[5][1], gi[5][2], f.gi_acc)
        acc = f.gi_acc
    c.gi_apply(f.image, acc, gi[0], gi[4], f.intersect_id, f.d_matlist, f.num_materials)


def glossy_pass(c, f, cam_pos, gl, shadow_light):
    """The lobe's gather, behind reflect_rays (f.rays / f.active: {o, R} of the pixels whose
    material reflects) and the uniform grid's build: {origin, normal} of every primary hit (ao_rays, into the AO buffers;
    the frame's other effects read them from there), then the closest-hit walk of the lobe's rays through c's uniform grid
    into f.glossy_sum.  gl: Renderer._glossy_stage's (S, (set_w, set_h), table, radius, gather, shadows); shadow_light: the
    point the hits are shadowed from, or None.  Runs before the shading call that rewrites the ids."""
    uvalue, uspan, uoffset, _ = c.grid_ptrs(GRID_UNIFORM)
    c.ao_rays(cam_pos, f.t, f.dir, f.intersect_id, f.d_verts, f.d_faces, f.reflect_eps, f.ao_rays, f.ao_active)
    c.glossy_gather(uvalue, uspan, uoffset, f.d_verts, f.d_faces, f.rays, f.active, f.ao_rays, f.intersect_id, f.d_matidx,
                    f.d_spread, gl[0], gl[1][0], gl[1][1], gl[2], gl[3], f.d_matlist, f.num_materials, shadow_light,
                    f.reflect_eps, f.glossy_sum)


def glossy_shade(c, f, gl):
    """The lobe's mean into the image, directly behind the frame's shading call (glossy_pass' gl): with a gather ((radius,
    cos, plane)) gi_filter over f.glossy_sum into f.glossy_acc -- among the pixels that carry a lobe: f.active stands in
    the place of the origins' flags --, then glossy_apply."""
    acc = f.glossy_sum
    if gl[4] is not None:
        c.gi_filter(f.glossy_sum, f.ao_rays, f.active, gl[4][0], gl[4][1], gl[4][2], f.glossy_acc)
        acc = f.glossy_acc
    c.glossy_apply(f.image, acc, gl[0], f.intersect_id, f.d_reflect, f.num_materials)


def temporal_blend(c, f, tp, st, call, sums, S, out):
    """One effect's temporal call: this frame's gathered sums into the effect's running mean and
    the pair its shading call takes.  tp: Renderer._temporal_begin's frame record; st: the effect's state, whose two
    histories change roles here and whose frame counter advances; call: "temporal_visibility" or "temporal_gi"."""
    turn = st["turn"]
    getattr(c, call)(sums, S, f.ao_rays, f.ao_active, tp["prev_cam"], f.prev_ao_rays, f.prev_ao_active, st["hist"][turn],
                     tp["max"], tp["cos"], tp["plane"], st["hist"][1 - turn], out)
    st["turn"] = 1 - turn
    st["n"] += 1


def ao_shade_temporal(c, f, tp, ao):
    """ao_shade in a temporal frame (ao: Renderer._temporal_ao's): the gather (radius 0 without ao_filter: it forms the
    pair), the running mean, and shade_ao_vis from the mean."""
    dirs, _, sets, st = ao
    c.filter_visibility(f.ao_mask, len(dirs), f.ao_rays, f.ao_active, sets[2][0], sets[2][1], sets[2][2], f.ao_vis)
    temporal_blend(c, f, tp, st, "temporal_visibility", f.ao_vis, len(dirs), f.ao_tvis)
    c.shade_ao_vis(f.image, f.ao_tvis, len(dirs))


def area_shade_temporal(c, f, tp, area):
    """The penumbra of a temporal frame (area: Renderer._temporal_area's): gather, running mean, shade_area_vis."""
    S, _, _, gather, st = area
    c.filter_visibility(f.area_mask, S, f.ao_rays, f.ao_active, gather[0], gather[1], gather[2], f.area_vis)
    temporal_blend(c, f, tp, st, "temporal_visibility", f.area_vis, S, f.area_tvis)
    c.shade_area_vis(f.image, f.area_tvis, S)


def gi_shade_temporal(c, f, tp, gi):
    """gi_shade in a temporal frame (gi: Renderer._temporal_gi's): gi_filter, the running mean of the three channels,
    gi_apply from the mean."""
    c.gi_filter(f.gi_sum, f.ao_rays, f.ao_active, gi[5][0], gi[5][1], gi[5][2], f.gi_acc)
    temporal_blend(c, f, tp, gi[7], "temporal_gi", f.gi_acc, gi[0], f.gi_tacc)
    c.gi_apply(f.image, f.gi_tacc, gi[0], gi[4], f.intersect_id, f.d_matlist, f.num_materials)


def aa_edges(c, f, cam_pos, aa, shadows):
    """The anti-aliasing's edge flags into f.aa_edge, behind the shadow stage and before the
    shading call that rewrites the ids.  aa: Renderer._aa_stage's (S, (set_w, set_h), table, cos, plane, shadows); shadows:
    the frame has a shadow stage and the edges of its shadows count."""
    c.aa_edges(f.normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx, f.is_shadowed if shadows else None, aa[3], aa[4],
               f.aa_edge)


def aa_pass(c, f, eye_camcoords, aa, shadow_light):
    """The sub-pixel eye rays of the flagged pixels through c's uniform grid into f.aa_sum (aa_edges' aa); eye_camcoords:
    the eye's block (the context holds the light camera's by now); shadow_light: the point the samples are shadowed
    from, or None."""
    uvalue, uspan, uoffset, _ = c.grid_ptrs(GRID_UNIFORM)
    c.aa_gather(uvalue, uspan, uoffset, f.d_verts, f.d_faces, eye_camcoords, f.aa_edge, aa[0], aa[1][0], aa[1][1], aa[2],
                f.d_matidx, f.d_matlist, f.num_materials, shadow_light, f.reflect_eps, f.aa_sum)


def dof_pixels(c, f, dof):
    """The depth of field's pixel flags into f.dof_flag, behind the shadow stage and before the
    shading call that rewrites the ids.  dof: Renderer._dof_stage's (S, (set_w, set_h), table, lens, coc_scale, min,
    window, shadows)."""
    lens = dof[3]
    c.dof_pixels(f.t, f.dir, f.intersect_id, lens[6:9], float(lens[9]), dof[4], dof[5], dof[6], f.dof_flag)


def dof_pass(c, f, eye_camcoords, dof, shadow_light):
    """The lens rays of the flagged pixels through c's uniform grid into f.dof_sum (dof_pixels' dof); eye_camcoords and
    shadow_light as in aa_pass."""
    uvalue, uspan, uoffset, _ = c.grid_ptrs(GRID_UNIFORM)
    c.dof_gather(uvalue, uspan, uoffset, f.d_verts, f.d_faces, eye_camcoords, dof[3], f.dof_flag, dof[0], dof[1][0], dof[1][1],
                 dof[2], f.d_matidx, f.d_matlist, f.num_materials, shadow_light, f.reflect_eps, f.dof_sum)


def area_pass(c, f, cam_pos, samples, thru=None, sets=None, have_rays=False):
    """An area light's shadow rays and walk: the origin of every primary hit (ao_rays, into the AO
    buffers), then the any-hit walk towards the points `samples` of the light's disk through c's uniform grid into
    f.area_mask.  thru (a refract frame: (mat_idx, transmit, num_materials)): the walk that sees through glass.  sets
    ((num_samples, set_w, set_h)): `samples` is the device table of a set per pixel of the tile,
    and the walk is the one over sample sets.  have_rays: glossy_pass of this frame wrote the origins already (area_pass is
    the first of the frame's other passes: ao_pass and gi_pass read what it wrote).  Runs
    behind the uniform grid's build and before the shading call that rewrites the ids."""
    uvalue, uspan, uoffset, _ = c.grid_ptrs(GRID_UNIFORM)
    if not have_rays:
        c.ao_rays(cam_pos, f.t, f.dir, f.intersect_id, f.d_verts, f.d_faces, f.reflect_eps, f.ao_rays, f.ao_active)
    if sets is not None:
        any_hit(c, "trace_dda_any_area_sets", thru, uvalue, uspan, uoffset, f.d_verts, f.d_faces, f.ao_rays, f.ao_active,
                sets[0], sets[1], sets[2], samples, f.area_mask)
    else:
        any_hit(c, "trace_dda_any_area", thru, uvalue, uspan, uoffset, f.d_verts, f.d_faces, f.ao_rays, f.ao_active,
                samples, f.area_mask)


def shade_frame(c, f, cam_pos, frame_cnt, shadows, reflect, bounces, reflect_shadows=False, glossy=None, normal=None,
                fresnel=None, albedo=None):
    """simpleShade | spotlight_shade, or the reflections' shading (shade_reflect at depth 1; with reflect_shadows the
    depth shading with the occluded levels darkened, at every depth), then add_shadows.  glossy (glossy_pass' gl): the
    lobe's blend directly behind the shading call, where the mirror frame has its own.  normal (smooth_pass'): the normals
    simpleShade | spotlight_shade read, f.normal unless given.  fresnel (check_fresnel's pair): shade_fresnel over
    fresnel_pass' sums in the place of the reflections' shading.  albedo (texture_pass'): texture_shade |
    texture_shade_spotlight in simpleShade's | spotlight_shade's place."""
    if fresnel:
        c.shade_fresnel(f.image, f.normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx, f.d_matlist, f.num_materials,
                        f.f_acc)
    elif reflect and reflect_shadows:
        c.shade_reflect_depth_occluded(f.image, f.normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx, f.d_matlist,
                                       level_weights(f), f.num_materials, f.d_verts, f.d_faces, bounces, f.rays_levels,
                                       f.active_levels, f.hit_t_levels, f.hit_id_levels, f.occluded_levels)
    elif reflect and bounces == 1:
        c.shade_reflect(f.image, f.normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx, f.d_matlist,
                        level_weights(f), f.num_materials, f.d_verts, f.d_faces, f.rays, f.active, f.hit_t, f.hit_id)
    elif reflect:
        c.shade_reflect_depth(f.image, f.normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx, f.d_matlist,
                              level_weights(f), f.num_materials, f.d_verts, f.d_faces, bounces, f.rays_levels,
                              f.active_levels, f.hit_t_levels, f.hit_id_levels)
    elif albedo is not None and frame_cnt < 2:
        c.texture_shade(f.image, f.normal if normal is None else normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx,
                        f.d_matlist, f.num_materials, albedo)
    elif albedo is not None:
        c.texture_shade_spotlight(f.image, f.normal if normal is None else normal, f.t, f.dir, f.intersect_id, cam_pos,
                                  f.d_matidx, f.d_matlist, f.num_materials, albedo)
    elif frame_cnt < 2:
        c.shade_simple(f.image, f.normal if normal is None else normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx,
                       f.d_matlist,
                       f.num_materials)
    else:
        c.shade_spotlight(f.image, f.normal if normal is None else normal, f.t, f.dir, f.intersect_id, cam_pos, f.d_matidx,
                          f.d_matlist,
                          f.num_materials)
    if glossy is not None:
        glossy_shade(c, f, glossy)
    if shadows:
        c.shade_add_shadows(f.image, f.is_shadowed)


class FrameSetup:
    def __init__(self, camera, light_camera, shading_light, fovy=45.0, lights=None):
        """lights: a sequence of (light_camera_params, shading_light) pairs, 1..MAX_LIGHTS of them, that the
        one-stream Renderer renders instead of light_camera / shading_light; None: the
        single-light frame."""
        self.camera, self.light_camera, self.shading_light, self.fovy = camera, light_camera, shading_light, fovy
        self.lights = lights

    @staticmethod
    def from_scene(info, cam="ref", lights=None):
        cams = info["cameras"]
        return FrameSetup(cams[cam] if cam in cams else next(iter(cams.values())), info["light_camera"],
                          info["shading_light"], lights=lights)


def make_camera(params, fovy, aspect):
    c = Camera(fovy, aspect)
    c.setCameraCenter(*params["eye"])
    c.setCameraLookAt(*params["look"])
    c.setCameraUp(*params["up"])
    c.setNearFar(params["near"], params["far"])
    return c.adjustCameraAndPosition()


class _Frame:
    """The scene on the device and the arrays of a whole frame, which every context that renders rows of it writes
    (pixel ids are global)."""

    def __init__(self, ctx, verts, faces, matidx, mat_list, reflect, reflect_eps, transmit=None, ior=None):
        t = ctx.torch
        self.F = int(len(faces))
        self.num_materials = int(len(mat_list) // 6 if np.ndim(mat_list) == 1 else len(mat_list))
        self.d_verts = ctx.upload(np.asarray(verts, np.float32).reshape(-1))
        self.d_faces = ctx.upload(np.asarray(faces, np.int32).reshape(-1))
        self.d_matidx = ctx.upload(np.asarray(matidx, np.int32).reshape(-1))
        self.d_matlist = ctx.upload(np.asarray(mat_list, np.float32).reshape(-1))
        refl = np.zeros(self.num_materials, np.float32) if reflect is None else np.asarray(reflect, np.float32)
        self.d_reflect = ctx.upload(refl)
        # refraction: how much of a material's colour comes from behind it, its index, and the
        # weight of the next level in a refract frame -- a glass material's transmit, otherwise its reflect
        tr = np.zeros(self.num_materials, np.float32) if transmit is None else np.asarray(transmit, np.float32)
        ni = np.ones(self.num_materials, np.float32) if ior is None else np.asarray(ior, np.float32)
        self.d_transmit = ctx.upload(tr)
        self.d_ior = ctx.upload(ni)
        self.d_continue = ctx.upload(np.where(tr > 0, tr, refl).astype(np.float32))
        self.refract = False  # this frame's display(..., refract=): read by the stages
        v = np.asarray(verts, np.float32).reshape(-1, 3)
        self.bbmin, self.bbmax = v.min(0), v.max(0)
        N = ctx.width * ctx.height
        self.N = N
        # DecisionData, decision_data.h:64-78
        self.normal = ctx.empty(3 * N, t.float32)
        self.t = ctx.empty(N, t.float32)
        self.dir = ctx.empty(3 * N, t.float32)
        self.is_shadowed = ctx.empty(N, t.int32)
        self.intersect_id = ctx.empty(N, t.int32)
        self.image = t.zeros(3 * N, dtype=t.uint8, device=ctx.device)
        self.torch = t
        # the reflection levels 1..D one behind the other (_ensure_reflect_buffers)
        self.rays = self.active = self.hit_t = self.hit_id = None
        self.rays_levels = self.active_levels = self.hit_t_levels = self.hit_id_levels = None
        # reflect_shadows: the levels' occlusion flags, and the occlusion rays of the level that is being traced
        self.occluded_levels = self.occlusion_rays = self.occlusion_active = None
        # FrameSetup.lights: the lights' shadow flags one behind the other (_ensure_light_buffers)
        self.shadowed_lights = None
        # reflect_lights with reflect_shadows: the levels' occlusion flags per light, a contiguous [D, L, W*H] view of
        # _occluded_lights_store (_ensure_reflect_lights_buffers)
        self.occluded_lights = self._occluded_lights_store = None
        # ao: the hemisphere rays' origins and normals, their active flags and the mask of occluded directions
        # (_ensure_ao_buffers); the direction sets asked for so far, by their size
        self.ao_rays = self.ao_active = self.ao_mask = None
        self._ao_dirs = {}
        # area: the mask of occluded samples of the light's disk (_ensure_area_buffers; the origins share ao_rays)
        self.area_mask = None
        # area_filter: the gather's two sums per pixel (_ensure_area_filter_buffers); area_sets: the uploaded tables
        self.area_vis = None
        self._area_set_tables = {}
        # ao_filter: the gather's two sums per pixel (_ensure_ao_filter_buffers); ao_sets: the uploaded tables (_ao_stage)
        self.ao_vis = None
        self._ao_set_tables = {}
        # gi: the byte sums of the indirect light's samples and the gather's sums, four words per pixel
        # (_ensure_gi_buffers; the origins share ao_rays); the uploaded direction tables by (gi, gi_sets) (_gi_stage)
        self.gi_sum = self.gi_acc = None
        self._gi_set_tables = {}
        # aa: the edge flags and the byte sums of the supersampled pixels, four words per pixel (_aa_stage); the uploaded
        # offset tables by (aa, aa_sets)
        self.aa_edge = self.aa_sum = None
        self._aa_set_tables = {}
        # dof: the lens flags and the byte sums of the pixels seen through the lens, four words per pixel (_dof_stage); the
        # uploaded sample tables by (dof, dof_sets)
        self.dof_flag = self.dof_sum = None
        self._dof_set_tables = {}
        # glossy: the byte sums of the lobe's samples and the gather's sums, four words per pixel (_ensure_glossy_buffers;
        # the rays are level 1's, the normals ao_rays'); the uploaded point tables by (glossy, glossy_sets) (_glossy_stage)
        self.glossy_sum = self.glossy_acc = None
        self._glossy_tables = {}
        # fresnel: the ray trees' sums, four float32 words per pixel (_ensure_fresnel_buffers; the rays are level 1's)
        self.f_acc = None
        # temporal: the previous frame's {o, n} and active flags (they change places with ao_rays / ao_active at the start
        # of every temporal frame), the temporal calls' outputs, the effects' states by name -- two histories, which of
        # them is read next, frames since the reset, the parameters they were accumulated under --, the 16 rotated tables
        # per key, and the eye's block of the frame before (Renderer._temporal_begin)
        self.prev_ao_rays = self.prev_ao_active = None
        self.ao_tvis = self.area_tvis = self.gi_tacc = None
        self._temporal = {}
        self._temporal_set_tables = {}
        self._temporal_prev_cam = None
        self._temporal_live = False
        self._temporal_serial = 0
        self.reflect_eps = float(reflect_eps)
        self.aspect = float(np.float32(ctx.width) / np.float32(ctx.height))

    def _ensure_ao_buffers(self, ao):
        """ao_rays [6 W*H], ao_active [W*H] and ao_mask [W*H] (uint32 words in an int32 tensor), allocated on first use;
        returns the ao directions of scenes.ao_directions."""
        t, N, dev = self.torch, self.N, self.image.device
        if self.ao_rays is None:
            self.ao_rays = t.empty(6 * N, dtype=t.float32, device=dev)
            self.ao_active = t.empty(N, dtype=t.int32, device=dev)
        if self.ao_mask is None:
            self.ao_mask = t.zeros(N, dtype=t.int32, device=dev)
        if ao not in self._ao_dirs:
            from .scenes import ao_directions

            self._ao_dirs[ao] = ao_directions(ao)
        return self._ao_dirs[ao]

    def _ensure_area_buffers(self):
        """area_mask [W*H] (uint32 words in an int32 tensor) and the origins' buffers ao_rays / ao_active, allocated on
        first use."""
        t, N, dev = self.torch, self.N, self.image.device
        if self.ao_rays is None:
            self.ao_rays = t.empty(6 * N, dtype=t.float32, device=dev)
            self.ao_active = t.empty(N, dtype=t.int32, device=dev)
        if self.area_mask is None:
            self.area_mask = t.zeros(N, dtype=t.int32, device=dev)

    def _ensure_area_filter_buffers(self):
        """area_vis [2 W*H] (uint32 words in an int32 tensor), allocated on first use."""
        if self.area_vis is None:
            self.area_vis = self.torch.zeros(2 * self.N, dtype=self.torch.int32, device=self.image.device)

    def _ensure_light_buffers(self, num_lights):
        """shadowed_lights [L, W*H]: light l's is_shadowed, allocated once for the most lights asked for."""
        t = self.torch
        if self.shadowed_lights is None or self.shadowed_lights.shape[0] < num_lights:
            self.shadowed_lights = t.empty((num_lights, self.N), dtype=t.int32, device=self.image.device)

    def _ensure_reflect_lights_buffers(self, bounces, num_lights, reflect_shadows):
        """The reflect buffers, and with reflect_shadows occluded_lights [bounces, num_lights, W*H]: a view of a store that
        is allocated once for the most (D, L) asked for, contiguous so that the kernels' light stride is this frame's L;
        the occlusion rays and their active flags are one level's, as in the single-light frame."""
        t, N, dev = self.torch, self.N, self.image.device
        self._ensure_reflect_buffers(bounces, False)
        if not reflect_shadows:
            return
        if self._occluded_lights_store is None or self._occluded_lights_store.numel() < bounces * num_lights * N:
            self._occluded_lights_store = t.empty(bounces * num_lights * N, dtype=t.int32, device=dev)
        self.occluded_lights = self._occluded_lights_store[:bounces * num_lights * N].view(bounces, num_lights, N)
        if self.occlusion_rays is None:
            self.occlusion_rays = t.empty(6 * N, dtype=t.float32, device=dev)
            self.occlusion_active = t.empty(N, dtype=t.int32, device=dev)

    def _ensure_fresnel_buffers(self):
        """f_acc [4 W*H] float32 and level 1's rays and active words, allocated on first use."""
        self._ensure_reflect_buffers(1, False)
        if self.f_acc is None:
            self.f_acc = self.torch.zeros(4 * self.N, dtype=self.torch.float32, device=self.image.device)

    def _ensure_reflect_buffers(self, bounces=1, reflect_shadows=False):
        """rays_levels / active_levels / hit_t_levels / hit_id_levels: [depth, W*H(*6)], allocated once for the
        deepest frame asked for; rays / active / hit_t / hit_id are level 1's views.  reflect_shadows: also
        occluded_levels [depth, W*H] and one level's occlusion rays [6 W*H] and their active flags [W*H]."""
        t, N, dev = self.torch, self.N, self.image.device
        if reflect_shadows and (self.occluded_levels is None or self.occluded_levels.shape[0] < bounces):
            self.occluded_levels = t.empty((bounces, N), dtype=t.int32, device=dev)
            if self.occlusion_rays is None:
                self.occlusion_rays = t.empty(6 * N, dtype=t.float32, device=dev)
                self.occlusion_active = t.empty(N, dtype=t.int32, device=dev)
        if self.rays_levels is not None and self.rays_levels.shape[0] >= bounces:
            return
        self.rays_levels = t.empty((bounces, 6 * N), dtype=t.float32, device=dev)
        self.active_levels = t.empty((bounces, N), dtype=t.int32, device=dev)
        self.hit_t_levels = t.empty((bounces, N), dtype=t.float32, device=dev)
        self.hit_id_levels = t.empty((bounces, N), dtype=t.int32, device=dev)
        self.rays, self.active = self.rays_levels[0], self.active_levels[0]
        self.hit_t, self.hit_id = self.hit_t_levels[0], self.hit_id_levels[0]


class _Band:
    """What each context that renders rows of a frame owns besides the frame's arrays: d_cam_position with the pinned
    staging that feeds it, and the ray map, chunk starts and chunk count of its shadow pass."""

    def __init__(self, ctx):
        t = ctx.torch
        self.ctx = ctx
        self.cam_pos = ctx.empty(3, t.float32)
        # pinned staging for d_cam_position: a pageable-memory copy would make the host wait for the whole
        # previous frame before it may enqueue the next one.  Two buffers alternate and an event behind each copy
        # is waited for before the buffer is rewritten, so no other call has to synchronise for this to be safe
        self._cam_pos_host = [t.empty(3, dtype=t.float32).pin_memory() for _ in range(2)]
        self._cam_pos_done = [None, None]  # event behind the copy out of each staging buffer
        self._cam_pos_turn = 0
        self._d_map = ctx.empty(2 * ctx.npix, t.int32)
        self._prefix = ctx.empty(ctx.prefix_capacity(), t.int32)
        self._num_chunks = 0

    def _upload_cam_pos(self, worldori):
        """main.cu:128 d_cam_position <- worldori, without a host wait in the steady state."""
        t = self.ctx.torch
        k = self._cam_pos_turn
        self._cam_pos_turn = 1 - k
        if self._cam_pos_done[k] is not None:
            self._cam_pos_done[k].synchronize()  # the copy that read this buffer two frames ago
        self._cam_pos_host[k].copy_(t.from_numpy(worldori[:3].copy()))
        self.cam_pos.copy_(self._cam_pos_host[k], non_blocking=True)
        ev = t.cuda.Event()
        ev.record(t.cuda.current_stream(self.ctx.device))
        self._cam_pos_done[k] = ev

    @property
    def num_chunks(self):
        """h_numCudaBlocks of the last frame (fetched from the device on first use: the frame loop itself
        never waits for it)."""
        if self._num_chunks == 0xFFFFFFFF:
            self._num_chunks = self.ctx.sort_rays_chunks()
        return self._num_chunks

    # The ray map sorted by light cell and the chunk starts (processData's outputs).  With FLAG_SHADOW_ALL_CHUNKS a frame
    # does not need them (ugrt_sort_rays, deferred form): they are produced when they are looked at.
    @property
    def d_map(self):
        self.num_chunks
        return self._d_map

    @property
    def prefix(self):
        self.num_chunks
        return self._prefix


class Renderer(_Frame, _Band):
    def __init__(self, ctx, verts, faces, matidx, mat_list, reflect=None, transmit=None, ior=None, reflect_eps=1e-3,
                 overlap=False, shards=None, helper_thread=True, aux_stream=None, batch_builds=False, spread=None,
                 vertex_key=None, uvs=None, uv_faces=None, textures=None, mat_texture=None):
        """uvs [T, 2] floats, uv_faces [F, 3] ints (an index into uvs per corner of the face list; outside 0..T-1: none),
        textures (a list of uint8 arrays [H, W, 3], row 0 at v = 0) and mat_texture (one int per material: its texture, -1:
        none), for display(..., textures=True); None: no uvs, no textures.  They are checked here;
        the atlas is built by the first textured frame, once.
        vertex_key: one int per vertex, in 0..V-1 (scenes.weld; None: every vertex is its own key), for
        display(..., smooth=True): the faces around the vertices of one key share their normals.
        spread: per material, the tangent of the half-angle of its reflection lobe (scenes.spread_from_sharpness; None:
        zeros, mirrors), for display(..., glossy=S).
        transmit, ior: per material, how much of its colour comes from behind it (0: opaque, the default) and its index
        of refraction (default 1), for display(..., refract=True).
        overlap=True: the light grid and the uniform grid (which do not depend on the camera pass) are built
        by a second context on a second HIP stream while the main stream builds the perspective grid and
        traces the primary rays; streams are joined with events before the grids are consumed.  Same results.
        A grid build blocks its caller once (the read-back of total_refs), so the second context is driven by
        a helper thread: both streams then really run side by side."""
        self.aux = None
        self._worker = None
        # parallel.GridShards: the light grid and the uniform grid are built in shards of the triangle list, one
        # per rank, exchanged and merged; one-stream frames only
        self.shards = shards
        assert not (overlap and shards is not None), "sharded builds run in the one-stream frame"
        # (two-stream frame from one host thread: the light and the uniform build may share their sorts' launches --
        # three launches less per frame, measured 2 % SLOWER with four frames in flight and equal with one:
        # profiles/r04_batched_builds.txt -- so it is off unless asked for)
        self.batch_builds = batch_builds
        self._inline = overlap and not helper_thread
        if overlap:
            self._make_side_context(ctx, aux_stream, helper_thread)
        _Frame.__init__(self, ctx, verts, faces, matidx, mat_list, reflect, reflect_eps, transmit, ior)
        _Band.__init__(self, ctx)
        self.orig = None
        spr = np.zeros(self.num_materials, np.float32) if spread is None else np.asarray(spread, np.float32).reshape(-1)
        if len(spr) != self.num_materials:
            raise ValueError("spread must hold one value per material (%d), not %d" % (self.num_materials, len(spr)))
        self.d_spread = ctx.upload(spr)
        # smooth shading: the host arrays are checked here, the device side is made by the first
        # smooth frame (_smooth_stage)
        V = len(np.asarray(verts).reshape(-1)) // 3
        f = np.asarray(faces).reshape(-1)
        self._smooth_faces_ok = bool(f.size == 0 or (f.min() >= 0 and f.max() < V))
        self._vertex_key = None
        if vertex_key is not None:
            key = np.asarray(vertex_key)
            if key.ndim != 1 or len(key) != V or not np.issubdtype(key.dtype, np.integer) \
                    or (V and (key.min() < 0 or key.max() >= V)):
                raise ValueError("vertex_key must hold one integer in 0..%d per vertex (%d)" % (V - 1, V))
            self._vertex_key = key.astype(np.int32)
        # texture mapping: checked here, the device side is made by the first textured frame
        # (_texture_stage)
        self._tex = None
        F = len(f) // 3
        tl = [] if textures is None else [np.asarray(a) for a in textures]
        if len(tl) > MAX_TEXTURES:
            raise ValueError("textures holds %d arrays, at most %d fit" % (len(tl), MAX_TEXTURES))
        for a in tl:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or not (1 <= a.shape[0] <= MAX_TEXTURE_DIM) \
                    or not (1 <= a.shape[1] <= MAX_TEXTURE_DIM):
                raise ValueError("a texture is a uint8 array [H, W, 3] with H, W in 1..%d, not %s %r"
                                 % (MAX_TEXTURE_DIM, a.dtype, a.shape))
        mt = np.full(self.num_materials, -1, np.int32) if mat_texture is None else np.asarray(mat_texture)
        if mt.ndim != 1 or len(mt) != self.num_materials or not np.issubdtype(mt.dtype, np.integer) \
                or (len(mt) and mt.max() >= len(tl)):
            raise ValueError("mat_texture must hold one integer below %d per material (%d)" % (len(tl), self.num_materials))
        uv = np.zeros((0, 2), np.float32) if uvs is None else np.asarray(uvs)
        if uv.ndim != 2 or uv.shape[1] != 2 or not (np.issubdtype(uv.dtype, np.floating) or np.issubdtype(uv.dtype, np.integer)):
            raise ValueError("uvs must be numbers [T, 2], not %r" % (uv.shape,))
        uf = np.full((F, 3), -1, np.int32) if uv_faces is None else np.asarray(uv_faces)
        if uf.shape != (F, 3) or not np.issubdtype(uf.dtype, np.integer):
            raise ValueError("uv_faces must hold three integers per face (%d), not %r" % (F, uf.shape))
        self._tex_host = (uv.astype(np.float32), uf.astype(np.int32), tl, mt.astype(np.int32))

    def _make_side_context(self, ctx, aux_stream, helper_thread):
        from .device import Context

        t = ctx.torch
        self.main_stream = t.cuda.current_stream(ctx.device)
        # (aux_stream: a stream the caller made; which streams end up on the same hardware queue depends on
        # the order in which they were created)
        self.aux_stream = aux_stream if aux_stream is not None else t.cuda.Stream(ctx.device)
        with t.cuda.stream(self.aux_stream):
            self.aux = Context(ctx.width, ctx.height, device=ctx.device_index, light_grid=ctx.light_grid,
                               rows=ctx.rows, flags=int(ctx.cfg.flags),
                               uniform_dims=tuple(ctx.cfg.uniform_dims[k] for k in range(3)),
                               slabs=int(ctx.cfg.slabs))
        if not helper_thread:
            # builds that never wait for the device (option async_build): one host thread keeps both streams fed
            ctx.set_option("async_build", 1)
            self.aux.set_option("async_build", 1)
        # the bounce runs beside the ray sort and the shadow pass and has slack: four persistent waves per CU leave
        # the registers and LDS of every CU to the main stream's workgroups (with the whole chip taken by
        # the bounce's waves, a sort pass of the main stream waited 0.2 ms for room)
        self.aux.set_option("dda_blocks", 1024)
        if not helper_thread:
            return
        import queue
        import threading

        self._jobs, self._done = queue.Queue(), queue.Queue()

        def loop():
            while True:
                job = self._jobs.get()
                if job is None:
                    return
                try:
                    job()
                    self._done.put(None)
                except BaseException as e:  # handed to the frame loop
                    self._done.put(e)

        self._worker = threading.Thread(target=loop, name="ugrt-aux", daemon=True)
        self._worker.start()

    # Model::init_orig_list, scene.h:336
    def init_orig_list(self, size, offset):
        self.orig = self.d_verts[3 * offset:3 * (offset + size)].clone()
        self.orig_size, self.orig_offset = size, offset

    # Model::rotate_bunny, scene.h:122
    def rotate_bunny(self, rot):
        self.ctx.animate(self.d_verts, self.orig, self.orig_size, self.orig_offset, rot)
        if self.aux is not None:
            self.aux.geometry_changed()  # the second context did not see the call
        self.temporal_reset()
        if getattr(self, "_smooth", None) is not None:
            self._smooth["normals"] = None  # the vertices moved: the corner normals are formed again

    def geometry_changed(self):
        """The vertex or face array was rewritten outside rotate_bunny: Context.geometry_changed on every context, and the
        temporal histories start again."""
        self.ctx.geometry_changed()
        if self.aux is not None:
            self.aux.geometry_changed()
        self.temporal_reset()
        if getattr(self, "_smooth", None) is not None:
            self._smooth["adjacency"] = False  # the faces may be others: the adjacency and the corner normals again
            self._smooth["normals"] = None

    def temporal_reset(self):
        """Every effect's running mean starts again with the next temporal frame: the frame
        counters go back to 0 and the histories are cleared in stream order.  display does this by itself when the
        geometry changes (rotate_bunny, geometry_changed), when an effect's parameters or, for area, the light change
        (that effect only), and when the frame before was not a temporal one.  A renderer that never rendered a
        temporal frame enqueues nothing here."""
        for st in getattr(self, "_temporal", {}).values():
            self._temporal_clear(st)

    def _temporal_clear(self, st):
        st["hist"][st["turn"]].zero_()  # (the one the next call reads; it rewrites the other one whole)
        st["n"] = 0

    def temporal_history(self, name):
        """The running mean of effect `name` ("ao", "area": floats [2 W*H], (share, frames) per pixel; "gi": [4 W*H],
        (r, g, b, frames)) as the last temporal frame left it."""
        st = self._temporal[name]
        return st["hist"][st["turn"]]

    def close(self):
        """Stops the helper thread of an overlapped renderer."""
        if self._worker is not None:
            self._jobs.put(None)
            self._worker.join()
            self._worker = None

    def display(self, setup, frame_cnt=1, shadows=True, reflect=False, shade=True, bounces=1, reflect_shadows=False,
                reflect_lights=False, ao=0, ao_radius=None, refract=False, area=0, area_radius=None, area_sets=1,
                area_filter=0, area_filter_cos=0.9, area_filter_plane=None, ao_sets=1, ao_filter=0, ao_filter_cos=0.9,
                ao_filter_plane=None, gi=0, gi_radius=None, gi_gain=1.0, gi_shadows=True, gi_sets=1, gi_filter=0,
                gi_filter_cos=0.9, gi_filter_plane=None, aa=0, aa_sets=1, aa_cos=0.9, aa_plane=None, aa_shadows=True,
                temporal=0, temporal_cos=0.9, temporal_plane=None, glossy=0, glossy_sets=1, glossy_filter=0,
                glossy_filter_cos=0.9, glossy_filter_plane=None, glossy_radius=None, glossy_shadows=True, smooth=False,
                smooth_cos=0.5, smooth_signed=False, dof=0, dof_aperture=0.0, dof_focus=None, dof_sets=1, dof_min=0.5,
                dof_window=4, dof_shadows=True, textures=False, texture_aniso=8, texture_bias=0, fresnel=False, fresnel_cut=0.0):
        """bounces: levels of reflection with reflect=True (1..8; 1 = the single bounce).  rays_levels /
        active_levels / hit_t_levels / hit_id_levels hold every level and rays / active / hit_t / hit_id are level
        1's views.  reflect_shadows (needs reflect=True): the hits of every reflection level are shadowed (from the light
        camera's eye, the point the primary shadow pass is cast from); occluded_levels holds the levels' flags.
        setup.lights (one-stream renderer, reflect=False): the shadow stage once per light into shadowed_lights, then one
        Lambertian shading pass over all of them, whatever frame_cnt says.
        reflect_lights (one-stream renderer; needs reflect=True and setup.lights): the reflections of depth `bounces` under
        all of setup.lights -- per light its shadow stage, per level one any-hit launch towards every light (with
        reflect_shadows; occluded_lights holds the flags [D, L, W*H]), one shading pass.
        ao (one-stream renderer, every frame above; 0: off): ambient occlusion with ao = 1..32 hemisphere rays
        (scenes.ao_directions) of length ao_radius per primary hit; ao_mask holds the occluded directions' bits and the
        image is scaled by the share of open rays behind the frame's own shading.
        refract (needs reflect=True; every frame that takes reflect): a level's ray goes through a hit whose material
        has transmit > 0 (Snell's law with the material's ior; total internal reflection mirrors) and is mirrored where
        the material only reflects; the shading weighs the next level with transmit there; with reflect_shadows the
        any-hit walk does not count glass as an occluder.  The primary shadow stage still does: a glass ball casts a
        full shadow.
        area (one-stream renderer, single-light frames, needs shadows=True; 0: off): the light is a disk of radius
        area_radius around the light camera's eye, perpendicular to its view; area = 1..32 shadow rays per primary hit
        towards scenes.area_samples' points of it walk the uniform grid in the place of the light-space shadow stage
        (is_shadowed is left alone), area_mask holds the occluded samples' bits and the image goes from b (every sample
        lit) to b / 3 (none); with refract the walk sees through glass.
        area_sets (needs area > 0; 1, 4 or 16): the pixels of a 1 x 1, 2 x 2 or 4 x 4 tile aim at different sets of `area`
        points (scenes.area_sample_sets; the table is uploaded once per (area, area_sets, area_radius, light)).
        area_filter (needs area > 0; 0: off): a gather of radius 1..8 over the pixels of the same surface -- normals within
        area_filter_cos, planes within area_filter_plane (None: 1 % of the scene's largest extent) -- averages the masks
        before the penumbra is shaded; area_vis holds its sums.
        ao_sets (needs ao > 0; 1, 4 or 16): the pixels of a 1 x 1, 2 x 2 or 4 x 4 tile walk along different sets of `ao`
        directions (scenes.ao_direction_sets; the table is uploaded once per (ao, ao_sets)) in the pixel-major walk.
        ao_filter (needs ao > 0; 0: off): area_filter's gather, with ao_filter_cos and ao_filter_plane, over ao_mask
        before the image is scaled; ao_vis holds its sums.
        gi (one-stream renderer, single-light frames, plain or reflect, with or without refract; ao and area compose; 0:
        off): one bounce of indirect diffuse light -- every primary hit sends gi = 1..32 hemisphere rays
        (scenes.ao_direction_sets(gi, gi_sets), uploaded once per (gi, gi_sets)) to their first hit within gi_radius (None:
        the whole grid), the hits are shaded under the light and, with gi_shadows, shadowed from the light camera's eye;
        gi_sum holds the bytes' sums, gi_filter (0: off) gathers them over the pixels of the same surface with
        gi_filter_cos and gi_filter_plane into gi_acc, and Kd * gi_gain of the mean is added to the image behind the
        frame's own shading and before ambient occlusion scales it.
        aa (one-stream renderer, the single-light plain frame: reflect=False, frame_cnt < 2, no setup.lights, area or gi;
        ao composes; 0: off): adaptive anti-aliasing -- the pixels on an edge (aa_edge: a silhouette, a material border, a
        crease sharper than aa_cos, a step off the neighbour's plane by more than aa_plane (None: 1 % of the scene's
        largest extent) or, with aa_shadows, a shadow edge) send aa = 1..32 sub-pixel eye rays
        (scenes.aa_offset_sets(aa, aa_sets), uploaded once per (aa, aa_sets)) through the uniform grid, each shaded as
        the frame shades a primary hit and, with shadows and aa_shadows, shadowed from the light camera's eye; aa_sum
        holds the bytes' sums and their mean replaces the pixel behind the frame's own shading and before ambient
        occlusion scales it.
        temporal (one-stream renderer, single-light frames, plain, reflect or refract; needs ao, area or gi; 0: off):
        consecutive display calls are the frames of a sequence -- frame f gives every effect that is on the f-th of 16
        rotated sample tables (scenes.temporal_sets of the 16-set table; uploaded once per key), the effect's gather (radius
        0 without *_filter) is blended into its running mean over at most temporal = 2..64 frames, fetched where the
        pixel's surface point lay under the previous frame's camera and dropped where the previous frame's normal
        (temporal_cos) or plane (temporal_plane; None: 1 % of the scene's largest extent) differ, and the effect is shaded
        from the mean (ao_tvis, area_tvis, gi_tacc; temporal_history).  A camera change does not reset the mean;
        temporal_reset lists what does.
        glossy (one-stream renderer, single-light frames with reflect=False; ao, area and gi compose; no aa, no temporal;
        0: off): rough mirrors -- every primary hit on a material with reflect > 0 sends glossy = 1..32 rays from
        reflect_rays' origin in a lobe around the mirror direction, tilted by the material's spread (Renderer(spread=))
        times the points of scenes.glossy_point_sets(glossy, glossy_sets) (uploaded once per (glossy, glossy_sets)) and
        mirrored back over the surface where they would enter it, to their first hit within glossy_radius (None: the whole
        grid); the hits are shaded under the light and, with glossy_shadows, shadowed from the light camera's eye;
        glossy_sum holds the bytes' sums, glossy_filter (0: off) gathers them over the lobe-carrying pixels of the same
        surface with glossy_filter_cos and glossy_filter_plane into glossy_acc, and the mean is blended into the image
        with the material's reflect directly behind the shading call, before the shadows darken it (DESIGN.md section
        6.13).
        smooth (one-stream renderer; the plain frame, frame_cnt=2, shadows=False and setup.lights; ao, area, gi and
        temporal compose; no reflect, refract, glossy, aa or reflect_lights; False: off): smooth shading -- the shading
        call reads, in the place of the triangles' own normals, the corner normals of the hit triangle mixed with the
        hit's barycentric coordinates (snormal).  A corner's normal is the normalised sum of the area-weighted normals of
        the faces around its vertex's key (Renderer(vertex_key=); scenes.weld) whose normal lies within smooth_cos, the
        cosine of the crease angle, of the corner's own face's (corner_normals).  The adjacency is built once per renderer
        and again after geometry_changed; the corner normals every frame, or with FLAG_STATIC_GEOMETRY when the geometry
        (rotate_bunny, geometry_changed) or smooth_cos changed.  smooth_signed keeps the normals' signs where the primary
        tracer folds them into the positive octant.  Nothing else reads snormal: normal, the {origin, normal} of ao_rays
        and every mask and sum are the frame's without smooth.
        textures (one-stream renderer; the plain frame, frame_cnt=2, shadows=False and setup.lights; smooth, ao, area and
        temporal compose; no reflect, refract, fresnel, glossy, gi, aa, dof or reflect_lights; False: off): texture
        mapping -- the shading call reads a per-pixel diffuse colour (albedo) in the place of the material's Kd: Kd times
        the material's texture (Renderer(textures=, mat_texture=, uvs=, uv_faces=)) filtered over the pixel's footprint from
        a mip atlas, with up to texture_aniso trilinear taps along the footprint's longer axis; texture_bias is added to
        every level.  The atlas is built by the first textured frame, once.  A renderer without textures gives the frame
        without the keyword, byte for byte.
        fresnel (one-stream renderer, single-light frames with reflect=True and refract=True, bounces <= 6; ao, area, gi
        and temporal compose as with the refract frame; no aa, glossy or smooth; False: off): Fresnel glass -- a glass hit
        sends the transmitted ray AND the reflected ray, weighted (1 - F) and F of the material's transmit, F = fresnel
        (True: 1.0; a number in (0, 1] scales it) times Schlick's share at the hit's angle; a pixel's rays form a tree
        of depth `bounces` that one fresnel_gather walks in the place of the level chain, with reflect_shadows shadowing
        every node from the light camera's eye; fresnel_cut (needs fresnel): children of a weight <= fresnel_cut are
        dropped; f_acc holds the trees' sums and shade_fresnel writes the bytes.
        dof (one-stream renderer, the single-light plain frame: frame_cnt < 2, no setup.lights, aa, reflect, refract,
        fresnel, glossy, gi, area, smooth or temporal; ao composes; 0: off): depth of field -- the camera is a thin lens
        of radius dof_aperture (world units) around the eye, perpendicular to the view, focused at the distance dof_focus
        along the view (None: the distance to the camera's look-at point).  A pixel is seen through the lens where its own
        circle of confusion, or that of a pixel at most dof_window = 0..8 pixels away which reaches it, is at least dof_min
        pixels wide (dof_flag); it sends dof = 1..32 rays (scenes.lens_sample_sets(dof, dof_sets), uploaded once per
        (dof, dof_sets)) from points of the lens through the uniform grid, each shaded as the frame shades a primary hit
        and, with shadows and dof_shadows, shadowed from the light camera's eye; dof_sum holds the bytes' sums and their
        mean replaces the pixel where aa_resolve stands in the order below.  dof_aperture=0 flags nothing (DESIGN.md
        section 6.17).
        The keywords that shape an effect need the effect: dof_* (need dof > 0), gi_sets and gi_filter (need gi > 0, like every other gi_*
        keyword), aa_sets (needs aa > 0, like every other aa_* keyword), glossy_sets and glossy_filter (need glossy > 0, like
        every other glossy_* keyword), temporal_cos and temporal_plane (need temporal > 0), smooth_cos and smooth_signed (need
        smooth=True).
        The passes over the image's bytes run in one order, whatever is on: the shading call;
        glossy_apply; shade_add_shadows, or with area shade_area / shade_area_vis in its place; gi_apply; aa_resolve;
        shade_ao / shade_ao_vis.  The primary hits' {origin, normal} (ao_rays / ao_active) are written once per frame, by
        the first of glossy, area, ao and gi that is on, and read by the others."""
        if textures is False and texture_aniso == 8 and texture_bias == 0:
            textures = None  # (the defaults: nothing to check, and the frame loop pays nothing for the keywords)
        else:
            textures = check_textures(textures, texture_aniso, texture_bias, reflect, refract, fresnel is not False, glossy, gi,
                                      aa, dof, frame_cnt, reflect_lights, self.aux is not None)
        if smooth is False and smooth_signed is False and smooth_cos == 0.5:
            smooth = None  # (the defaults: nothing to check, and the frame loop pays nothing for the keywords)
        else:
            smooth = check_smooth(smooth, smooth_cos, smooth_signed, reflect, refract, glossy, aa, reflect_lights,
                                  self.aux is not None)
        glossy = check_glossy(glossy, glossy_sets, glossy_filter, glossy_filter_cos, glossy_filter_plane, glossy_radius,
                              glossy_shadows, reflect, refract, aa, temporal, getattr(setup, "lights", None), reflect_lights,
                              self.aux is not None)
        aa = check_aa(aa, aa_sets, aa_cos, aa_plane, aa_shadows, reflect, frame_cnt, getattr(setup, "lights", None), area, gi,
                      reflect_lights, self.aux is not None)
        if dof != 0 or dof_aperture != 0.0 or dof_focus is not None or dof_sets != 1 or dof_min != 0.5 or dof_window != 4 \
                or dof_shadows is not True:
            dof = check_dof(dof, dof_aperture, dof_focus, dof_sets, dof_min, dof_window, dof_shadows, aa, reflect, refract,
                            fresnel is not False, glossy, gi, area, bool(smooth), temporal,
                            frame_cnt, getattr(setup, "lights", None), reflect_lights, self.aux is not None)
        else:
            dof = None  # (the defaults: nothing to check)
        gi = check_gi(gi, gi_radius, gi_gain, gi_shadows, gi_sets, gi_filter, gi_filter_cos, gi_filter_plane,
                      getattr(setup, "lights", None), reflect_lights, self.aux is not None)
        area, area_radius = check_area(area, area_radius, shadows, getattr(setup, "lights", None), self.aux is not None)
        area_sets, area_filter, area_filter_cos, area_filter_plane = check_area_filter(area, area_sets, area_filter,
                                                                                       area_filter_cos, area_filter_plane)
        self.refract = check_refract(refract, reflect)
        bounces = check_bounces(bounces)
        if fresnel is not False or fresnel_cut != 0.0:
            fresnel = check_fresnel(fresnel, fresnel_cut, reflect, refract, bounces, getattr(setup, "lights", None),
                                    reflect_lights, self.aux is not None)
        reflect_shadows = check_reflect_shadows(reflect_shadows, reflect)
        reflect_lights = check_reflect_lights(reflect_lights, reflect, getattr(setup, "lights", None))
        ao, ao_radius = check_ao(ao, ao_radius, self.aux is not None)
        ao_more = check_ao_filter(ao, ao_sets, ao_filter, ao_filter_cos, ao_filter_plane)
        temporal = check_temporal(temporal, temporal_cos, temporal_plane, bool(ao or area or gi), getattr(setup, "lights", None),
                                  reflect_lights, self.aux is not None)
        if not (temporal and shade):
            self._temporal_live = False  # the next temporal frame starts its means again
        if reflect_lights:
            lights = check_lights(setup.lights, reflect, self.aux is not None, True)
            return self._display_reflect_lights(setup, lights, shadows, shade, bounces, reflect_shadows,
                                                self._ao_stage(ao, ao_radius, shade, ao_more))
        if getattr(setup, "lights", None) is not None:
            lights = check_lights(setup.lights, reflect, self.aux is not None)
            return self._display_lights(setup, lights, shadows, shade, self._ao_stage(ao, ao_radius, shade, ao_more), smooth,
                                        textures)
        if temporal and shade:  # (the effects' stages are made behind _temporal_begin)
            ao_asked, gi_asked, ao = ao, gi, None
        else:
            ao = self._ao_stage(ao, ao_radius, shade, ao_more)
            if gi:
                gi = self._gi_stage(gi, shade)
        if aa:
            aa = self._aa_stage(aa, shade)
        if glossy:
            glossy = self._glossy_stage(glossy, shade)
        if fresnel and shade:
            self._ensure_fresnel_buffers()
        elif reflect and shade:
            self._ensure_reflect_buffers(bounces, reflect_shadows)
        if self.aux is not None and shade:
            two_streams = self._display_two_streams_inline if self._inline else self._display_overlapped
            return two_streams(setup, frame_cnt, shadows, reflect, bounces, reflect_shadows)
        ctx = self.ctx
        cam = make_camera(setup.camera, setup.fovy, self.aspect)
        if dof:
            dof = self._dof_stage(dof, shade, cam)
        tp = area_t = None
        if temporal and shade:
            tp = self._temporal_begin(temporal, cam)
            ao = self._temporal_ao(tp, ao_asked, ao_radius, ao_more) if ao_asked else None
            gi = self._temporal_gi(tp, gi_asked, setup) if gi_asked else None
            if area:
                area_t = self._temporal_area(tp, area, area_sets, area_radius, area_filter, area_filter_cos,
                                             area_filter_plane, setup)
        camera_pass(ctx, self, self, setup, cam)
        albedo = None
        if textures and shade:  # (here: the context's camera is the eye's until the light's is uploaded)
            self._texture_stage()
            albedo = texture_pass(ctx, self, self.cam_pos, textures)
        lcam = make_camera(setup.light_camera, setup.fovy, self.aspect)
        use_light_camera(ctx, lcam)
        if shadows and not area:
            map_rays(ctx, self, self)
            build_grid(ctx, self, GRID_SPHERICAL, self.shards)
            light_grid = ctx.grid_ptrs(GRID_SPHERICAL)
            sort_rays(ctx, self)
            trace_shadows(ctx, self, self, light_grid)
        if not shade:
            return
        if aa:
            aa_edges(ctx, self, self.cam_pos, aa, shadows and aa[5])
        if dof:
            dof_pixels(ctx, self, dof)
        if reflect:
            reflect_rays(ctx, self, self.cam_pos)
            build_grid(ctx, self, GRID_UNIFORM, self.shards)
            if fresnel:
                fresnel_pass(ctx, self, self.cam_pos, bounces, fresnel, lcam.worldori[:3] if reflect_shadows else None)
            else:
                trace_reflections(ctx, self, bounces, lcam.worldori[:3] if reflect_shadows else None)
        elif glossy:
            # (reflect_rays although reflect=False: the lobe's origins and mirror directions are level 1's rays)
            ctx.reflect_rays(self.cam_pos, self.t, self.dir, self.intersect_id, self.d_matidx, self.d_reflect, self.num_materials,
                             self.d_verts, self.d_faces, self.reflect_eps, self.rays, self.active)
            build_grid(ctx, self, GRID_UNIFORM, self.shards)
            glossy_pass(ctx, self, self.cam_pos, glossy, lcam.worldori[:3] if glossy[5] else None)
        elif ao or area or gi or aa or dof:
            build_grid(ctx, self, GRID_UNIFORM, self.shards)
        have_rays = bool(glossy)  # (glossy_pass wrote ao_rays / ao_active)
        if area:
            thru = see_through(self)
            if tp:
                area_pass(ctx, self, self.cam_pos, area_t[1], thru, (area,) + area_t[2])
            elif area_sets > 1:
                area_pass(ctx, self, self.cam_pos, self._area_sets_stage(area, area_sets, area_radius, setup), thru,
                          (area,) + AREA_SET_TILES[area_sets], have_rays=have_rays)
            else:
                area_pass(ctx, self, self.cam_pos, self._area_stage(area, area_radius, setup), thru, have_rays=have_rays)
        if ao:
            ao_pass(ctx, self, self.cam_pos, *ao[:3], have_rays=have_rays or bool(area))  # (area_pass wrote them as well)
        if gi:
            gi_pass(ctx, self, self.cam_pos, gi, lcam.worldori[:3] if gi[6] else None, bool(ao or area or glossy))
        if aa:
            aa_pass(ctx, self, cam.camcoords, aa, lcam.worldori[:3] if shadows and aa[5] else None)
        if dof:
            dof_pass(ctx, self, cam.camcoords, dof, lcam.worldori[:3] if shadows and dof[7] else None)
        normal = None
        if smooth:
            self._smooth_stage(smooth[0])
            normal = smooth_pass(ctx, self, self.cam_pos, smooth[1])
        shade_frame(ctx, self, self.cam_pos, frame_cnt, shadows and not area, reflect, bounces, reflect_shadows,
                    glossy or None, normal, fresnel or None, albedo)
        if area and tp:
            area_shade_temporal(ctx, self, tp, area_t)
        elif area and area_filter:
            self._ensure_area_filter_buffers()
            plane = default_filter_plane(self.bbmin, self.bbmax) if area_filter_plane is None else area_filter_plane
            ctx.filter_visibility(self.area_mask, area, self.ao_rays, self.ao_active, area_filter, area_filter_cos, plane,
                                  self.area_vis)
            ctx.shade_area_vis(self.image, self.area_vis, area)
        elif area:
            ctx.shade_area(self.image, self.area_mask, area)
        if gi and tp:
            gi_shade_temporal(ctx, self, tp, gi)
        elif gi:
            gi_shade(ctx, self, gi)
        if aa:
            ctx.aa_resolve(self.image, self.aa_sum, aa[0])
        if dof:
            ctx.aa_resolve(self.image, self.dof_sum, dof[0])
        if ao and tp:
            ao_shade_temporal(ctx, self, tp, ao)
        elif ao:
            ao_shade(ctx, self, *ao)

    # -- texture mapping
    def _texture_stage(self):
        """What texture_pass reads: the atlas, the uvs, the uv indices and the materials' textures on the device and albedo
        [3 W*H], made on the first textured frame and kept -- the uvs ride on the face list, so rotate_bunny and
        geometry_changed invalidate nothing here."""
        if self._tex is None:
            ctx, t = self.ctx, self.torch
            uv, uf, tl, mt = self._tex_host
            ctx.texture_set(tl)
            self._tex = {"uvs": ctx.upload(uv.reshape(-1)) if len(uv) else None, "num_uvs": len(uv),
                         "uv_faces": ctx.upload(uf.reshape(-1)), "mat_texture": ctx.upload(mt), "mat_texture_host": mt}
            self.albedo = ctx.empty(3 * self.N, t.float32)

    # -- smooth shading
    def _smooth_stage(self, cos):
        """What smooth_pass reads, in place: snormal [3 W*H] and corner_normals [9 F], allocated on first use; the
        context's adjacency, built once and again after geometry_changed; the corner normals, formed every frame -- with
        FLAG_STATIC_GEOMETRY only when the geometry (rotate_bunny, geometry_changed) or cos is not what they were formed
        of."""
        ctx, t = self.ctx, self.torch
        st = getattr(self, "_smooth", None)
        if st is None:
            if not self._smooth_faces_ok:
                raise ValueError("smooth needs every index of the face list in 0..V-1")
            st = self._smooth = {"adjacency": False, "normals": None,
                                 "key": None if self._vertex_key is None else ctx.upload(self._vertex_key)}
            self.snormal = ctx.empty(3 * self.N, t.float32)
            self.corner_normals = ctx.empty(9 * self.F, t.float32)
        if not st["adjacency"]:
            ctx.smooth_adjacency(self.d_faces, self.F, self.d_verts.numel() // 3, st["key"])
            st["adjacency"], st["normals"] = True, None
        static = bool(int(ctx.cfg.flags) & FLAG_STATIC_GEOMETRY)
        if not static or st["normals"] != (cos,):
            ctx.smooth_corner_normals(self.d_faces, self.d_verts, self.F, cos, self.corner_normals)
            st["normals"] = (cos,)

    # -- temporal accumulation
    def _temporal_begin(self, temporal, cam):
        """Starts a temporal frame: the G-buffer of the frame before becomes prev_ao_rays / prev_ao_active (the buffers
        change places: ao_rays keeps naming the frame that is being rendered), and every mean starts again when the frame
        before was not a temporal one.  Returns the frame's record: the most frames of a mean, the surface tests' bounds,
        the eye's block of the frame before (this frame's own where there is none: the histories are empty then) and the
        bounds as part of the effects' keys."""
        N, cos, plane = temporal
        plane = default_filter_plane(self.bbmin, self.bbmax) if plane is None else plane
        self._ensure_temporal_gbuffers()
        if not self._temporal_live:
            self.temporal_reset()
            self._temporal_prev_cam = None
            self._temporal_live = True
        self._temporal_serial += 1
        self.ao_rays, self.prev_ao_rays = self.prev_ao_rays, self.ao_rays
        self.ao_active, self.prev_ao_active = self.prev_ao_active, self.ao_active
        now = np.array(cam.camcoords, np.float32)
        prev, self._temporal_prev_cam = self._temporal_prev_cam, now
        return {"max": N, "cos": cos, "plane": plane, "prev_cam": now if prev is None else prev, "key": (N, cos, plane)}

    def _ensure_temporal_gbuffers(self):
        """ao_rays / ao_active and their twins of the frame before, allocated on first use (the twins zeroed: nothing
        reads them before a frame has written them, the empty histories stand in front)."""
        t, N, dev = self.torch, self.N, self.image.device
        if self.ao_rays is None:
            self.ao_rays = t.empty(6 * N, dtype=t.float32, device=dev)
            self.ao_active = t.empty(N, dtype=t.int32, device=dev)
        if self.prev_ao_rays is None:
            self.prev_ao_rays = t.zeros(6 * N, dtype=t.float32, device=dev)
            self.prev_ao_active = t.zeros(N, dtype=t.int32, device=dev)

    def _temporal_words(self, name, words):
        """The temporal call's output of an effect, [words W*H] uint32 words in an int32 tensor, allocated on first use."""
        if getattr(self, name) is None:
            setattr(self, name, self.torch.zeros(words * self.N, dtype=self.torch.int32, device=self.image.device))

    def _temporal_alloc(self, words):
        t = self.torch
        return [t.zeros(words * self.N, dtype=t.float32, device=self.image.device) for _ in range(2)]

    def _temporal_effect(self, name, key, words):
        """The state of effect `name` for this frame: made on first use, cleared when its parameters `key` are not those
        it was accumulated under or when it did not run in the temporal frame before."""
        st = self._temporal.get(name)
        if st is None:
            st = self._temporal[name] = {"key": key, "hist": self._temporal_alloc(words), "turn": 0, "n": 0}
        elif st["key"] != key or st["serial"] != self._temporal_serial - 1:
            self._temporal_clear(st)
            st["key"] = key
        st["serial"] = self._temporal_serial
        return st

    def _temporal_table(self, key, sets, frame, table16):
        """Frame `frame`'s device table of the 16-set table table16(): the 16 rotated tables (scenes.temporal_sets) are
        uploaded once per key and kept."""
        if key not in self._temporal_set_tables:
            from .scenes import temporal_sets

            whole = table16()
            self._temporal_set_tables[key] = [self._upload_ao_sets(temporal_sets(whole, sets, f)) for f in range(16)]
        return self._temporal_set_tables[key][frame % 16]

    def _temporal_ao(self, tp, ao, ao_radius, sets):
        """_ao_stage for a temporal frame: (directions, radius, (frame table, (set_w, set_h), gather), state) with the
        walk over sets and the gather always there (a 1 x 1 tile with ao_sets = 1, radius 0 without ao_filter)."""
        from .scenes import ao_direction_sets

        ao_sets, ao_filter, cos, plane = sets
        dirs = self._ensure_ao_buffers(ao)
        self._ensure_ao_filter_buffers()
        self._temporal_words("ao_tvis", 2)
        cos = 0.9 if cos is None else cos
        plane = default_filter_plane(self.bbmin, self.bbmax) if plane is None else plane
        st = self._temporal_effect("ao", (ao, ao_radius, ao_sets, ao_filter, cos, plane) + tp["key"], 2)
        table = self._temporal_table(("ao", ao, ao_sets), ao_sets, st["n"], lambda: ao_direction_sets(ao, 16))
        return (dirs, ao_radius, (table, AREA_SET_TILES[ao_sets], (ao_filter, cos, plane)), st)

    def _temporal_gi(self, tp, gi, setup):
        """_gi_stage for a temporal frame: its tuple with the frame's table, the gather always there, and the state behind
        it.  The light the hits are shaded and shadowed under is part of the key."""
        from .scenes import ao_direction_sets

        S, radius, gain, shadows, sets, filt, cos, plane = gi
        self._ensure_gi_buffers(True)
        self._temporal_words("gi_tacc", 4)
        cos = 0.9 if cos is None else cos
        plane = default_filter_plane(self.bbmin, self.bbmax) if plane is None else plane
        light = tuple(map(float, setup.shading_light)) + tuple(map(float, setup.light_camera["eye"]))
        st = self._temporal_effect("gi", (S, radius, gain, shadows, sets, filt, cos, plane, light) + tp["key"], 4)
        table = self._temporal_table(("gi", S, sets), sets, st["n"], lambda: ao_direction_sets(S, 16))
        return (S, AREA_SET_TILES[sets], table, radius, gain, (filt, cos, plane), shadows, st)

    def _temporal_area(self, tp, area, area_sets, area_radius, area_filter, cos, plane, setup):
        """(S, frame table, (set_w, set_h), gather, state) of an area light in a temporal frame: _area_sets_stage's disk,
        16 sets of it.  The light is part of the key."""
        from .scenes import area_sample_sets

        self._ensure_area_buffers()
        self._ensure_area_filter_buffers()
        self._temporal_words("area_tvis", 2)
        cos = 0.9 if cos is None else cos
        plane = default_filter_plane(self.bbmin, self.bbmax) if plane is None else plane
        eye, look = tuple(map(float, setup.light_camera["eye"])), tuple(map(float, setup.light_camera["look"]))
        st = self._temporal_effect("area", (area, area_sets, area_radius, area_filter, cos, plane, eye, look) + tp["key"], 2)
        table = self._temporal_table(("area", area, area_sets, area_radius, eye, look), area_sets, st["n"],
                                     lambda: area_sample_sets(area, 16, np.float64(eye), np.float64(look) - np.float64(eye),
                                                              area_radius))
        return (area, table, AREA_SET_TILES[area_sets], (area_filter, cos, plane), st)

    def _aa_stage(self, aa, shade):
        """(S, (set_w, set_h), table, cos, plane, shadows) for aa_edges and aa_pass from what check_aa returned, with the
        buffers aa_edge [W*H] and aa_sum [4 W*H] (uint32 words in an int32 tensor) in place; None: nothing is shaded.
        table: scenes.aa_offset_sets(S, aa_sets) on the device, uploaded once per (S, aa_sets) and kept."""
        if not shade:
            return None
        S, sets, cos, plane, shadows = aa
        self._ensure_aa_buffers()
        tables = self._aa_set_tables
        if (S, sets) not in tables:
            from .scenes import aa_offset_sets

            tables[(S, sets)] = self._upload_ao_sets(aa_offset_sets(S, sets))
        return (S, AREA_SET_TILES[sets], tables[(S, sets)], cos, default_filter_plane(self.bbmin, self.bbmax) if plane is None else plane,
                shadows)

    def _dof_stage(self, dof, shade, cam):
        """(S, (set_w, set_h), table, lens, coc_scale, min, window, shadows) for dof_pixels and dof_pass from what check_dof
        returned and the frame's camera (Camera.lens: U, V, A, F and the circle's scale in pixels), with the buffers
        dof_flag [W*H] and dof_sum [4 W*H] (uint32 words in an int32 tensor) in place; None: nothing is shaded.  table:
        scenes.lens_sample_sets(S, dof_sets) on the device, uploaded once per (S, dof_sets) and kept."""
        if not shade:
            return None
        S, sets, aperture, focus, cmin, window, shadows = dof
        self._ensure_dof_buffers()
        tables = self._dof_set_tables
        if (S, sets) not in tables:
            from .scenes import lens_sample_sets

            tables[(S, sets)] = self._upload_ao_sets(lens_sample_sets(S, sets))
        lens, coc_scale = cam.lens(aperture, focus, self.ctx.height)
        return (S, AREA_SET_TILES[sets], tables[(S, sets)], lens, coc_scale, cmin, window, shadows)

    def _ensure_dof_buffers(self):
        """dof_flag [W*H] and dof_sum [4 W*H] (uint32 words in an int32 tensor), allocated on first use."""
        t, N, dev = self.torch, self.N, self.image.device
        if self.dof_flag is None:
            self.dof_flag = t.zeros(N, dtype=t.int32, device=dev)
            self.dof_sum = t.zeros(4 * N, dtype=t.int32, device=dev)

    def _ensure_aa_buffers(self):
        """aa_edge [W*H] and aa_sum [4 W*H] (uint32 words in an int32 tensor), allocated on first use."""
        t, N, dev = self.torch, self.N, self.image.device
        if self.aa_edge is None:
            self.aa_edge = t.zeros(N, dtype=t.int32, device=dev)
            self.aa_sum = t.zeros(4 * N, dtype=t.int32, device=dev)

    def _gi_stage(self, gi, shade):
        """(S, (set_w, set_h), table, radius, gain, gather, shadows) for gi_pass and gi_shade from what check_gi returned,
        with the buffers in place; None: nothing is shaded.  table: scenes.ao_direction_sets(S, gi_sets) on the device,
        uploaded once per (S, gi_sets) and kept; gather: (radius, cos, plane), or None without one."""
        if not shade:
            return None
        S, radius, gain, shadows, sets, filt, cos, plane = gi
        self._ensure_gi_buffers(bool(filt))
        tables = self._gi_set_tables
        if (S, sets) not in tables:
            from .scenes import ao_direction_sets

            tables[(S, sets)] = self._upload_ao_sets(ao_direction_sets(S, sets))
        gather = None
        if filt:
            gather = (filt, cos, default_filter_plane(self.bbmin, self.bbmax) if plane is None else plane)
        return (S, AREA_SET_TILES[sets], tables[(S, sets)], radius, gain, gather, shadows)

    def _glossy_stage(self, glossy, shade):
        """(S, (set_w, set_h), table, radius, gather, shadows) for glossy_pass and glossy_shade from what check_glossy
        returned, with the buffers in place; None: nothing is shaded.  table: scenes.glossy_point_sets(S, glossy_sets) on
        the device, uploaded once per (S, glossy_sets) and kept; gather: (radius, cos, plane), or None without one."""
        if not shade:
            return None
        S, radius, shadows, sets, filt, cos, plane = glossy
        self._ensure_glossy_buffers(bool(filt))
        tables = self._glossy_tables
        if (S, sets) not in tables:
            from .scenes import glossy_point_sets

            tables[(S, sets)] = self._upload_glossy_points(glossy_point_sets(S, sets))
        gather = None
        if filt:
            gather = (filt, cos, default_filter_plane(self.bbmin, self.bbmax) if plane is None else plane)
        return (S, AREA_SET_TILES[sets], tables[(S, sets)], radius, gather, shadows)

    def _upload_glossy_points(self, table):
        return self.ctx.upload(table.reshape(-1))

    def _ensure_glossy_buffers(self, gather):
        """glossy_sum [4 W*H] and, with a gather, glossy_acc [4 W*H] (uint32 words in int32 tensors), level 1's rays and
        the normals' buffers ao_rays / ao_active, allocated on first use."""
        t, N, dev = self.torch, self.N, self.image.device
        self._ensure_reflect_buffers(1, False)
        if self.ao_rays is None:
            self.ao_rays = t.empty(6 * N, dtype=t.float32, device=dev)
            self.ao_active = t.empty(N, dtype=t.int32, device=dev)
        if self.glossy_sum is None:
            self.glossy_sum = t.zeros(4 * N, dtype=t.int32, device=dev)
        if gather and self.glossy_acc is None:
            self.glossy_acc = t.zeros(4 * N, dtype=t.int32, device=dev)

    def _ensure_gi_buffers(self, gather):
        """gi_sum [4 W*H] and, with a gather, gi_acc [4 W*H] (uint32 words in int32 tensors), and the origins' buffers
        ao_rays / ao_active, allocated on first use."""
        t, N, dev = self.torch, self.N, self.image.device
        if self.ao_rays is None:
            self.ao_rays = t.empty(6 * N, dtype=t.float32, device=dev)
            self.ao_active = t.empty(N, dtype=t.int32, device=dev)
        if self.gi_sum is None:
            self.gi_sum = t.zeros(4 * N, dtype=t.int32, device=dev)
        if gather and self.gi_acc is None:
            self.gi_acc = t.zeros(4 * N, dtype=t.int32, device=dev)

    def _ao_stage(self, ao, ao_radius, shade, sets=(1, 0, None, None)):
        """(directions, radius) for ao_pass and ao_shade, with the buffers in place; None: the frame has no ambient
        occlusion (ao == 0, or nothing is shaded).  sets (what check_ao_filter returned) away from the defaults: a third
        entry (table, (set_w, set_h), gather) -- the device table of scenes.ao_direction_sets, uploaded once per
        (ao, ao_sets) and kept, or None with ao_sets = 1; the gather's (radius, cos, plane), with ao_vis in place, or None
        without one."""
        if not (ao and shade):
            return None
        ao_sets, ao_filter, ao_filter_cos, ao_filter_plane = sets
        stage = (self._ensure_ao_buffers(ao), ao_radius)
        if ao_sets == 1 and not ao_filter:
            return stage
        table = gather = None
        if ao_sets > 1:
            if (ao, ao_sets) not in self._ao_set_tables:
                from .scenes import ao_direction_sets

                self._ao_set_tables[(ao, ao_sets)] = self._upload_ao_sets(ao_direction_sets(ao, ao_sets))
            table = self._ao_set_tables[(ao, ao_sets)]
        if ao_filter:
            self._ensure_ao_filter_buffers()
            plane = default_filter_plane(self.bbmin, self.bbmax) if ao_filter_plane is None else ao_filter_plane
            gather = (ao_filter, ao_filter_cos, plane)
        return stage + ((table, AREA_SET_TILES[ao_sets], gather),)

    def _upload_ao_sets(self, table):
        return self.ctx.upload(table.reshape(-1))

    def _ensure_ao_filter_buffers(self):
        """ao_vis [2 W*H] (uint32 words in an int32 tensor), allocated on first use."""
        if self.ao_vis is None:
            self.ao_vis = self.torch.zeros(2 * self.N, dtype=self.torch.int32, device=self.image.device)

    def _area_stage(self, area, area_radius, setup):
        """The sample points for area_pass, with the buffers in place: the disk of area_radius around the light camera's
        eye (the point the hard shadows are cast from), perpendicular to its look - eye."""
        from .scenes import area_samples

        self._ensure_area_buffers()
        eye = np.asarray(setup.light_camera["eye"], np.float64)
        return area_samples(area, eye, np.asarray(setup.light_camera["look"], np.float64) - eye, area_radius)

    def _area_sets_stage(self, area, area_sets, area_radius, setup):
        """The device table of sample sets for area_pass, with the buffers in place: scenes.area_sample_sets of
        _area_stage's disk, uploaded once per (area, area_sets, area_radius, light) and kept."""
        from .scenes import area_sample_sets

        self._ensure_area_buffers()
        eye, look = tuple(map(float, setup.light_camera["eye"])), tuple(map(float, setup.light_camera["look"]))
        key = (area, area_sets, area_radius, eye, look)
        if key not in self._area_set_tables:
            table = area_sample_sets(area, area_sets, np.float64(eye), np.float64(look) - np.float64(eye), area_radius)
            self._area_set_tables[key] = self._upload_area_sets(table)
        return self._area_set_tables[key]

    def _upload_area_sets(self, table):
        return self.ctx.upload(table.reshape(-1))

    def _display_lights(self, setup, lights, shadows, shade, ao=None, smooth=None, textures=None):
        """The reference's loop over the lights (main.cu:148-203) made real: the camera pass, per light its camera and
        shadow stage into its row of shadowed_lights, then ONE shading pass.  dd_camcoords is the last light's when
        the shading runs, as the reference's loop leaves it."""
        ctx = self.ctx
        if shadows:
            self._ensure_light_buffers(len(lights))
        camera_pass(ctx, self, self, setup, make_camera(setup.camera, setup.fovy, self.aspect))
        albedo = None
        if textures and shade:  # (here: the context's camera is the eye's until the first light's is uploaded)
            self._texture_stage()
            albedo = texture_pass(ctx, self, self.cam_pos, textures)
        if shadows:
            self.shadowed_lights[:len(lights)].zero_()  # the shadow pass only sets flags: rows of earlier frames are stale
        for l, (params, _) in enumerate(lights):
            use_light_camera(ctx, make_camera(params, setup.fovy, self.aspect))
            if shadows:
                map_rays(ctx, self, self)
                build_grid(ctx, self, GRID_SPHERICAL, self.shards)
                light_grid = ctx.grid_ptrs(GRID_SPHERICAL)
                sort_rays(ctx, self)
                trace_shadows(ctx, self, self, light_grid, self.shadowed_lights[l])
        if not shade:
            return
        if ao:
            build_grid(ctx, self, GRID_UNIFORM, self.shards)
            ao_pass(ctx, self, self.cam_pos, *ao)
        normal = None
        if smooth:
            self._smooth_stage(smooth[0])
            normal = smooth_pass(ctx, self, self.cam_pos, smooth[1])
        shade_lights(ctx, self, self.cam_pos, lights, shadows, normal, albedo)
        if ao:
            ao_shade(ctx, self, *ao)

    def _display_reflect_lights(self, setup, lights, shadows, shade, bounces, reflect_shadows, ao=None):
        """_display_lights' camera pass and per-light shadow stages, then the reflection levels once (the uniform grid and
        the reflected rays do not know the light) with every level's hits tested against the eyes of all light cameras in
        one launch, then ONE shading pass.  No host wait is added."""
        ctx = self.ctx
        if shadows:
            self._ensure_light_buffers(len(lights))
        if shade:
            self._ensure_reflect_lights_buffers(bounces, len(lights), reflect_shadows)
        camera_pass(ctx, self, self, setup, make_camera(setup.camera, setup.fovy, self.aspect))
        if shadows:
            self.shadowed_lights[:len(lights)].zero_()  # the shadow pass only sets flags: rows of earlier frames are stale
        eyes = []
        for l, (params, _) in enumerate(lights):
            lcam = make_camera(params, setup.fovy, self.aspect)
            eyes.append(tuple(float(x) for x in lcam.worldori[:3]))
            use_light_camera(ctx, lcam)
            if shadows:
                map_rays(ctx, self, self)
                build_grid(ctx, self, GRID_SPHERICAL, self.shards)
                light_grid = ctx.grid_ptrs(GRID_SPHERICAL)
                sort_rays(ctx, self)
                trace_shadows(ctx, self, self, light_grid, self.shadowed_lights[l])
        if not shade:
            return
        reflect_rays(ctx, self, self.cam_pos)
        build_grid(ctx, self, GRID_UNIFORM, self.shards)
        trace_reflections(ctx, self, bounces, shadow_lights=eyes if reflect_shadows else None)
        if ao:
            ao_pass(ctx, self, self.cam_pos, *ao)
        shade_reflect_lights(ctx, self, self.cam_pos, lights, bounces, shadows, reflect_shadows)
        if ao:
            ao_shade(ctx, self, *ao)

    def _display_overlapped(self, setup, frame_cnt, shadows, reflect, bounces, reflect_shadows=False):
        """display() on two streams.  Side stream (second context, driven by the helper thread): light grid,
        uniform grid, then - once the primary hits exist - secondary rays and the 3D-DDA.  Main stream: screen
        grid, primary rays, ray mapping and sort, shadow rays (after the light grid), shading (after the DDA).
        The shadow pass and the bounce only depend on the primary hits, not on each other."""
        import threading

        ctx, aux, t = self.ctx, self.aux, self.ctx.torch
        main, side = self.main_stream, self.aux_stream
        lcam = make_camera(setup.light_camera, setup.fovy, self.aspect)
        ev_primary, ev_light_grid = t.cuda.Event(), t.cuda.Event()
        primary_recorded, light_grid_recorded = threading.Event(), threading.Event()
        # side stream: starts once the geometry of this frame is final on the main stream
        side.wait_stream(main)

        status = {"primary_failed": False, "light_grid_failed": False}

        def side_job():
            try:
                if shadows:
                    use_light_camera(aux, lcam)
                    build_grid(aux, self, GRID_SPHERICAL)
                    ev_light_grid.record(side)
            except BaseException:
                status["light_grid_failed"] = True  # the main thread must not wait for an event never recorded
                raise
            finally:
                light_grid_recorded.set()
            if reflect:
                build_grid(aux, self, GRID_UNIFORM)
                primary_recorded.wait()
                if status["primary_failed"]:
                    return
                side.wait_event(ev_primary)
                reflect_rays(aux, self, self.cam_pos)
                trace_reflections(aux, self, bounces, lcam.worldori[:3] if reflect_shadows else None)

        self._jobs.put(side_job)
        failed = None
        try:
            try:
                camera_pass(ctx, self, self, setup, make_camera(setup.camera, setup.fovy, self.aspect))
                ev_primary.record(main)
            except BaseException as e:
                status["primary_failed"] = True  # the side job skips what depends on the primary hits
                raise e
            finally:
                primary_recorded.set()
            use_light_camera(ctx, lcam)
            if shadows:
                map_rays(ctx, self, self)
                sort_rays(ctx, self)
                light_grid_recorded.wait()
                if status["light_grid_failed"]:
                    raise RuntimeError("the light grid build on the side stream failed")
                main.wait_event(ev_light_grid)
                trace_shadows(ctx, self, self, aux.grid_ptrs(GRID_SPHERICAL))
        except BaseException as e:
            failed = e
        finally:
            # exactly one result per submitted job is consumed, whatever happened above: a result left in the
            # queue would make the NEXT frame join the side stream before its own work was enqueued
            err = self._done.get()
        main.wait_stream(side)
        if failed is not None:
            raise failed
        if err is not None:
            raise err
        shade_frame(ctx, self, self.cam_pos, frame_cnt, shadows, reflect, bounces, reflect_shadows)

    def _display_two_streams_inline(self, setup, frame_cnt, shadows, reflect, bounces, reflect_shadows=False):
        """The two-stream frame from ONE host thread: with option async_build no call waits for the device, so the
        side stream's work is simply enqueued first (light grid, uniform grid), then the camera pass on the main
        stream, then what depends on the primary hits on either stream; events join them as in _display_overlapped."""
        ctx, aux, t = self.ctx, self.aux, self.ctx.torch
        main, side = self.main_stream, self.aux_stream
        lcam = make_camera(setup.light_camera, setup.fovy, self.aspect)
        ev_primary, ev_light_grid = t.cuda.Event(), t.cuda.Event()
        side.wait_stream(main)  # the geometry of this frame is final on the main stream
        # the light grid and the uniform grid depend on the geometry only: their reference lists are sorted in shared
        # launches (one histogram kernel and one kernel per pass level for both: ugrt_grid_build_batch_begin / _end)
        batch = shadows and reflect and self.batch_builds
        if batch:
            aux.grid_build_batch_begin()
        try:
            if shadows:
                use_light_camera(aux, lcam)
                build_grid(aux, self, GRID_SPHERICAL)
                if not batch:
                    ev_light_grid.record(side)
            if reflect:
                build_grid(aux, self, GRID_UNIFORM)
        except BaseException:
            if batch:  # an open batch would refuse every later frame's; the build's own failure is the one raised
                with contextlib.suppress(Exception):
                    aux.grid_build_batch_end()
            raise
        if batch:
            aux.grid_build_batch_end()
            ev_light_grid.record(side)
        camera_pass(ctx, self, self, setup, make_camera(setup.camera, setup.fovy, self.aspect))
        ev_primary.record(main)
        if reflect:
            side.wait_event(ev_primary)
            reflect_rays(aux, self, self.cam_pos)
            trace_reflections(aux, self, bounces, lcam.worldori[:3] if reflect_shadows else None)
        use_light_camera(ctx, lcam)
        if shadows:
            map_rays(ctx, self, self)
            sort_rays(ctx, self)
            main.wait_event(ev_light_grid)
            trace_shadows(ctx, self, self, aux.grid_ptrs(GRID_SPHERICAL))
        main.wait_stream(side)
        shade_frame(ctx, self, self.cam_pos, frame_cnt, shadows, reflect, bounces, reflect_shadows)

    def synchronize(self):
        """Both contexts are synchronised before anything is raised: an overflow reported by one must not leave the
        other's report pending (it would be raised again after the frames had been repeated)."""
        err = None
        for c in (self.ctx, self.aux):
            if c is None:
                continue
            try:
                c.synchronize()
            except Exception as e:  # UGRT_EOVERFLOW of either context: one report for the pair
                err = err or e
        if err is not None:
            raise err

    def band_image(self):
        """uint8 view [rows*8, W, 3] of this context's band."""
        ctx = self.ctx
        return self.image[3 * ctx.p0:3 * (ctx.p0 + ctx.npix)].view(-1, ctx.width, 3)


class BandedRenderer(_Frame):
    """ONE frame at a time, cut into bands of tile rows that run on HIP streams of their own (SURVEY 8(e)'s sharding,
    applied to the streams of one GPU instead of to GPUs).

    A frame alone cannot fill the chip: its main stream is a chain of ~45 dependent launches, most of them short and
    latency-bound (the sorts' passes, scans, run and item kernels), and only the three tracers are wide.  With B band
    contexts the chains of the bands run beside each other; the light grid, the uniform grid and the bounce stay whole
    on ONE side context (they depend on the geometry, not on the band).  Every band context writes its rows of the SAME
    per-pixel arrays (pixel ids are global: a band context writes its band), so the frame's buffers are those of a
    single-context frame, bit for bit (tests/test_gpu_parity.py::test_banded_frame_equals_the_single_context_frame).

        side:    light grid, uniform grid .................. (all primaries) secondary rays, 3D-DDA
        band i:  screen grid (rows of the band), primary ... ray map + sort, (grids) shadow pass, (DDA) shading

    No call waits for the device (option async_build on every context); one host thread enqueues the stages band by
    band."""

    def __init__(self, Context, W, H, verts, faces, matidx, mat_list, reflect=None, transmit=None, ior=None, bands=2, device=0,
                 light_grid=(128, 128), uniform_dims=(128, 128, 64), flags=0):
        from . import parallel

        assert bands >= 1
        self.bands = bands
        nby = H // 8
        import torch as t

        dev = t.device("cuda", device)
        self.main_stream = t.cuda.current_stream(dev)
        self.side_stream = t.cuda.Stream(dev)
        with t.cuda.stream(self.side_stream):
            self.aux = Context(W, H, device=device, light_grid=light_grid, flags=flags, uniform_dims=uniform_dims)
        self.streams, self._per_band = [], []
        bounds = parallel.equal_bounds(bands, nby)
        for b in range(bands):
            st = self.main_stream if b == 0 else t.cuda.Stream(self.aux.device)
            with t.cuda.stream(st):
                cx = Context(W, H, device=device, light_grid=light_grid, rows=(bounds[b], bounds[b + 1]), flags=flags,
                             uniform_dims=uniform_dims)
                self._per_band.append(_Band(cx))
            self.streams.append(st)
        # the scene and the frame's arrays once, on the main stream (band 0's)
        _Frame.__init__(self, self._per_band[0].ctx, verts, faces, matidx, mat_list, reflect, 1e-3, transmit, ior)
        for c in self.contexts():
            c.set_option("async_build", 1)
        # (as in the two-stream frame: the bounce's persistent waves leave room for the bands' short kernels)
        self.aux.set_option("dda_blocks", 1024)

    def contexts(self):
        return [self.aux] + [b.ctx for b in self._per_band]

    def display(self, setup, frame_cnt=1, shadows=True, reflect=True, bounces=1, reflect_shadows=False, ao=0,
                ao_radius=None, refract=False, area=0, area_radius=None, area_sets=1, area_filter=0, area_filter_cos=0.9,
                area_filter_plane=None, ao_sets=1, ao_filter=0, ao_filter_cos=0.9, ao_filter_plane=None, gi=0, gi_radius=None,
                gi_gain=1.0, gi_shadows=True, gi_sets=1, gi_filter=0, gi_filter_cos=0.9, gi_filter_plane=None, aa=0, aa_sets=1,
                aa_cos=0.9, aa_plane=None, aa_shadows=True, temporal=0, temporal_cos=0.9, temporal_plane=None, glossy=0,
                glossy_sets=1, glossy_filter=0, glossy_filter_cos=0.9, glossy_filter_plane=None, glossy_radius=None,
                glossy_shadows=True, smooth=False, smooth_cos=0.5, smooth_signed=False, dof=0, dof_aperture=0.0, dof_focus=None,
                dof_sets=1, dof_min=0.5, dof_window=4, dof_shadows=True, textures=False, texture_aniso=8,
                texture_bias=0, fresnel=False, fresnel_cut=0.0):
        if textures is not False or texture_aniso != 8 or texture_bias != 0:
            check_textures(textures, texture_aniso, texture_bias, two_streams=True)  # raises with textures=True
        check_dof(dof, dof_aperture, dof_focus, dof_sets, dof_min, dof_window, dof_shadows, two_streams=True)  # raises with dof > 0
        check_smooth(smooth, smooth_cos, smooth_signed, False, False, 0, 0, False, True)  # raises with smooth=True
        check_fresnel(fresnel, fresnel_cut, reflect, refract, 1, getattr(setup, "lights", None), False,
                      True)  # raises with fresnel: the tree's gather is not built here
        check_glossy(glossy, glossy_sets, glossy_filter, glossy_filter_cos, glossy_filter_plane, glossy_radius, glossy_shadows,
                     reflect, refract, aa, temporal, getattr(setup, "lights", None), False, True)  # raises with glossy > 0
        check_temporal(temporal, temporal_cos, temporal_plane, True, getattr(setup, "lights", None), False,
                       True)  # raises with temporal > 0: the effects it averages are not built here
        check_aa(aa, aa_sets, aa_cos, aa_plane, aa_shadows, reflect, frame_cnt, getattr(setup, "lights", None), 0, gi, False,
                 True)  # raises with aa > 0, as gi does
        check_gi(gi, gi_radius, gi_gain, gi_shadows, gi_sets, gi_filter, gi_filter_cos, gi_filter_plane,
                 getattr(setup, "lights", None), False, True)  # raises with gi > 0, as ao and area do
        check_area(area, area_radius, shadows, getattr(setup, "lights", None), True)  # raises with area > 0, as ao does
        check_area_filter(0, area_sets, area_filter, area_filter_cos, area_filter_plane)  # raises unless at the defaults
        check_ao_filter(0, ao_sets, ao_filter, ao_filter_cos, ao_filter_plane)  # the same
        self.refract = check_refract(refract, reflect)
        bounces = check_bounces(bounces)
        reflect_shadows = check_reflect_shadows(reflect_shadows, reflect)
        check_ao(ao, ao_radius, True)  # raises with ao > 0: the uniform grid lives on the side context
        if getattr(setup, "lights", None) is not None:
            check_lights(setup.lights, reflect, True)  # raises: one light grid on the side context
        t, aux, main, side = self.torch, self.aux, self.main_stream, self.side_stream
        if reflect:
            self._ensure_reflect_buffers(bounces, reflect_shadows)
        cam = make_camera(setup.camera, setup.fovy, self.aspect)
        lcam = make_camera(setup.light_camera, setup.fovy, self.aspect)
        ev_grids, ev_dda = t.cuda.Event(), t.cuda.Event()
        ev_prim = [t.cuda.Event() for _ in self._per_band]
        for st in self.streams[1:] + [side]:
            st.wait_stream(main)  # the geometry of this frame (and the last frame's readers) are behind the main stream
        with t.cuda.stream(side):
            if shadows:
                use_light_camera(aux, lcam)
                build_grid(aux, self, GRID_SPHERICAL)
            if reflect:
                build_grid(aux, self, GRID_UNIFORM)
            ev_grids.record(side)
        for b, st, ev in zip(self._per_band, self.streams, ev_prim):
            with t.cuda.stream(st):
                camera_pass(b.ctx, self, b, setup, cam)
                ev.record(st)
        if reflect:
            with t.cuda.stream(side):
                for ev in ev_prim:
                    side.wait_event(ev)
                reflect_rays(aux, self, self._per_band[0].cam_pos)
                trace_reflections(aux, self, bounces, lcam.worldori[:3] if reflect_shadows else None)
                ev_dda.record(side)
        for b, st in zip(self._per_band, self.streams):
            with t.cuda.stream(st):
                use_light_camera(b.ctx, lcam)
                if shadows:
                    map_rays(b.ctx, self, b)
                    sort_rays(b.ctx, b)
                    st.wait_event(ev_grids)
                    trace_shadows(b.ctx, self, b, aux.grid_ptrs(GRID_SPHERICAL))
        for b, st in zip(self._per_band, self.streams):
            with t.cuda.stream(st):
                if reflect:
                    st.wait_event(ev_dda)
                shade_frame(b.ctx, self, b.cam_pos, frame_cnt, shadows, reflect, bounces, reflect_shadows)
        for st in self.streams[1:] + [side]:
            main.wait_stream(st)

    def synchronize(self):
        err = None
        for c in self.contexts():
            try:
                c.synchronize()
            except Exception as e:  # UGRT_EOVERFLOW of any context: one report for the frame
                err = err or e
        if err is not None:
            raise err
