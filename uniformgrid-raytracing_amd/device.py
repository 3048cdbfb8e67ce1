"""Device context: one per GPU / per image band.  Thin wrappers over the C-ABI.

Every tensor argument must be a contiguous torch tensor on the context's device;
only its ``data_ptr()`` crosses the boundary.
"""
import ctypes as C

import numpy as np

from . import lib, check, Config, GridInfo, SlabInfo, STAGES, _f3, _P


def _ptr(t):
    """torch tensor -> device pointer; raw pointers (int / c_void_p) pass through."""
    if t is None:
        return None
    if isinstance(t, (int, C.c_void_p)):
        return t
    assert t.is_contiguous(), "ugrt: tensors must be contiguous"
    return C.c_void_p(t.data_ptr())


def _points(pts):
    """Points as host floats [n, 3] (a sequence of triples or an array; None: no argument) -> (n, the 3n floats)."""
    if pts is None:
        return 0, None
    flat = _f3(np.asarray(pts, np.float32).reshape(-1))
    return len(flat) // 3, flat


class Context:
    def __init__(self, width, height, device=0, light_grid=(128, 128), rows=None, flags=0,
                 uniform_dims=(64, 64, 32), slabs=1):
        import torch  # device memory, streams

        self.torch = torch
        cfg = Config()
        cfg.width, cfg.height, cfg.tile, cfg.slabs = width, height, 8, slabs
        cfg.light_nbx, cfg.light_nby = light_grid
        nby = height // 8
        cfg.row_begin, cfg.row_end = rows if rows is not None else (0, nby)
        cfg.flags = flags
        for k in range(3):
            cfg.uniform_dims[k] = uniform_dims[k]
        self.cfg = cfg
        self.width, self.height = width, height
        self.nbx, self.nby = width // 8, nby
        self.rows = (cfg.row_begin, cfg.row_end)
        self.p0 = cfg.row_begin * 8 * width
        self.npix = (cfg.row_end - cfg.row_begin) * 8 * width
        self.light_grid = tuple(light_grid)
        self.device_index = device
        self._h = _P()
        check(lib.ugrt_ctx_create(C.byref(self._h), device, C.byref(cfg)))
        self.device = torch.device("cuda", device)
        self.use_current_stream()

    def __del__(self):
        if getattr(self, "_h", None):
            lib.ugrt_ctx_destroy(self._h)
            self._h = None

    # -- plumbing ----------------------------------------------------------
    def use_current_stream(self):
        s = self.torch.cuda.current_stream(self.device)
        check(lib.ugrt_ctx_set_stream(self._h, C.c_void_p(s.cuda_stream)))

    def synchronize(self):
        check(lib.ugrt_ctx_synchronize(self._h))

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    def upload(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)

    def wrap_u32(self, ptr, n):
        """int32 tensor view of n uint32 values that the context owns (grid arrays)."""
        if n == 0:
            return self.torch.empty(0, dtype=self.torch.int32, device=self.device)
        key = (int(ptr), int(n))
        cache = self.__dict__.setdefault("_wrap_cache", {})
        if key in cache:
            return cache[key]
        if len(cache) > 64:
            cache.clear()
        cache[key] = self._wrap_u32_uncached(ptr, n)
        return cache[key]

    def _wrap_u32_uncached(self, ptr, n):
        iface = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}
        holder = type("_P", (), {"__cuda_array_interface__": iface})()
        return self.torch.as_tensor(holder, device=self.device)

    # -- camera / light ----------------------------------------------------
    def upload_camera(self, camcoords):
        check(lib.ugrt_upload_camera(self._h, _f3(camcoords)))

    def set_light_position(self, pos):
        check(lib.ugrt_set_light_position(self._h, _f3(pos)))

    # -- grids -------------------------------------------------------------
    def grid_build_perspective(self, d_faces, d_verts, num_faces):
        check(lib.ugrt_grid_build_perspective(self._h, _ptr(d_faces), _ptr(d_verts), num_faces))

    def grid_build_spherical(self, d_faces, d_verts, num_faces, xM, yM):
        """The light grid of the camera block uploaded last (upload_camera).  With FLAG_STATIC_GEOMETRY the call enqueues
        nothing while the grid the context holds was built from the same tensors, face window, xM, yM and camera block
        and the geometry has not changed since (rotate_bunny / geometry_changed); get_state("light_builds_reused")
        counts such calls, option "light_reuse" 0 builds every time (ugrt.h: ugrt_grid_build_spherical)."""
        check(lib.ugrt_grid_build_spherical(self._h, _ptr(d_faces), _ptr(d_verts), num_faces, xM, yM))

    def grid_build_uniform(self, d_faces, d_verts, num_faces, bbmin, bbmax):
        """The uniform grid of the bounce.  With FLAG_STATIC_GEOMETRY the call enqueues nothing while the grid the
        context holds was built from the same tensors, box and face window and the geometry has not changed since
        (rotate_bunny / geometry_changed); get_state("uniform_builds_reused") counts such calls, option
        "uniform_reuse" 0 builds every time (ugrt.h: ugrt_grid_build_uniform)."""
        check(lib.ugrt_grid_build_uniform(self._h, _ptr(d_faces), _ptr(d_verts), num_faces, _f3(bbmin), _f3(bbmax)))

    def grid_build_batch_begin(self):
        """The grid builds that follow (at most two, asynchronous form) stop in front of their sorts ..."""
        check(lib.ugrt_grid_build_batch_begin(self._h))

    def grid_build_batch_end(self):
        """... and are sorted in shared launches and completed here; the grids must not be used before."""
        check(lib.ugrt_grid_build_batch_end(self._h))

    def grid_info(self, which):
        gi = GridInfo()
        check(lib.ugrt_grid_get_info(self._h, which, C.byref(gi)))
        return gi

    def set_face_window(self, begin, end):
        """Triangles [begin, end) the light / uniform builds bin (end < 0: to the last one; 0, -1 = all; begin == end:
        none): this rank's shard of the build."""
        check(lib.ugrt_ctx_set_face_window(self._h, int(begin), int(end)))

    def grid_merge_shards(self, which, keys, vals, spans, counts):
        """keys/vals/spans: per rank, device tensors (or pointers) of that rank's shard; counts: refs per rank."""
        n = len(counts)
        arr = lambda xs: (_P * n)(*[_ptr(x) for x in xs])
        check(lib.ugrt_grid_merge_shards(self._h, which, n, arr(keys), arr(vals), arr(spans),
                                         (C.c_uint * n)(*[int(c) for c in counts])))

    def grid_slabs(self, which):
        si = SlabInfo()
        check(lib.ugrt_grid_get_slabs(self._h, which, C.byref(si)))
        return si

    def grid_ptrs(self, which):
        """(value, span, offset) as raw device pointers + the GridInfo: what a frame loop passes on."""
        gi = self.grid_info(which)
        return gi.d_triangle_value_list, gi.d_span, gi.d_offset, gi

    def grid_arrays(self, which):
        """(value, key, span, offset) as int32 torch views + the GridInfo (tests, analysis)."""
        gi = self.grid_info(which)
        return (self.wrap_u32(gi.d_triangle_value_list, gi.total_refs),
                self.wrap_u32(gi.d_triangle_key_list, gi.total_refs),
                self.wrap_u32(gi.d_span, gi.num_cells), self.wrap_u32(gi.d_offset, gi.num_cells), gi)

    def set_option(self, key, value):
        """Launch-shape options (no effect on results), e.g. "dda_rays_per_wave"; "uniform_reuse" 0 makes
        grid_build_uniform build every time, "light_reuse" 0 grid_build_spherical, "shadow_frags" 0 the shadow pass
        sort every ray where it would sort tile fragments."""
        check(lib.ugrt_ctx_set_option(self._h, key.encode(), int(value)))

    def get_state(self, key):
        """Counters and findings of the context: "radix_launches", "sort_rank_atomic", "shadow_key_bits" (key bits the
        last shadow pass sorted its rays on), "shadow_fragments" (tile fragments the last shadow pass formed and sorted
        instead of its rays, option "shadow_frags"; 0 = it sorted every ray), "uniform_builds_reused" (grid_build_uniform calls that kept the grid the
        context held), "light_builds_reused" (the same for grid_build_spherical), "primary_deferred_merges" / "primary_completed_merges" /
        "primary_merge_pending" (screen-grid builds that put their merge off, those merged later after all, one pending), "recip_mismatches" (runs the exhaustive check of the tracers' reciprocal
        on the device), "f2i_mismatches" (the same for the device's float -> integer conversions), "lane_reduce_mismatches"
        (the tracers' DPP / permlane-swap reductions against __shfl_xor)."""
        v = C.c_longlong(0)
        check(lib.ugrt_ctx_get_state(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def geometry_changed(self):
        """With FLAG_STATIC_GEOMETRY: the vertex or face array was rewritten outside ugrt_animate (the triangle
        records, the light grid and the uniform grid kept from the old contents are built again)."""
        check(lib.ugrt_geometry_changed(self._h))

    def sort_pairs(self, keys_in, keys_out, values_in, values_out, key_bits, library=False):
        """cudppSort on (uint key, uint value) pairs: stable, on key bits [0, key_bits)."""
        check(lib.ugrt_sort_pairs(self._h, _ptr(keys_in), _ptr(keys_out), _ptr(values_in), _ptr(values_out),
                                  keys_in.numel(), key_bits, 1 if library else 0))

    def sort_pairs_lists(self, lists):
        """The built-in sort of one or two lists in shared launches.  Each list is a tuple (keys_in, keys_out, values_in,
        values_out, key_bits[, count[, n]]): count is None (a host count) or one device word holding the pair count, n
        the count or the capacity (default keys_in.numel()); keys_in is keys_out and values_in is values_out sorts in
        place (2 or 4 passes only)."""
        m = len(lists)
        full = [tuple(l) + (None,) * (7 - len(l)) for l in lists]
        arr = lambda i: (_P * m)(*[_ptr(l[i]) for l in full])
        ns = (C.c_size_t * m)(*[int(l[0].numel() if l[6] is None else l[6]) for l in full])
        bits = (C.c_int * m)(*[int(l[4]) for l in full])
        check(lib.ugrt_sort_pairs_lists(self._h, m, arr(0), arr(1), arr(2), arr(3), ns, bits, arr(5)))

    def scan(self, d_in, d_out, inclusive=True, n=None):
        """cudppScan: prefix sums modulo 2^32 of the first n (default d_in.numel()) words."""
        check(lib.ugrt_scan(self._h, _ptr(d_in), _ptr(d_out), d_in.numel() if n is None else int(n), 1 if inclusive else 0))

    def scan_pair(self, in_a, out_a, in_b, out_b, inclusive=True, n=None):
        """Two independent scans of n (default in_a.numel()) words each in one launch."""
        check(lib.ugrt_scan_pair(self._h, _ptr(in_a), _ptr(out_a), _ptr(in_b), _ptr(out_b),
                                 in_a.numel() if n is None else int(n), 1 if inclusive else 0))

    # -- tracing -----------------------------------------------------------
    def trace_primary(self, value, span, offset, normal, t, ray_dir, shadowed, ids, verts, faces):
        """FrustumTracer::trace on the given lists; value, span and offset all None: through the context's current
        perspective grid (trace_primary_grid), which is how a frame traces the grid it has just built."""
        if value is None and span is None and offset is None:
            return self.trace_primary_grid(normal, t, ray_dir, shadowed, ids, verts, faces)
        if value is None or span is None or offset is None:
            raise ValueError("trace_primary: give value, span and offset, or None for all three (the context's own grid)")
        check(lib.ugrt_trace_primary(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(normal), _ptr(t),
                                     _ptr(ray_dir), _ptr(shadowed), _ptr(ids), _ptr(verts), _ptr(faces)))

    def trace_primary_grid(self, normal, t, ray_dir, shadowed, ids, verts, faces):
        """trace_primary through the context's current perspective grid, without asking for its lists: a build whose
        merge of the wide triangles is put off (see ugrt.h) is traced from the narrow runs and the one wide list."""
        check(lib.ugrt_trace_primary_grid(self._h, _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(shadowed), _ptr(ids),
                                          _ptr(verts), _ptr(faces)))

    def map_rays_to_light(self, t, ray_dir, d_map, cam_pos, xM, yM):
        check(lib.ugrt_map_rays_to_light(self._h, _ptr(t), _ptr(ray_dir), _ptr(d_map), _ptr(cam_pos), xM, yM))

    def prefix_capacity(self):
        return self.npix // 64 + self.light_grid[0] * self.light_grid[1] + 2

    def sort_rays(self, d_map, d_prefix, deferred=False):
        """processData.  deferred=True: does not wait for the device; returns CHUNKS_ON_DEVICE, which
        trace_shadow accepts, and sort_rays_chunks() fetches the number later."""
        if deferred:
            check(lib.ugrt_sort_rays(self._h, _ptr(d_map), _ptr(d_prefix), d_prefix.numel(), None))
            return 0xFFFFFFFF
        n = C.c_uint()
        check(lib.ugrt_sort_rays(self._h, _ptr(d_map), _ptr(d_prefix), d_prefix.numel(), C.byref(n)))
        return n.value

    def sort_rays_chunks(self):
        n = C.c_uint()
        check(lib.ugrt_sort_rays_chunks(self._h, C.byref(n)))
        return n.value

    def trace_shadow(self, value, verts, faces, span, offset, t, ray_dir, is_shadowed, d_map, d_prefix, cam_pos,
                     num_chunks):
        check(lib.ugrt_trace_shadow(self._h, _ptr(value), _ptr(verts), _ptr(faces), _ptr(span), _ptr(offset),
                                    _ptr(t), _ptr(ray_dir), _ptr(is_shadowed), _ptr(d_map), _ptr(d_prefix),
                                    _ptr(cam_pos), num_chunks))

    # -- shading -----------------------------------------------------------
    def shade_simple(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, num_materials):
        check(lib.ugrt_shade_simple(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids),
                                    _ptr(cam_pos), _ptr(mat_idx), _ptr(mat_list), num_materials))

    def shade_lights(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, num_materials, light_pos,
                     is_shadowed=None):
        """shade_simple + shade_add_shadows per light and the mean, in one pass.  light_pos: one
        position (three host floats) per light; is_shadowed: the lights' flags stacked [L, W*H], or None."""
        n, pos = _points(light_pos)
        check(lib.ugrt_shade_lights(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(cam_pos),
                                    _ptr(mat_idx), _ptr(mat_list), num_materials, n, pos, _ptr(is_shadowed)))

    def shade_spotlight(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, num_materials, dump=None):
        check(lib.ugrt_shade_spotlight(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids),
                                       _ptr(cam_pos), _ptr(mat_idx), _ptr(mat_list), num_materials, _ptr(dump)))

    def shade_add_shadows(self, img, is_shadowed):
        check(lib.ugrt_shade_add_shadows(self._h, _ptr(img), _ptr(is_shadowed)))

    def shade_perlin(self, img, t, ray_dir, cam_pos, ids):
        check(lib.ugrt_shade_perlin(self._h, _ptr(img), _ptr(t), _ptr(ray_dir), _ptr(cam_pos), _ptr(ids)))

    # -- reflection bounce ---------------------------------------------------
    def reflect_rays(self, cam_pos, t, ray_dir, ids, mat_idx, reflect, num_materials, verts, faces, eps, rays,
                     active):
        check(lib.ugrt_reflect_rays(self._h, _ptr(cam_pos), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(mat_idx),
                                    _ptr(reflect), num_materials, _ptr(verts), _ptr(faces), eps, _ptr(rays),
                                    _ptr(active)))

    def trace_dda(self, value, span, offset, verts, faces, rays, active, hit_t, hit_id):
        check(lib.ugrt_trace_dda(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                 _ptr(rays), _ptr(active), _ptr(hit_t), _ptr(hit_id)))

    def shade_reflect(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, reflect, num_materials,
                      verts, faces, rays, active, hit_t, hit_id):
        check(lib.ugrt_shade_reflect(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids),
                                     _ptr(cam_pos), _ptr(mat_idx), _ptr(mat_list), _ptr(reflect), num_materials,
                                     _ptr(verts), _ptr(faces), _ptr(rays), _ptr(active), _ptr(hit_t),
                                     _ptr(hit_id)))

    def reflect_rays_next(self, rays, active, hit_t, hit_id, mat_idx, reflect, num_materials, verts, faces, eps,
                          rays_next, active_next):
        """Level j's hits -> level j+1's reflected rays (j >= 1; level 1 is reflect_rays)."""
        check(lib.ugrt_reflect_rays_next(self._h, _ptr(rays), _ptr(active), _ptr(hit_t), _ptr(hit_id), _ptr(mat_idx),
                                         _ptr(reflect), num_materials, _ptr(verts), _ptr(faces), eps,
                                         _ptr(rays_next), _ptr(active_next)))

    def shade_reflect_depth(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, reflect, num_materials,
                            verts, faces, depth, rays, active, hit_t, hit_id):
        """shade_reflect over `depth` levels; rays / active / hit_t / hit_id hold levels 1..depth one behind the
        other (level j at (j-1) * W*H pixels)."""
        check(lib.ugrt_shade_reflect_depth(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids),
                                           _ptr(cam_pos), _ptr(mat_idx), _ptr(mat_list), _ptr(reflect),
                                           num_materials, _ptr(verts), _ptr(faces), int(depth), _ptr(rays),
                                           _ptr(active), _ptr(hit_t), _ptr(hit_id)))

    # -- shadows on reflected hits --------------------
    def occlusion_rays(self, rays, active, hit_t, hit_id, verts, faces, light_pos, eps, orays, oactive):
        """One level's hits -> rays towards light_pos (three host floats); the light lies at t = 1."""
        check(lib.ugrt_occlusion_rays(self._h, _ptr(rays), _ptr(active), _ptr(hit_t), _ptr(hit_id), _ptr(verts),
                                      _ptr(faces), _f3(light_pos), eps, _ptr(orays), _ptr(oactive)))

    def trace_dda_any(self, value, span, offset, verts, faces, rays, active, t_max, occluded):
        """occluded[p] = 1 where a triangle of a visited cell is hit with 0 < t < t_max."""
        check(lib.ugrt_trace_dda_any(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                     _ptr(rays), _ptr(active), t_max, _ptr(occluded)))

    def shade_reflect_depth_occluded(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, reflect,
                                     num_materials, verts, faces, depth, rays, active, hit_t, hit_id, occluded):
        """shade_reflect_depth with the levels whose hit is occluded (stacked like active) darkened to a third."""
        check(lib.ugrt_shade_reflect_depth_occluded(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir),
                                                    _ptr(ids), _ptr(cam_pos), _ptr(mat_idx), _ptr(mat_list),
                                                    _ptr(reflect), num_materials, _ptr(verts), _ptr(faces), int(depth),
                                                    _ptr(rays), _ptr(active), _ptr(hit_t), _ptr(hit_id),
                                                    _ptr(occluded)))

    # -- reflections under several lights -------------
    def trace_dda_any_lights(self, value, span, offset, verts, faces, orays, oactive, light_pos, occluded):
        """occluded[l, p] = trace_dda_any's flag (t_max 1) of the ray from orays' origin of p towards light_pos[l]; light_pos:
        one point (three host floats) per light; occluded: the lights' flags stacked [L, W*H]."""
        n, pos = _points(light_pos)
        check(lib.ugrt_trace_dda_any_lights(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                            _ptr(orays), _ptr(oactive), n, pos, _ptr(occluded)))

    def shade_reflect_lights(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, reflect, num_materials,
                             verts, faces, depth, rays, active, hit_t, hit_id, light_pos, is_shadowed=None,
                             occluded=None):
        """shade_reflect_depth_occluded + shade_add_shadows per light and the mean, in one pass.  light_pos: one position
        (three host floats) per light; is_shadowed: [L, W*H] or None; occluded: [depth, L, W*H] or None."""
        n, pos = _points(light_pos)
        check(lib.ugrt_shade_reflect_lights(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids),
                                            _ptr(cam_pos), _ptr(mat_idx), _ptr(mat_list), _ptr(reflect), num_materials,
                                            _ptr(verts), _ptr(faces), int(depth), _ptr(rays), _ptr(active), _ptr(hit_t),
                                            _ptr(hit_id), n, pos, _ptr(is_shadowed), _ptr(occluded)))

    # -- ambient occlusion ------------------------------
    def ao_rays(self, cam_pos, t, ray_dir, ids, verts, faces, eps, orays, oactive):
        """The primary hits (triangle ids: before any shading call) -> {o', n} per pixel: the origin reflect_rays gives
        the reflected ray and the flipped unit normal."""
        check(lib.ugrt_ao_rays(self._h, _ptr(cam_pos), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(verts), _ptr(faces), eps,
                               _ptr(orays), _ptr(oactive)))

    def trace_dda_any_hemi(self, value, span, offset, verts, faces, orays, oactive, dirs, radius, mask):
        """Bit s of mask[p] = trace_dda_any's flag (t_max radius) of the ray from orays' origin of p along dirs[s] in the
        basis of orays' normal of p; dirs: host floats [S, 3] (scenes.ao_directions), z along the normal; mask: uint32
        words (an int32 tensor serves)."""
        n, flat = _points(dirs)
        check(lib.ugrt_trace_dda_any_hemi(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                          _ptr(orays), _ptr(oactive), n, flat, radius, _ptr(mask)))

    def shade_ao(self, img, mask, num_dirs):
        """Each byte b of a pixel becomes (b * open) // num_dirs, open = num_dirs - popcount(mask & low num_dirs bits)."""
        check(lib.ugrt_shade_ao(self._h, _ptr(img), _ptr(mask), int(num_dirs)))

    # -- refraction -------------------------------------
    def refract_rays(self, cam_pos, t, ray_dir, ids, mat_idx, reflect, transmit, ior, num_materials, verts, faces, eps,
                     rays, active):
        """reflect_rays where a material with transmit > 0 sends the refracted ray on instead (index ior)."""
        check(lib.ugrt_refract_rays(self._h, _ptr(cam_pos), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(mat_idx),
                                    _ptr(reflect), _ptr(transmit), _ptr(ior), num_materials, _ptr(verts), _ptr(faces),
                                    eps, _ptr(rays), _ptr(active)))

    def refract_rays_next(self, rays, active, hit_t, hit_id, mat_idx, reflect, transmit, ior, num_materials, verts,
                          faces, eps, rays_next, active_next):
        """reflect_rays_next where a material with transmit > 0 sends the refracted ray on instead."""
        check(lib.ugrt_refract_rays_next(self._h, _ptr(rays), _ptr(active), _ptr(hit_t), _ptr(hit_id), _ptr(mat_idx),
                                         _ptr(reflect), _ptr(transmit), _ptr(ior), num_materials, _ptr(verts),
                                         _ptr(faces), eps, _ptr(rays_next), _ptr(active_next)))

    def trace_dda_any_thru(self, value, span, offset, verts, faces, rays, active, t_max, occluded, mat_idx, transmit,
                           num_materials):
        """trace_dda_any in which a triangle whose material has transmit > 0 does not occlude."""
        check(lib.ugrt_trace_dda_any_thru(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                          _ptr(rays), _ptr(active), t_max, _ptr(occluded), _ptr(mat_idx),
                                          _ptr(transmit), num_materials))

    def trace_dda_any_lights_thru(self, value, span, offset, verts, faces, orays, oactive, light_pos, occluded, mat_idx,
                                  transmit, num_materials):
        """trace_dda_any_lights in which a triangle whose material has transmit > 0 does not occlude."""
        n, pos = _points(light_pos)
        check(lib.ugrt_trace_dda_any_lights_thru(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts),
                                                 _ptr(faces), _ptr(orays), _ptr(oactive), n, pos, _ptr(occluded),
                                                 _ptr(mat_idx), _ptr(transmit), num_materials))

    # -- area lights -------------------------------------
    def trace_dda_any_area(self, value, span, offset, verts, faces, orays, oactive, samples, mask):
        """Bit s of mask[p] = trace_dda_any's flag (t_max 1) of the ray from orays' origin of p towards samples[s];
        samples: host floats [S, 3], world positions (scenes.area_samples); mask: uint32 words (an int32 tensor serves)."""
        n, flat = _points(samples)
        check(lib.ugrt_trace_dda_any_area(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                          _ptr(orays), _ptr(oactive), n, flat, _ptr(mask)))

    def trace_dda_any_area_thru(self, value, span, offset, verts, faces, orays, oactive, samples, mask, mat_idx, transmit,
                                num_materials):
        """trace_dda_any_area in which a triangle whose material has transmit > 0 does not occlude."""
        n, flat = _points(samples)
        check(lib.ugrt_trace_dda_any_area_thru(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                               _ptr(orays), _ptr(oactive), n, flat, _ptr(mask), _ptr(mat_idx),
                                               _ptr(transmit), num_materials))

    def shade_area(self, img, mask, num_samples):
        """Each byte b of a pixel becomes (b * (S + 2 * lit)) // (3 * S), lit = S - popcount(mask & low S bits)."""
        check(lib.ugrt_shade_area(self._h, _ptr(img), _ptr(mask), int(num_samples)))

    # -- interleaved sample sets and the gather ----------
    def trace_dda_any_area_sets(self, value, span, offset, verts, faces, orays, oactive, num_samples, set_w, set_h,
                                sample_pos, mask):
        """trace_dda_any_area with a sample set per pixel of a set_w x set_h tile: pixel (x, y) of the full image aims at
        set (y % set_h) * set_w + x % set_w of sample_pos, a DEVICE tensor of floats [set_w * set_h, num_samples, 3]
        (scenes.area_sample_sets, uploaded)."""
        check(lib.ugrt_trace_dda_any_area_sets(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                               _ptr(orays), _ptr(oactive), int(num_samples), int(set_w), int(set_h),
                                               _ptr(sample_pos), _ptr(mask)))

    def trace_dda_any_area_sets_thru(self, value, span, offset, verts, faces, orays, oactive, num_samples, set_w, set_h,
                                     sample_pos, mask, mat_idx, transmit, num_materials):
        """trace_dda_any_area_sets in which a triangle whose material has transmit > 0 does not occlude."""
        check(lib.ugrt_trace_dda_any_area_sets_thru(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts),
                                                    _ptr(faces), _ptr(orays), _ptr(oactive), int(num_samples), int(set_w),
                                                    int(set_h), _ptr(sample_pos), _ptr(mask), _ptr(mat_idx),
                                                    _ptr(transmit), num_materials))

    def filter_visibility(self, mask, num_bits, orays, oactive, radius, normal_cos, plane_tol, vis):
        """The edge-aware gather: vis[2p] = sum of w * open_q and vis[2p + 1] = sum of w over the active pixels q within
        `radius` of p (inside the image and the band) whose normal and plane agree with p's (orays / oactive: what ao_rays
        wrote), w = (R + 1 - |dx|) * (R + 1 - |dy|), open_q = num_bits - popcount(mask[q] & low num_bits bits); vis:
        uint32 words [2 * W * H] (an int32 tensor serves)."""
        check(lib.ugrt_filter_visibility(self._h, _ptr(mask), int(num_bits), _ptr(orays), _ptr(oactive), int(radius),
                                         normal_cos, plane_tol, _ptr(vis)))

    def shade_area_vis(self, img, vis, num_samples):
        """Each byte b of a pixel with den = vis[2p + 1] != 0 becomes (b * (S * den + 2 * vis[2p])) // (3 * S * den)."""
        check(lib.ugrt_shade_area_vis(self._h, _ptr(img), _ptr(vis), int(num_samples)))

    # -- ambient occlusion over interleaved direction sets
    def trace_dda_any_hemi_sets(self, value, span, offset, verts, faces, orays, oactive, num_dirs, set_w, set_h, dirs,
                                radius, mask):
        """trace_dda_any_hemi with a set of directions per pixel of a set_w x set_h tile, the rays of a pixel side by side
        in a wave: pixel (x, y) of the full image walks along set (y % set_h) * set_w + x % set_w of dirs, a DEVICE tensor
        of floats [set_w * set_h, num_dirs, 3] (scenes.ao_direction_sets, uploaded), z along the normal."""
        check(lib.ugrt_trace_dda_any_hemi_sets(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                               _ptr(orays), _ptr(oactive), int(num_dirs), int(set_w), int(set_h),
                                               _ptr(dirs), radius, _ptr(mask)))

    def shade_ao_vis(self, img, vis, num_dirs):
        """Each byte b of a pixel with den = vis[2p + 1] != 0 becomes (b * vis[2p]) // (num_dirs * den)."""
        check(lib.ugrt_ao_shade_vis(self._h, _ptr(img), _ptr(vis), int(num_dirs)))

    # -- indirect diffuse light -------------------------
    def gi_gather(self, value, span, offset, verts, faces, orays, oactive, num_dirs, set_w, set_h, dirs, radius, mat_idx,
                  mat_list, num_materials, shadow_light, eps, sums):
        """The closest-hit hemisphere gather: pixel p walks trace_dda_any_hemi_sets' num_dirs rays (dirs: the DEVICE
        table [set_w * set_h, num_dirs, 3]) to their first hit below radius (float('inf'): the whole grid), shades the
        hit as a reflection level's hit is shaded, divides by 3 where the hit does not see shadow_light (three host floats,
        or None: no shadow phase), and sums the bytes: sums[4p + k] for k < 3, sums[4p + 3] = 1; sums: uint32 words
        [4 * W * H] (an int32 tensor serves)."""
        light = None if shadow_light is None else _points([shadow_light])[1]
        check(lib.ugrt_gi_gather(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces), _ptr(orays),
                                 _ptr(oactive), int(num_dirs), int(set_w), int(set_h), _ptr(dirs), radius, _ptr(mat_idx),
                                 _ptr(mat_list), int(num_materials), light, eps, _ptr(sums)))

    def gi_filter(self, sums, orays, oactive, radius, normal_cos, plane_tol, acc):
        """filter_visibility's gather over gi_gather's sums: acc[4p + k] = sum of w * sums[4q + k] for k < 3 and
        acc[4p + 3] = sum of w; acc: uint32 words [4 * W * H]."""
        check(lib.ugrt_gi_filter(self._h, _ptr(sums), _ptr(orays), _ptr(oactive), int(radius), normal_cos, plane_tol,
                                 _ptr(acc)))

    def gi_apply(self, img, acc, num_dirs, gain, ids, mat_list, num_materials):
        """Behind the shading call (ids holds material indices): each byte b of a pixel with a material in range and
        den = acc[4p + 3] != 0 becomes min(255, b + byte(clamp((Kd * gain) * (acc[4p + k] / (255 * num_dirs * den)))))."""
        check(lib.ugrt_gi_apply(self._h, _ptr(img), _ptr(acc), int(num_dirs), gain, _ptr(ids), _ptr(mat_list),
                                int(num_materials)))

    # -- glossy reflections ----------------------------
    def glossy_gather(self, value, span, offset, verts, faces, rays, active, orays, ids, mat_idx, spread, num_samples, set_w,
                      set_h, points, radius, mat_list, num_materials, shadow_light, eps, sums):
        """The lobe's closest-hit gather, before the shading call (ids holds triangle ids): an active pixel p of
        reflect_rays' {o, R} sends num_samples rays from o around normalize(R), tilted by spread[material] times the
        points of its set (points: the DEVICE table [set_w * set_h, num_samples, 2], scenes.glossy_point_sets) and
        mirrored back over the surface where they would enter it (orays: ao_rays' {o', n}); each is walked, shaded,
        shadowed and summed as gi_gather does it: sums[4p + k] for k < 3, sums[4p + 3] = 1."""
        light = None if shadow_light is None else _points([shadow_light])[1]
        check(lib.ugrt_glossy_gather(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces), _ptr(rays),
                                     _ptr(active), _ptr(orays), _ptr(ids), _ptr(mat_idx), _ptr(spread), int(num_samples),
                                     int(set_w), int(set_h), _ptr(points), radius, _ptr(mat_list), int(num_materials), light,
                                     eps, _ptr(sums)))

    def glossy_apply(self, img, acc, num_samples, ids, reflect, num_materials):
        """Directly behind the shading call (ids holds material indices): each byte b of a pixel with den = acc[4p + 3]
        != 0 and k = min(reflect[material], 1) > 0 becomes round((1 - k) * b + k * acc[4p + c] / (num_samples * den))."""
        check(lib.ugrt_glossy_apply(self._h, _ptr(img), _ptr(acc), int(num_samples), _ptr(ids), _ptr(reflect),
                                    int(num_materials)))

    # -- Fresnel glass ----------------------------------
    def fresnel_gather(self, value, span, offset, verts, faces, rays, active, normal, t, ray_dir, ids, cam_pos, mat_idx,
                       mat_list, reflect, transmit, ior, num_materials, depth, scale, min_weight, shadow_light, eps, acc):
        """A pixel's whole ray tree in one launch, before the shading call (ids holds triangle ids): an active pixel of
        refract_rays' level-1 rays follows, at every glass hit down to level `depth` (1..MAX_FRESNEL_DEPTH), the
        transmitted ray with (1 - F) and the reflected ray with F of the material's transmit, F = scale * Schlick's share,
        children of a weight <= min_weight dropped; the levels' Lambert colours (a third where shadow_light, three host
        floats or None, is hidden behind something that is not glass) are blended as shade_reflect_depth blends the
        chain's: acc[4p + k] for k < 3 (float32), acc[4p + 3] = 1."""
        light = None if shadow_light is None else _points([shadow_light])[1]
        check(lib.ugrt_fresnel_gather(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces), _ptr(rays),
                                      _ptr(active), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(cam_pos),
                                      _ptr(mat_idx), _ptr(mat_list), _ptr(reflect), _ptr(transmit), _ptr(ior),
                                      int(num_materials), int(depth), scale, min_weight, light, eps, _ptr(acc)))

    def shade_fresnel(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, num_materials, acc):
        """The shading call of a fresnel frame (ugrt_fresnel_shade; ids become material indices): the bytes of
        fresnel_gather's sums where acc[4p + 3] != 0, elsewhere the primary hit's colour as shade_reflect_depth gives it
        to a pixel without a level-1 ray."""
        check(lib.ugrt_fresnel_shade(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(cam_pos),
                                     _ptr(mat_idx), _ptr(mat_list), int(num_materials), _ptr(acc)))

    # -- smooth shading ---------------------------------
    def smooth_adjacency(self, faces, num_faces, num_vertices, vertex_key=None):
        """The corners 3f + k of the face list stably sorted by their vertex's key (vertex_key: a DEVICE tensor of one
        int32 per vertex, scenes.weld's, or None: the vertex itself) and the keys' starts, kept by the context; indices and
        keys lie in 0..num_vertices-1.  get_state("smooth_adjacency_builds") counts the calls."""
        check(lib.ugrt_smooth_adjacency(self._h, _ptr(faces), int(num_faces), int(num_vertices), _ptr(vertex_key)))
        self._smooth_counts = (int(num_faces), int(num_vertices))  # (the sizes of smooth_get_adjacency's views)

    def smooth_get_adjacency(self):
        """(corners [3F], start [V + 1]) as int32 torch views of the context's arrays (tests)."""
        corners, start = _P(), _P()
        check(lib.ugrt_smooth_get_adjacency(self._h, C.byref(corners), C.byref(start)))
        nf, nv = self._smooth_counts
        return (self._wrap_u32_uncached(corners.value, 3 * nf) if nf else self.wrap_u32(0, 0),
                self._wrap_u32_uncached(start.value, nv + 1))

    def smooth_corner_normals(self, faces, verts, num_faces, crease_cos, corner_normals):
        """corner_normals[9F]: per corner the normalised sum of the area-weighted normals of the faces around its key
        whose unit normal lies within crease_cos of its own face's (<= -1: all of them, > 1: its own only), in the
        adjacency's list order; the face's own normal where that sum has no direction.  Needs smooth_adjacency.
        get_state("smooth_normal_builds") counts the calls."""
        check(lib.ugrt_smooth_corner_normals(self._h, _ptr(faces), _ptr(verts), int(num_faces), crease_cos,
                                             _ptr(corner_normals)))

    def smooth_normals(self, t, ray_dir, ids, cam_pos, verts, faces, corner_normals, normal_in, fold, normal_out):
        """Before the shading call (ids holds triangle ids): normal_out[3p ..] = the hit triangle's corner normals mixed
        with the hit's barycentric coordinates and normalised, the triangle's own normal where that fails or points away
        from it, folded into the positive octant with fold; normal_in's where the pixel has no hit.  normal_out may be
        normal_in."""
        check(lib.ugrt_smooth_normals(self._h, _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(cam_pos), _ptr(verts), _ptr(faces),
                                      _ptr(corner_normals), _ptr(normal_in), 1 if fold else 0, _ptr(normal_out)))

    # -- texture mapping ----------------------------------
    def texture_set(self, textures):
        """The mip atlas of `textures`, a list of uint8 host arrays [H, W, 3] (row 0: v = 0); an empty list drops it.  Level 0
        is copied, the further levels are built on the device; the call does not wait.  get_state("texture_builds")
        counts the calls that built."""
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in textures]
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("ugrt: a texture is a uint8 array [H, W, 3], not %r" % (a.shape,))
        n = len(arrs)
        wh = (C.c_int * max(2 * n, 1))(*[d for a in arrs for d in (a.shape[1], a.shape[0])])
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        check(lib.ugrt_texture_set(self._h, n, wh, ptrs))

    def texture_get_level(self, tex, level):
        """(width, height, the level's packed words r | g << 8 | b << 16 | 255 << 24 as an int32 tensor view) (tests)."""
        w, h, p = C.c_int(), C.c_int(), C.c_void_p()
        check(lib.ugrt_texture_get_level(self._h, int(tex), int(level), C.byref(w), C.byref(h), C.byref(p)))
        return w.value, h.value, self._wrap_u32_uncached(p.value, w.value * h.value)

    def texture_albedo(self, t, ray_dir, ids, cam_pos, verts, faces, uvs, num_uvs, uv_faces, mat_idx, mat_list, num_materials,
                       mat_texture, mat_texture_host, max_aniso, lod_bias, albedo):
        """The diffuse colour of every pixel's primary hit, three floats per pixel, before the shading call (ids: triangle
        ids): Kd, times the texture of the hit's material filtered over the pixel's footprint -- up to max_aniso trilinear
        taps along its longer axis -- where the material has one (mat_texture[m] >= 0) and the triangle has uvs.
        mat_texture_host: the host copy of mat_texture (a sequence of ints), which the call checks against the atlas."""
        host = np.ascontiguousarray(mat_texture_host, dtype=np.int32)
        check(lib.ugrt_texture_albedo(self._h, _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(cam_pos), _ptr(verts), _ptr(faces),
                                      _ptr(uvs), int(num_uvs), _ptr(uv_faces), _ptr(mat_idx), _ptr(mat_list), int(num_materials),
                                      _ptr(mat_texture), host.ctypes.data_as(C.POINTER(C.c_int)), int(max_aniso), int(lod_bias),
                                      _ptr(albedo)))

    def texture_shade(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, num_materials, albedo):
        """shade_simple with the pixel's albedo (texture_albedo) in the place of its material's Kd."""
        check(lib.ugrt_texture_shade(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(cam_pos),
                                    _ptr(mat_idx), _ptr(mat_list), num_materials, _ptr(albedo)))

    def texture_shade_spotlight(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, num_materials, albedo, dump=None):
        """shade_spotlight with the pixel's albedo (texture_albedo) in the place of its material's Kd."""
        check(lib.ugrt_texture_shade_spotlight(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(cam_pos),
                                               _ptr(mat_idx), _ptr(mat_list), num_materials, _ptr(dump), _ptr(albedo)))

    def texture_shade_lights(self, img, normal, t, ray_dir, ids, cam_pos, mat_idx, mat_list, num_materials, light_pos,
                            is_shadowed, albedo):
        """shade_lights with the pixel's albedo (texture_albedo) in the place of its material's Kd."""
        n, pos = _points(light_pos)
        check(lib.ugrt_texture_shade_lights(self._h, _ptr(img), _ptr(normal), _ptr(t), _ptr(ray_dir), _ptr(ids), _ptr(cam_pos),
                                           _ptr(mat_idx), _ptr(mat_list), num_materials, n, pos, _ptr(is_shadowed),
                                           _ptr(albedo)))

    # -- anti-aliasing --------------------------------
    def aa_edges(self, normal, t, dirs, ids, cam_pos, mat_idx, is_shadowed, normal_cos, plane_tol, edge):
        """Before the shading call (ids holds triangle ids): edge[p] = 1 where one of the up to eight neighbours of p
        differs from it in hit or miss, in material, in its normal by more than normal_cos, in its plane by more than
        plane_tol (the last three between different triangles), or, with is_shadowed (None: not looked at), in its
        shadow flag; 0 elsewhere.  edge: int32 [W * H]."""
        check(lib.ugrt_aa_edges(self._h, _ptr(normal), _ptr(t), _ptr(dirs), _ptr(ids), _ptr(cam_pos), _ptr(mat_idx),
                                _ptr(is_shadowed), normal_cos, plane_tol, _ptr(edge)))

    def aa_gather(self, value, span, offset, verts, faces, eye_camcoords, edge, num_samples, set_w, set_h, offsets, mat_idx,
                  mat_list, num_materials, shadow_light, eps, sums):
        """The sub-pixel eye rays of the pixels with edge[p] != 0: num_samples rays from the eye of eye_camcoords (64 host
        floats: the EYE's block, whatever block the context holds) through (col + sx, row + sy), (sx, sy) from offsets (the
        DEVICE table [set_w * set_h, num_samples, 2]: scenes.aa_offset_sets, uploaded), each to its closest hit, shaded as
        the frame shades a primary hit under the context's current camera block, each byte b / 3 where the hit does not see
        shadow_light (three host floats, or None: no shadow phase); sums[4p + k] for k < 3 holds the bytes' sums and
        sums[4p + 3] = 1; sums: uint32 words [4 * W * H] (an int32 tensor serves)."""
        light = None if shadow_light is None else _points([shadow_light])[1]
        check(lib.ugrt_aa_gather(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                 None if eye_camcoords is None else _f3(eye_camcoords), _ptr(edge), int(num_samples), int(set_w),
                                 int(set_h), _ptr(offsets), _ptr(mat_idx), _ptr(mat_list), int(num_materials), light, eps,
                                 _ptr(sums)))

    def aa_resolve(self, img, sums, num_samples):
        """Behind the shading calls: each byte of a pixel with sums[4p + 3] != 0 becomes
        (sums[4p + k] + num_samples // 2) // num_samples; every other pixel stays."""
        check(lib.ugrt_aa_resolve(self._h, _ptr(img), _ptr(sums), int(num_samples)))

    # -- depth of field --------------------------------
    def dof_pixels(self, t, dirs, ids, axis, focus, coc_scale, coc_min, radius, flags):
        """Before the shading call (ids holds triangle ids): flags[p] = 1 where the circle of confusion of a pixel q within
        `radius` pixels of p (p included) is at least coc_min and at least max(|dx|, |dy|) wide; 0 elsewhere.  The circle of
        a hit at depth z = t * (dir . axis) > 0 is coc_scale * |z - focus| / z, of every other pixel 0.  axis: three host
        floats, the unit view axis; flags: int32 [W * H]."""
        check(lib.ugrt_dof_pixels(self._h, _ptr(t), _ptr(dirs), _ptr(ids), None if axis is None else _f3(axis), focus,
                                  coc_scale, coc_min, int(radius), _ptr(flags)))

    def dof_gather(self, value, span, offset, verts, faces, eye_camcoords, lens, flags, num_samples, set_w, set_h, table,
                   mat_idx, mat_list, num_materials, shadow_light, eps, sums):
        """The lens rays of the pixels with flags[p] != 0: aa_gather with a table of (sx, sy, lu, lv) entries (the DEVICE
        table [set_w * set_h, num_samples, 4]: scenes.lens_sample_sets, uploaded) and lens, ten host floats: U[3] and V[3],
        the lens's axes with the lens radius as their length, A[3], the unit view axis, and F, the focus distance along
        A.  A sample starts at eye + lu U + lv V and meets the pinhole ray through (col + sx, row + sy) on the plane
        A . (P - eye) = F; everything else, sums included, is aa_gather's."""
        light = None if shadow_light is None else _points([shadow_light])[1]
        check(lib.ugrt_dof_gather(self._h, _ptr(value), _ptr(span), _ptr(offset), _ptr(verts), _ptr(faces),
                                  None if eye_camcoords is None else _f3(eye_camcoords), None if lens is None else _f3(lens),
                                  _ptr(flags), int(num_samples), int(set_w), int(set_h), _ptr(table), _ptr(mat_idx),
                                  _ptr(mat_list), int(num_materials), light, eps, _ptr(sums)))

    # -- temporal accumulation -------------------------
    def temporal_visibility(self, vis, num_bits, orays, oactive, prev_camcoords, prev_orays, prev_oactive, hist_in, max_frames,
                            normal_cos, plane_tol, hist_out, vis_out):
        """The running mean of a gathered share: vis is what filter_visibility wrote for this frame, hist_in / hist_out
        floats [2 * W * H], (share, frames) per pixel.  The share c = vis[2p] / (num_bits * vis[2p + 1]) of an active pixel
        is blended into the history of the frame before, fetched with four taps in sixteenths of a pixel where the pixel's
        origin (orays) lay under prev_camcoords (64 host floats: the EYE's block of the previous frame) and kept where
        prev_orays / prev_oactive hold the same surface (normal_cos, plane_tol): h = hp + (c - hp) / n, n = min(frames of
        the taps + 1, max_frames); without a tap h = c, n = 1.  vis_out: the pair (round(h * num_bits * 256), 256) that
        shade_area_vis and shade_ao_vis take; uint32 words [2 * W * H] (an int32 tensor serves)."""
        check(lib.ugrt_temporal_visibility(self._h, _ptr(vis), int(num_bits), _ptr(orays), _ptr(oactive),
                                           None if prev_camcoords is None else _f3(prev_camcoords), _ptr(prev_orays),
                                           _ptr(prev_oactive), _ptr(hist_in), int(max_frames), normal_cos, plane_tol,
                                           _ptr(hist_out), _ptr(vis_out)))

    def temporal_gi(self, acc, num_dirs, orays, oactive, prev_camcoords, prev_orays, prev_oactive, hist_in, max_frames,
                    normal_cos, plane_tol, hist_out, acc_out):
        """temporal_visibility over gi_filter's sums: acc / acc_out uint32 words and hist_in / hist_out floats
        [4 * W * H], (r, g, b shares, frames) per pixel, c_k = acc[4p + k] / (255 * num_dirs * acc[4p + 3]); acc_out:
        (round(h_k * 255 * num_dirs * 256) for k < 3, 256), what gi_apply takes."""
        check(lib.ugrt_temporal_gi(self._h, _ptr(acc), int(num_dirs), _ptr(orays), _ptr(oactive),
                                   None if prev_camcoords is None else _f3(prev_camcoords), _ptr(prev_orays), _ptr(prev_oactive),
                                   _ptr(hist_in), int(max_frames), normal_cos, plane_tol, _ptr(hist_out), _ptr(acc_out)))

    # -- animation -----------------------------------------------------------
    def animate(self, verts, orig, size, offset, rot):
        check(lib.ugrt_animate(self._h, _ptr(verts), _ptr(orig), size, offset, rot))

    # -- profiling -----------------------------------------------------------
    def prof_enable(self, on=True, stages=None):
        """stages: iterable of stage names to time (default: all)."""
        if on and stages is not None:
            mask = 0
            for name in stages:
                mask |= 1 << (STAGES.index(name) + 1)
            check(lib.ugrt_prof_enable(self._h, mask))
        else:
            check(lib.ugrt_prof_enable(self._h, 1 if on else 0))

    def prof_reset(self):
        check(lib.ugrt_prof_reset(self._h))

    def prof_get(self):
        """{stage name: (total ms, launches)} since the last reset."""
        out = {}
        for i, name in enumerate(STAGES):
            ms, n = C.c_double(), C.c_int()
            check(lib.ugrt_prof_get(self._h, i, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def stats(self):
        a = (C.c_ulonglong * 8)()
        check(lib.ugrt_stats_get(self._h, a))
        return list(a)

    PRIMARY_STATS = ("items", "batches", "batches_with_tile_survivors", "references", "tile_survivors",
                     "quadrant_survivors", "jobs", "flushes", "rounds", "rounds_to_division", "rounds_to_v",
                     "rounds_to_t", "lane_tests", "hits", "jobs_behind_the_flush_s_final_hits", "jobs_dropped_by_the_depth_bound")

    def stats_primary(self):
        """Work counters of the primary tracer's last counting launch (a FLAG_COUNT_WORK context)."""
        a = (C.c_ulonglong * 16)()
        check(lib.ugrt_stats_primary(self._h, a, 16))
        return dict(zip(self.PRIMARY_STATS, list(a)))

    WALK_STATS = ("windows", "jobs", "job_rays", "cull_batches", "cull_tests", "rounds", "round_pairs", "empty_windows")

    def stats_dda_split(self):
        """Split walks of the last trace_dda (option dda_split): segments the cut groups were listed as, jobs of the launch
        before, cut groups with rays that were walked again in one piece, those rays."""
        a = (C.c_uint * 4)()
        check(lib.ugrt_stats_dda_split(self._h, a))
        return dict(zip(("segments", "jobs_of_the_launch_before", "groups_walked_again", "rays_walked_again"), list(a)))

    def stats_dda(self, kernel=0):
        """Work sharing of the window kernel's last counting launch (a FLAG_COUNT_WORK context, "dda_kernel" 0)."""
        a = (C.c_ulonglong * 46)()
        check(lib.ugrt_stats_dda(self._h, a, 46))
        d = dict(zip(self.WALK_STATS, list(a)[:8]))
        d["waves_by_log2_cycles_over_4096"] = list(a)[8:24]
        d["cycles_sum"], d["cycles_max"] = a[24], a[25]
        phases = ("plan_bitmap", "job_list_headers", "operand_arrival", "box", "cull", "exact_rounds", "settle", "rest")
        d["phase_cycles"] = dict(zip(phases, list(a)[26:34]))
        d["waves_of_2e19_cycles_or_more"] = dict(zip(phases + ("waves", "rounds", "jobs", "windows"), list(a)[34:46]))
        return d
