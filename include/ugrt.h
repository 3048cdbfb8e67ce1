/*
 * ugrt.h -- C-ABI of the MI355X-native grid ray tracer (libugrt.so).
 *
 * Drop-in boundary for the render hot path of sushruta/uniformgrid-raytracing.
 * The reference has no FFI; its operator API is the set of C++ methods that
 * display() calls (main.cu:59-302).  Every entry point below names the
 * reference method it replaces (file:line under /root/reference) and keeps the
 * reference's argument ORDER, so a shim class with the reference's method names
 * is a one-liner.
 *
 * Conventions
 *  - plain C, pointers + sizes only; "d_" = device pointer (HIP), everything
 *    else is host memory.  The caller owns what it passes in; the context owns
 *    what it hands out (grid arrays stay valid until the next build of the
 *    same grid or ugrt_ctx_destroy).
 *  - every function returns 0 on success, a UGRT_E* code otherwise, and
 *    ugrt_last_error() describes the failure.  (The reference aborts the
 *    process instead: cutilSafeCall / exit(-1), frustum_grid.h:127-131.)
 *  - all device work is enqueued on the context's stream (ugrt_ctx_set_stream);
 *    functions that must return a host value (the grid builders' total_refs,
 *    ugrt_sort_rays' chunk count) synchronise that stream.
 *  - there is NO CPU fallback: a device entry point fails with UGRT_ENODEV
 *    when no HIP device is usable.
 *  - matrices are OpenGL column-major, indices int32/uint32, geometry fp32,
 *    image uint8 RGB, pixel id = row*width + col with row 0 at the BOTTOM of
 *    the view (trace_kernel.cu:91).
 */
#ifndef UGRT_H
#define UGRT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UGRT_VERSION 105

enum {
	UGRT_OK = 0,
	UGRT_EINVAL = 1, /* bad argument / unsupported configuration */
	UGRT_ENODEV = 2, /* no usable HIP device */
	UGRT_EHIP = 3,   /* a HIP runtime call failed */
	UGRT_EIO = 4,    /* file could not be opened / parsed */
	UGRT_ENOMEM = 5,
	UGRT_EOVERFLOW = 6 /* option "async_build": a call's data-dependent size exceeded the room estimated from the call
			      before; returned by ugrt_ctx_synchronize, the frames since the last one are to be repeated */
};

/* flags in ugrt_config.flags */
enum {
	/* trace every shadow chunk instead of reproducing the reference's launch
	 * (block b handles chunk b-1, at most nbx*nby blocks: light_kernel.cu:76-85,
	 * per_frame_funcs.h:144) */
	UGRT_FLAG_SHADOW_ALL_CHUNKS = 1u,
	/* tracers also count their work (DDA: candidates tested, cells visited, active rays) for
	 * ugrt_stats_get; a counting context is for measurement set-up, never for timing */
	UGRT_FLAG_COUNT_WORK = 2u,
	/* the caller promises that the vertex and face arrays passed to the grid builds only change
	 * through ugrt_animate, or that it calls ugrt_geometry_changed after changing them itself
	 * (the reference's other writer is the per-frame upload of scene.h:70 frames).  The builds then
	 * keep the per-triangle records of the previous build instead of rewriting them three times a
	 * frame.  Without the flag every build assumes new geometry, as the reference does.
	 * The same promise keeps the uniform grid: it has no other input than these arrays, the box and the
	 * context's uniform_dims, so ugrt_grid_build_uniform enqueues nothing while they stand (see there). */
	UGRT_FLAG_STATIC_GEOMETRY = 4u,
	/* ray set-up (trace_kernel.cu:96-105, per_frame_funcs.h:421-433): the reference samples its 5x5 direction
	 * texture through the texture unit's linear filter, whose interpolation weights have 8 fractional bits.  By default
	 * the fetch is the exact float bilinear interpolation at texel coordinate 4 ftx, which has the
	 * same weights k/256 at width and height 1024 and finer ones elsewhere.  With this flag the weights are quantised
	 * as the CUDA programming guide states the rule (ugrt_tex_linear8 in ugrt_fmath.h: coordinate ftx*0.8+0.1 on 5
	 * texels, alpha rounded to 8 fractional bits): identical rays at 1024 x 1024, other rays at 1920 or 3840.  What the
	 * reference's GPU really does beyond the documented rule cannot be checked here: parity unpinned either way. */
	UGRT_FLAG_STRICT_TEXTURE = 8u
};

/* which grid of the context */
enum { UGRT_GRID_PERSPECTIVE = 0, UGRT_GRID_SPHERICAL = 1, UGRT_GRID_UNIFORM = 2 };

/* stages timed by the built-in hipEvent profiler (ugrt_prof_*) */
enum {
	UGRT_ST_BUILD_COUNT = 0, /* DSKernel / DS_spherical_Kernel / uniform count */
	UGRT_ST_BUILD_SCAN,      /* cudppScan inclusive, frustum_grid.h:249 */
	UGRT_ST_BUILD_FILL,      /* DSFillkernel */
	UGRT_ST_BUILD_SORT,      /* cudppSort, frustum_grid.h:298 */
	UGRT_ST_BUILD_BOUNDS,    /* do_scan_dump .. cudppScan exclusive */
	UGRT_ST_TRACE_PRIMARY,   /* rckernel_alpha */
	UGRT_ST_MAP_RAYS,        /* mapSort_Effective_kernel */
	UGRT_ST_SORT_RAYS,       /* processData */
	UGRT_ST_TRACE_SHADOW,    /* mod_light_rckernel: the exact per-ray pass */
	UGRT_ST_SHADE,           /* lambertian_shade / spot_shade / shadow_kernel */
	UGRT_ST_REFLECT_GEN,     /* secondary ray generation (not in reference) */
	UGRT_ST_TRACE_DDA,       /* 3D-DDA traversal (not in reference) */
	UGRT_ST_ANIMATE,         /* copy_data_transform */
	UGRT_ST_WORKLIST,        /* work-item list construction for the tracers */
	UGRT_ST_SHADOW_CULL,     /* shadow tracer's (beam, triangle) cull pass */
	UGRT_ST_SHADOW_PREP,     /* shadow tracer's private re-grouping: ray keys + sort, beams, candidate sort */
	UGRT_ST_COUNT
};

typedef struct ugrt_ctx ugrt_ctx;     /* device context */
typedef struct ugrt_scene ugrt_scene; /* host scene = class Model, scene.h:13-57 */

/* main.cu.h:1-42 turned into run-time parameters */
typedef struct ugrt_config {
	int width, height;       /* SCREEN_WIDTH, SCREEN_HEIGHT; multiples of tile */
	int tile;                /* NUM_THREADS_X = NUM_THREADS_Y; must be 8 */
	int slabs;               /* NUM_SLABS (main.cu.h:18), 1..64: z-slabs of the perspective and the light grid */
	int light_nbx, light_nby; /* spherical light grid, 128 x 128 in the reference; even */
	int row_begin, row_end;  /* tile rows [begin,end) this context renders (multi-GPU band);
				    0, height/tile for the whole image */
	unsigned flags;          /* UGRT_FLAG_* */
	int uniform_dims[3];     /* cells of the uniform (reflection) grid */
} ugrt_config;

/* public members of class Camera, camera.h:19-35, plus the 64-float block of
 * fillCoordinatesData, per_frame_funcs.h:18-39 */
typedef struct ugrt_camera {
	float worldori[4];
	float modelview_matrix[16];
	float projection_matrix[16];
	float mvp_matrix[16];
	float frustum_plane_eq[6][6];
	float frustumcorner[8][3];
	float camcoords[64];
} ugrt_camera;

/* outputs of FrustumGrid, frustum_grid.h:24-29 */
typedef struct ugrt_grid_info {
	unsigned *d_triangle_value_list; /* [total_refs] triangle ids, grouped by cell */
	unsigned *d_triangle_key_list;   /* [total_refs] cell ids, ascending */
	unsigned *d_span;                /* [num_cells] triangles per cell */
	unsigned *d_offset;              /* [num_cells] exclusive scan of d_span */
	unsigned total_refs;             /* "total_triangles", frustum_grid.h:254 */
	unsigned num_cells;
	unsigned cells_used;             /* "Number of actual cells", frustum_grid.h:337; final once the
					    stream has been synchronised after the build */
} ugrt_grid_info;

/* the z-slab stage of FrustumGrid::buildGrid / buildSphericalGrid (NUM_SLABS > 1) */
typedef struct ugrt_slab_info {
	int slabs;
	float *d_proj_coord_z; /* [num_faces] d_projCoordZ: min ndc z (perspective) / min distance from the light
				  (spherical) per triangle, grid_kernel.cu:212,651; NULL when slabs == 1 */
	float z_min, z_max;    /* the host loop's zMin / zMax, frustum_grid.h:221-241 / :384-404 */
} ugrt_slab_info;

/* ---- library ---------------------------------------------------------- */
int ugrt_version(void);
const char *ugrt_last_error(void);

/* ---- host: scene I/O (scene.h, obj_parser/) --------------------------- */
/* new Model(frames), scene.h:59 */
int ugrt_scene_create(ugrt_scene **out);
/* Model::some_material(char*), scene.h:370: positional material token file */
int ugrt_scene_some_material(ugrt_scene *s, const char *file);
/* Model::load_model(char*), scene.h:141 (static branch) -> objLoader::load,
 * obj_parser/objLoader.cpp:5; the mtllib is opened relative to the cwd as in
 * obj_parser.cpp:417 unless it is found next to the .obj first */
int ugrt_scene_load_model(ugrt_scene *s, const char *path);
/* Model::tmp_model(char*, int), scene.h:70: <dir>/f_<i>.obj, vertices only */
int ugrt_scene_load_frame(ugrt_scene *s, const char *dir, int frame);
int ugrt_scene_counts(const ugrt_scene *s, int *num_vertices, int *num_faces, int *num_materials);
const float *ugrt_scene_vertexlist(const ugrt_scene *s);        /* h_vertexlist [3V] */
const int *ugrt_scene_facelist(const ugrt_scene *s);            /* h_facelist [3F] */
const int *ugrt_scene_materiallist_index(const ugrt_scene *s);  /* h_materiallist_index [F] */
const float *ugrt_scene_materiallist(const ugrt_scene *s);      /* h_materiallist [6M] Ka,Kd */
/* obj_material.reflect of the mtllib (obj_parser.h:53, token "r"), [mtl_count] */
const float *ugrt_scene_reflectlist(const ugrt_scene *s, int *mtl_count);
/* How much of a material's colour comes from behind it, [mtl_count]: (float)(1 - obj_material.trans) clamped to [0, 1]
 * (a NaN: 0).  The MTL token "d" is OBJ's dissolve -- 1 is opaque -- and defaults to 1, so a material without it has
 * transmit 0.  A scene loaded from a cache reports 0 for every material: the cache format does not hold the list. */
const float *ugrt_scene_transmitlist(const ugrt_scene *s, int *mtl_count);
/* (float)obj_material.refract_index of the mtllib (token "Ni", default 1), [mtl_count].  A scene loaded from a cache
 * reports 1 for every material: the cache format does not hold the list. */
const float *ugrt_scene_iorlist(const ugrt_scene *s, int *mtl_count);
/* (float)obj_material.glossy of the mtllib (token "sharpness", 0..1000, default 98), raw, [mtl_count]: 1000 is a mirror,
 * and what a lobe's spread is made of is the caller's business (scenes.spread_from_sharpness).  A scene loaded from a
 * cache reports 1000 for every material -- the cache format does not hold the list --, so its reflections stay mirrors. */
const float *ugrt_scene_sharpnesslist(const ugrt_scene *s, int *mtl_count);
/* Texture coordinates and texture names of the loaded OBJ / MTL (obj_parser.cpp:52-104, 281-285, 348-351).
 * ugrt_scene_uvlist: [2T] floats, the first two atof() values of every "vt" line in file order (a missing value is 0, a
 * third one is dropped); *count = T.
 * ugrt_scene_uv_facelist: [3F] ints, one per corner of the face list.  A token "v/t" or "v/t/n" has the texture index
 * atoi() finds behind its first '/', a token "v" or "v//n" has 0; the index is converted like a vertex index against the
 * number of "vt" lines read so far (0: -1, negative: relative to that number, else 1-based to 0-based), and whatever then
 * lies outside 0..T-1 is stored as -1: that face is untextured.  load_model does not fail on such a face.
 * ugrt_scene_texture_name: the texture of material `material` of the mtllib (0..mtl_count-1), "" for none and for a
 * material out of range.  It is the token behind "map_Kd"; where the material has no map_Kd line, the token behind
 * "map_Ka" (the field the reference fills).  Tokens split on " \t"; trailing '\r' and '\n' are stripped.  Options such as
 * "-s" are not supported: a name that starts with '-' makes the material untextured.  The pointer stands until the
 * scene is loaded again or destroyed.
 * ugrt_scene_texture_dir: the directory of the mtllib that was read, with its trailing '/', or "" (the working
 * directory): directory + name is the texture's path.
 * A scene loaded from a cache has no texture coordinate, uv indices of -1 and no texture name: the cache format does not
 * hold them. */
const float *ugrt_scene_uvlist(const ugrt_scene *s, int *count);
const int *ugrt_scene_uv_facelist(const ugrt_scene *s);
const char *ugrt_scene_texture_name(const ugrt_scene *s, int material);
const char *ugrt_scene_texture_dir(const ugrt_scene *s);
/* Binary cache of a loaded scene (the strtok parser takes seconds on 1 M triangles).
 * Little-endian: "UGRTSCN1", counts, then the flat lists exactly as the accessors return them.
 * load_cache replaces the scene's contents; a truncated or foreign file gives UGRT_EIO. */
int ugrt_scene_save_cache(const ugrt_scene *s, const char *path);
int ugrt_scene_load_cache(ugrt_scene *s, const char *path);
/* xMin..zMax, scene.h:43 */
int ugrt_scene_bounds(const ugrt_scene *s, float bbmin[3], float bbmax[3]);
void ugrt_scene_destroy(ugrt_scene *s);

/* ---- host: camera (camera.h) ------------------------------------------ */
/* setCameraCenter/LookAt/Up/setNearFar :13-16 + adjustCameraAndPosition :135 +
 * getGLMatrices :86 + getFrustumProperties :115 + fillCoordinatesData's block.
 * fovy in degrees (FOVY, main.cu.h:14), aspect = width/height. */
int ugrt_camera_set(ugrt_camera *cam, const float eye[3], const float look[3], const float up[3],
		    float near_plane, float far_plane, float fovy, float aspect);
/* the 5x5x4 node table of setDirectionTexture, per_frame_funcs.h:161-419 */
int ugrt_camera_direction_table(const float camcoords[64], float table[100]);

/* writePPM(char*), per_app_funcs.h:39 (returns UGRT_EIO instead of exit(1)) */
int ugrt_write_ppm(const char *path, int width, int height, const unsigned char *rgb);
/* The counterpart of ugrt_write_ppm: reads a P3 (text) or P6 (binary) PPM.  The header is the magic, width, height and
 * maxval, separated by white space, with "# ... end of line" comments anywhere between them; one white-space character
 * follows the maxval of a P6 file.  maxval is 1..255; a sample v of a file whose maxval is below 255 becomes
 * v * 255 / maxval in integers.  *width and *height are set once the header is read; rgb == NULL returns there (the size
 * only).  Otherwise rgb[0 .. 3 * width * height) gets the samples in file order and `capacity` is the room of rgb in bytes.
 * UGRT_EINVAL: path, width or height null.  UGRT_EIO, with a message: the file cannot be opened, is no P3 / P6 file, a
 * dimension outside 1..UGRT_MAX_TEXTURE_DIM, a maxval outside 1..255, a sample above maxval, a file that ends before its
 * last sample, capacity below 3 * width * height.  Nothing outside rgb[0 .. capacity) is written and no allocation is
 * sized by a header value. */
#define UGRT_MAX_TEXTURE_DIM 4096
int ugrt_read_ppm(const char *path, int *width, int *height, unsigned char *rgb, size_t capacity);
/* cosf/sinf of the animation angle as the library evaluates them */
int ugrt_rot_cos_sin(float rot, float *c, float *s);

/* ---- device: context --------------------------------------------------- */
int ugrt_ctx_create(ugrt_ctx **out, int device, const ugrt_config *cfg);
int ugrt_ctx_set_stream(ugrt_ctx *ctx, void *hip_stream);
/* launch-shape options of this context; none changes a result; value < 0 restores the default.  Keys:
 * "dda_kernel" 0 = window kernel (occupancy bitmap, jobs per occupied cell, (survivor, ray) pair rounds),
 * 1 = per-ray kernel of round 1 (kept as the cross-check); "dda_rays_per_wave" 1..64 (0 = default: 32);
 * "dda_cull_min" / "dda_cull_work": a job's list is culled against its ray bundle first from this
 * many triangles / (triangles x rays) on; "dda_coop" (kernel 1) list length from which a lone ray's cell is
 * tested by the whole wave; "dda_sort" 1 = the bounce's ray list sorted by (entry cell, octant) instead of tile
 * order; "dda_split" (window kernel) 1 = the ray groups that were long in the context's last bounce are cut into
 * segments of their walk that run on different waves and are merged per ray (default; the history is kept per pixel,
 * so it serves the next frame of a moving scene as far as it goes), 0 = off, 2..4 = every group is cut (tests);
 * "dda_split_load" a group's jobs, in percent of the average group's, per segment it is cut into (default 400),
 * "dda_split_segments" segments a group is cut into at most (4; 1 = none is cut: the long groups only start first);
 * "primary_seg" triangles per primary work item; "primary_order" 0 = a flush's jobs run in list order
 * (default: nearest triangles first), "primary_chunk" jobs between two looks at the rays' closest hits;
 * "shadow_beam", "shadow_xseg", "shadow_sizebits", "shadow_itemsort", "shadow_mbits", "shadow_key64", "shadow_sieve" shape the
 * shadow tracer's private regrouping; "sort_library" 1 = rocPRIM's radix sort instead of the built-in
 * one; "shadow_pairs" 0 = the shadow tracer sorts the cull pass's (beam, triangle) candidate pairs by (beam, size class)
 * with the radix sort, 1 / default = it counts them per (beam, size class) bucket in the cull pass, scans the counts
 * and places the triangle ids - no sort (the pairs are sorted whatever the option with "sort_library" 1 and where the
 * bucket table, beams x 2^"shadow_sizebits" words, would exceed 4 Mi words);
 * "shadow_frags" 0 = the shadow tracer keys and sorts every ray, 1 / default = where ugrt_sort_rays put its sort off
 * (num_chunks NULL under UGRT_FLAG_SHADOW_ALL_CHUNKS) the rays of an 8x8-pixel tile that share a light cell and a block of direction codes
 * are one sorted item, a fragment (every ray is sorted whatever the option with the sorted map, strict chunks, 64-bit keys,
 * "sort_library" 1 and a band that is not whole 8x8 tiles);
 * "sort_items" 8 / 16 pairs per thread of a radix pass (default: by size), "sort_rank" 0 = the passes rank by
 * ballots instead of LDS atomics, "ray_sort" 1 = the deferred ugrt_sort_rays sorts at once also where nothing needs it
 * (see there); "dda_blocks", "primary_waves",
 * "any_rays_per_wave", "any_coop": ugrt_trace_dda_any (see there);
 * "uniform_reuse" 0 = ugrt_grid_build_uniform builds every time (default 1: it keeps the grid while its inputs stand, see there);
 * "light_reuse" 0 = ugrt_grid_build_spherical builds every time (default 1: it keeps the grid while the light and the geometry stand, see there);
 * "shadow_waves": number of persistent single-wave workgroups of the bounce, the primary tracer and the two
 * shadow kernels (the primary tracer and the exact shadow pass run one wave per work item by default, "primary_xcd_run" /
 * "shadow_xcd_run" neighbouring items per XCD in turn; "primary_waves" set / "shadow_xcd_run" 0 restore their persistent
 * forms; "shadow_waves" is always the cull pass's; "primary_centre" 0 = the primary tracer's runs of items start in
 * list order instead of from the middle of the list outwards).
 * "async_build" 1: the grid builds and ugrt_trace_shadow stop waiting for the device.  The reference reads
 * total_triangles back to size its lists (frustum_grid.h:254); here the second and later builds of a grid size
 * buffers and launches by what the build before needed plus a quarter, every kernel takes the real counts from
 * device memory, and a count that does not fit raises a flag instead of writing out of bounds:
 * ugrt_ctx_synchronize then returns UGRT_EOVERFLOW once (the frames since the last synchronisation are
 * incomplete) and the next calls run in the waiting form again, which sizes everything exactly: every build and
 * shadow pass up to the next ugrt_ctx_synchronize, so that the repeat of a frame which builds a grid or traces shadows
 * more than once (one pass per light) succeeds whatever the passes need.  A pass takes its estimate from the pass
 * before it, which in such a frame is another light's.
 * ugrt_grid_info.total_refs of such a build is final once the stream has been synchronised. */
int ugrt_ctx_set_option(ugrt_ctx *ctx, const char *key, int value);
/* counters and findings of this context (no reference counterpart; the bench line and the tests read them):
 * "radix_launches" histogram + pass kernels of the built-in radix sort enqueued so far, "sort_rank_atomic" 1 = the radix passes rank by LDS
 * atomics (the context's self-test found them served in lane order on this device), 0 = by ballots, -1 = no sort
 * has run yet; "shadow_key_bits" key bits the last ugrt_trace_shadow sorted its rays on (0 = no pass has sorted yet);
 * "shadow_pairs_counted" 1 = the last ugrt_trace_shadow bucketed its candidate pairs by counting, 0 = it sorted them (option "shadow_pairs");
 * "shadow_fragments" fragments the last ugrt_trace_shadow formed (option "shadow_frags"; 0 = it sorted every ray; current once the
 * context has been synchronised);
 * "uniform_builds_reused" ugrt_grid_build_uniform calls so far that kept the grid the context held instead of building;
 * "light_builds_reused" the same for ugrt_grid_build_spherical;
 * "smooth_adjacency_builds" / "smooth_normal_builds" ugrt_smooth_adjacency / ugrt_smooth_corner_normals calls so far that built;
 * "recip_mismatches" runs every float bit pattern through the tracers' short reciprocal on the device and
 * returns the number of operands whose result differs from 1.0f / x (0), "f2i_mismatches" does the same for the device
 * forms of ugrt_f2i / ugrt_f2u / ugrt_floor2i against the portable ones of ugrt_fmath.h (0), "lane_reduce_mismatches"
 * compares the tracers' DPP / permlane-swap reductions with the same reductions by __shfl_xor (0): all three wait for the stream.
 * Unknown key: UGRT_EINVAL. */
int ugrt_ctx_get_state(ugrt_ctx *ctx, const char *key, long long *value);
int ugrt_ctx_synchronize(ugrt_ctx *ctx);
void ugrt_ctx_destroy(ugrt_ctx *ctx);

/* fillCoordinatesData(), per_frame_funcs.h:18: makes `camcoords` the current
 * camera block (dd_camcoords) and rebuilds the direction table (texdir) */
int ugrt_upload_camera(ugrt_ctx *ctx, const float camcoords[64]);
/* updateLightPosition(), per_frame_funcs.h:6: dd_light_position */
int ugrt_set_light_position(ugrt_ctx *ctx, const float pos[3]);

/* ---- device: grid build (frustum_grid.h) ------------------------------- */
/* FrustumGrid::buildGrid(int*, float*), frustum_grid.h:210 */
int ugrt_grid_build_perspective(ugrt_ctx *ctx, const int *d_facelist, const float *d_vertlist, int num_faces);
/* FrustumGrid::buildSphericalGrid(int*, float*, float, float), frustum_grid.h:368: the light grid of the current camera
 * block (ugrt_upload_camera: the light's).  It depends on the triangles, the context's light_nbx / light_nby / slabs, xM,
 * yM and that camera block only -- no pixel camera, no rays, no frame number -- and the reference's light stands still
 * (per_frame_funcs.h:8-10, main.cu:155-166).  The call returns UGRT_OK without enqueuing or changing anything (counted by
 * "light_builds_reused") under the conditions of ugrt_grid_build_uniform below, with xM, yM and the 64 floats of the
 * camera block, bit for bit, in the place of the box.  An asynchronous build is confirmed by a waiting one in the same
 * way; a light that moves every frame, or several lights that take the one light grid in turn, never meet the inputs of
 * the build before and so neither keep anything nor wait.  Option "light_reuse" 0 builds every time. */
int ugrt_grid_build_spherical(ugrt_ctx *ctx, const int *d_facelist, const float *d_vertlist, int num_faces,
			      float xM, float yM);
/* uniform world-space grid for the reflection bounce (README.md:1; no reference code).
 * The grid depends on the triangles, the box and the context's uniform_dims only -- no camera, no light.  The call
 * returns UGRT_OK without enqueuing or changing anything (counted by "uniform_builds_reused") when the grid the context
 * holds is the one it would build: UGRT_FLAG_STATIC_GEOMETRY is set; d_facelist, d_vertlist, num_faces, the face window
 * and the bits of bbmin / bbmax are those of the grid's last build; neither ugrt_animate nor ugrt_geometry_changed has
 * been called since, and no grid build has met arrays the context had not seen; ugrt_grid_merge_shards has not
 * rewritten the grid; no overflow of an asynchronous call is reported or under repair; and that last build waited
 * for its counts.  A build in the asynchronous form ("async_build") is never kept, since one that overflowed its
 * estimate leaves an emptied grid: the next build of the same inputs waits instead, and the calls after it keep that
 * one.  Where the geometry changes every frame nothing waits that did not wait before.  Option "uniform_reuse" 0
 * builds every time.  The arrays handed out by ugrt_grid_get_info are read-only for the caller either way. */
int ugrt_grid_build_uniform(ugrt_ctx *ctx, const int *d_facelist, const float *d_vertlist, int num_faces,
			    const float bbmin[3], const float bbmax[3]);
/* The grid's arrays.  The merged lists exist after this call: a build of the PERSPECTIVE grid that has wide
 * triangles -- triangles whose cell range is the whole band; every cell holds them -- stops behind its spans and
 * offsets (no z slabs, at most 4096 wide triangles; every other build merges at once) and puts off the merge of the
 * sorted narrow references with the wide ids, which only writes the same few hundred ids into every cell.  This call
 * enqueues that merge if it is still pending (it does not wait), and so does ugrt_trace_primary when it is handed this
 * grid's arrays by pointers kept from an earlier call; a frame that traces through ugrt_trace_primary_grid never runs
 * it.  What is handed out is element for element what a build that merges at once writes.  The merge goes onto the
 * context's stream as it is when it is asked for; ugrt_ctx_set_stream waits for the old stream before it switches, so
 * a merge on the new stream still runs behind the build it completes.  With profiling on, its time is booked under
 * the build's bounds stage, whenever it runs. */
int ugrt_grid_get_info(ugrt_ctx *ctx, int which, ugrt_grid_info *out);
/* With slabs > 1 the arrays of ugrt_grid_info hold num_cells = cells * slabs entries, cell-major
 * (key = cell * slabs + slab, grid_kernel.cu:322).  This call synchronises the stream. */
int ugrt_grid_get_slabs(ugrt_ctx *ctx, int which, ugrt_slab_info *out);
/* Sharded build of the light grid and the uniform grid across the GPUs of a node (not in the reference, which
 * has one GPU).  Each rank restricts its builds to a window [begin, end) of the triangle list
 * (end < 0: to the last triangle, so 0, -1 restores the full build; begin == end: an empty shard), the ranks exchange the arrays of their shards
 * (ugrt_grid_get_info: keys, values, span; total_refs entries) and every rank merges them: part r must hold the
 * window of rank r, windows ascending with r and disjoint.  The merged arrays become the context's grid and are
 * element for element those of a full build.  The parts are the caller's buffers, not the context's arrays. */
int ugrt_ctx_set_face_window(ugrt_ctx *ctx, int begin, int end);
int ugrt_grid_merge_shards(ugrt_ctx *ctx, int which, int nparts, const unsigned *const *d_keys,
			   const unsigned *const *d_vals, const unsigned *const *d_span, const unsigned *counts);
/* Two grid builds that depend on the geometry only (a frame's light grid and uniform grid) in shared sort launches:
 * between _begin and _end each ugrt_grid_build_* call of this context enqueues its count, scan and fill and returns;
 * _end sorts the (at most two) reference lists together -- one histogram kernel and one kernel per pass level for
 * both -- and completes the builds.  Results are those of two separate builds.  Only builds in the asynchronous form
 * ("async_build") are deferred; any other is built at once.  The grids of the batch must not be used (traced,
 * queried, waited for by another stream) before _end has returned.  No reference counterpart. */
int ugrt_grid_build_batch_begin(ugrt_ctx *ctx);
int ugrt_grid_build_batch_end(ugrt_ctx *ctx);
/* with UGRT_FLAG_STATIC_GEOMETRY: the vertex or face array was rewritten by the caller */
int ugrt_geometry_changed(ugrt_ctx *ctx);
/* cudppSort(plan, keys, values, bits, n) with CUDPP_SORT_RADIX on (uint key, uint value) pairs
 * (cudpp/cudpp.h:426-471; call sites frustum_grid.h:298, decision_data.h:177): the stable radix sort
 * the builds and the ray sort run on, exposed for callers that drive the stages themselves and for
 * the tests.  Sorts on key bits [0, key_bits); inputs are left untouched; all pointers are device
 * memory, outputs must not alias inputs.  use_library != 0 runs rocPRIM's radix sort instead of the
 * built-in one (same result). */
int ugrt_sort_pairs(ugrt_ctx *ctx, const unsigned *d_keys_in, unsigned *d_keys_out, const unsigned *d_values_in,
		    unsigned *d_values_out, size_t n, int key_bits, int use_library);
/* The built-in radix sort in the forms the frame uses beyond ugrt_sort_pairs: 1 or 2 independent lists in shared
 * launches (one histogram kernel, one kernel per pass level of 8 key bits; a list with fewer passes drops out), a pair
 * count that only the device knows, and a sort in place.  Every argument but ctx is a host array of nlists entries;
 * list j sorts n[j] pairs on key bits [0, key_bits[j]).  d_counts may be NULL; d_counts[j] NULL: n[j] is the count.
 * Otherwise d_counts[j] points at one device word and n[j] is the capacity the launches are sized by: the first
 * min(*d_counts[j], n[j]) outputs are the stable sort of the first min(*d_counts[j], n[j]) inputs and nothing is
 * written behind them.  Inputs are left untouched unless list j is sorted in place: d_keys_in[j] == d_keys_out[j]
 * together with d_values_in[j] == d_values_out[j] is accepted exactly when the list takes 2 or 4 passes (key_bits[j]
 * in 9..16 or 25..32: the input is then read in the first pass only, which writes the context's own buffers).
 * UGRT_EINVAL: nlists outside 1..2, key_bits[j] outside 1..32, a null argument (a list's arrays only with n[j] > 0), an
 * in-place list with 1 or 3 passes, one of a list's two arrays aliased without the other, an output that is another
 * array of the call.  Option "sort_library" does not apply.  No reference counterpart. */
int ugrt_sort_pairs_lists(ugrt_ctx *ctx, int nlists, const unsigned *const *d_keys_in, unsigned *const *d_keys_out,
			  const unsigned *const *d_values_in, unsigned *const *d_values_out, const size_t *n,
			  const int *key_bits, const unsigned *const *d_counts);
/* cudppScan(plan, out, in, n) with CUDPP_ADD on uint (cudpp/cudpp.h:426-471; call sites frustum_grid.h:249 inclusive,
 * frustum_grid.h:361 exclusive, decision_data.h:209): the single-kernel prefix sum the builds and the ray sort run
 * on, sums modulo 2^32, exposed like ugrt_sort_pairs.  inclusive != 0: d_out[i] = d_in[0] + ... + d_in[i], otherwise
 * without d_in[i].  The arrays need no alignment beyond their words' (16-byte accesses are used where both allow them).
 * n == 0 enqueues nothing.  A null argument with n > 0 or d_in == d_out: UGRT_EINVAL. */
int ugrt_scan(ugrt_ctx *ctx, const unsigned *d_in, unsigned *d_out, size_t n, int inclusive);
/* Two scans of n words each, which must not depend on each other, in ONE launch (the first half of the workgroups
 * serves a, the second b).  UGRT_EINVAL as for ugrt_scan, and for d_out_a == d_out_b or an output that is the other
 * scan's input. */
int ugrt_scan_pair(ugrt_ctx *ctx, const unsigned *d_in_a, unsigned *d_out_a, const unsigned *d_in_b, unsigned *d_out_b,
		   size_t n, int inclusive);

/* ---- device: tracing --------------------------------------------------- */
/* FrustumTracer::trace(...), frustum_tracer.h:20-23 -> rckernel_alpha */
int ugrt_trace_primary(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
		       const unsigned *d_offset, float *d_normal, float *d_t_value, float *d_ray_dir,
		       int *d_shadowed, int *d_intersect_id, const float *d_vertlist, const int *d_trilist);
/* The same trace through the context's current perspective grid (ugrt_grid_build_perspective must have run), without
 * asking for its lists: while the build's merge is put off (ugrt_grid_get_info) the tracer reads a cell's run of the
 * sorted narrow references and then the one list of wide triangle ids, and breaks ties between equal distances by
 * triangle id -- inside a cell the ids ascend, so that is the reference's "first in the list wins".  Every output is
 * bit for bit that of ugrt_trace_primary on the merged arrays.  With no merge pending (no wide triangle, z slabs, the
 * lists have been asked for) the call IS ugrt_trace_primary on the grid's arrays.  ugrt_ctx_get_state
 * "primary_deferred_merges" counts the builds that put their merge off, "primary_completed_merges" those of them whose
 * merge was carried out after all, "primary_merge_pending" is 1 while one is put off.  No reference counterpart. */
int ugrt_trace_primary_grid(ugrt_ctx *ctx, float *d_normal, float *d_t_value, float *d_ray_dir, int *d_shadowed,
			    int *d_intersect_id, const float *d_vertlist, const int *d_trilist);
/* getEffectiveRayGridMapping(...), per_frame_funcs.h:97 -> mapSort_Effective_kernel.
 * d_map holds 2n entries, n = pixels of this context's band. */
int ugrt_map_rays_to_light(ugrt_ctx *ctx, const float *d_t_value, const float *d_ray_dir, unsigned *d_map,
			   const float *d_cam_position, float xM, float yM);
/* processData(), per_frame_funcs.h:116: sorts d_map by light cell and writes the
 * chunk start indices; *num_chunks = h_numCudaBlocks (decision_data.h:264).
 * prefix_capacity entries must fit: n/64 + light cells + 1 always does (a smaller map makes the call fail with
 * UGRT_EINVAL; in the deferred form below the shadow tracer then traces nothing and ugrt_sort_rays_chunks reports
 * the error). */
int ugrt_sort_rays(ugrt_ctx *ctx, unsigned *d_map, unsigned *d_prefix_map, unsigned prefix_capacity,
		   unsigned *num_chunks);
/* num_chunks may be NULL: the call then does not wait for the device; the count is passed on to
 * ugrt_trace_shadow as UGRT_CHUNKS_ON_DEVICE and can be fetched later (ugrt_sort_rays_chunks waits for the stream).
 * In a context with UGRT_FLAG_SHADOW_ALL_CHUNKS this deferred form also puts off the SORT: the chunk list only decides
 * which rays the reference's launch traces, with the flag that is every ray, and ugrt_trace_shadow reads the
 * (pixel, light cell) pairs of d_map in any order.  d_map and d_prefix_map are then left as they are until
 * ugrt_sort_rays_chunks is called, which sorts them (they must still hold what ugrt_map_rays_to_light wrote) and
 * returns the count: processData's outputs on demand, two radix passes and five launches less in a frame that never
 * asks.  Option "ray_sort" 1 sorts at once as before. */
int ugrt_sort_rays_chunks(ugrt_ctx *ctx, unsigned *num_chunks);
#define UGRT_CHUNKS_ON_DEVICE 0xFFFFFFFFu
/* check_for_shadows(int), per_frame_funcs.h:139 -> mod_light_rckernel; same
 * argument order as the kernel (light_kernel.cu:53) */
int ugrt_trace_shadow(ugrt_ctx *ctx, const unsigned *d_value_list, const float *d_vertlist,
		      const int *d_trilist, const unsigned *d_span, const unsigned *d_offset,
		      const float *d_t_value, const float *d_ray_dir, int *d_is_shadowed, const unsigned *d_map,
		      const unsigned *d_prefix_map, const float *d_cam_position, unsigned num_chunks);

/* ---- device: shading (shader.h:20-24) ----------------------------------
 * What every float shading call below does with inputs that no traced frame holds (tests/test_shade_synthetic.py runs
 * them all; fp32 denormals are kept in every operation, the comparisons, the square roots and the divisions included):
 * - the id of a pixel is a triangle id or negative.  A negative id is written back as it is, any other as
 *   d_mat_idx[id]; a material index outside 0..num_materials-1 (INT_MAX too) reads no material and is black.
 * - ugrt_shade_spotlight looks at no t; every other call shades a primary hit only where t > 0, which a positive
 *   denormal and +inf are and -0, a negative value and NaN are not.
 * - a colour is Kd/2 + Kd |L.N| where |L.N| > 0, clamped to 1 from above only.  A NaN dot product (the point on the
 *   light, a zero, tiny or NaN normal, a degenerate triangle, a NaN or infinite t) is not > 0: the colour is Kd/2.
 * - a byte is the low 8 bits of ugrt_f2u(colour * 255): 0 for a NaN and for a negative colour.
 * - a level is active where its d_active entry is not 0 (2, -1 and INT_MIN are); only a flag == 1 darkens.
 * - a level that misses (hit id < 0) or whose material is out of range has the colour 0 and leaves k where it was: if
 *   the next level is active all the same, the weight goes on with the k of the last level that had a material.
 * - reflect values are taken as they are (1.5, -0.5, a denormal, NaN); nothing is clamped but the colours. */
int ugrt_shade_simple(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
		      const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
		      const int *d_mat_idx, const float *d_mat_list, int num_materials);
int ugrt_shade_spotlight(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
			 const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
			 const int *d_mat_idx, const float *d_mat_list, int num_materials, float *d_dump);
int ugrt_shade_add_shadows(ugrt_ctx *ctx, unsigned char *d_img, const int *d_is_shadowed);
int ugrt_shade_perlin(ugrt_ctx *ctx, unsigned char *d_img, const float *d_t_value, const float *d_ray_dir,
		      const float *d_cam_position, const int *d_intersect_id);

/* ---- device: several lights ----------------------
 * The reference's frame loops over h_numLights (main.cu:148-203) but runs with one, and its shading kernels index
 * light 0 (shader_kernel.cu:52-56); this is the shading for 1..UGRT_MAX_LIGHTS lights, own spec. */
#define UGRT_MAX_LIGHTS 8
/* ugrt_shade_simple + ugrt_shade_add_shadows once per light and the mean of the results, in one pass.  light_pos is
 * host memory ([3 * num_lights], passed on by value); light l's flags are d_is_shadowed[l * W*H + p], indexed by
 * absolute pixel p as every per-pixel array (the stacking of the reflection levels); d_is_shadowed may be NULL: no
 * light is shadowed.  d_intersect_id is rewritten to material indices as ugrt_shade_simple does.  A pixel whose
 * material index is out of range or whose t is not > 0 is black.  Every other pixel gets, per component,
 * (sum over l of b_l) / num_lights in unsigned integers, where b_l is the byte ugrt_shade_simple would write with
 * light l in place of ugrt_set_light_position's and the context's current camera block, divided by 3 (integer) where
 * light l's flag == 1.  num_lights == 1 gives the bytes of ugrt_shade_simple + ugrt_shade_add_shadows.  Stage
 * UGRT_ST_SHADE.  num_lights outside 1..UGRT_MAX_LIGHTS or a null argument other than d_is_shadowed: UGRT_EINVAL and
 * nothing is enqueued. */
int ugrt_shade_lights(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
		      const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position, const int *d_mat_idx,
		      const float *d_mat_list, int num_materials, int num_lights, const float *light_pos,
		      const int *d_is_shadowed);

/* ---- device: reflection bounce (not in the reference) ---- */
/* secondary rays for hit pixels whose material has reflect > 0 */
/* The domain of the six secondary-ray generators (ugrt_reflect_rays, _reflect_rays_next, _refract_rays,
 * _refract_rays_next, _occlusion_rays, _ao_rays), as tests/test_secondary_rays_synthetic.py pins it against their CPU
 * restatements.  Every pixel of the band gets its six floats and its active word written, 1 with a ray, else six +0 and 0.
 *  - t: a ray leaves only where t > 0.  NaN, +0, -0, negative and -inf t give none; a denormal t gives one; t = +inf
 *    gives one whose origin words are infinite, or NaN where the direction's component is 0.
 *  - ids: a triangle id below 0 gives no ray (ids are triangle ids: the calls run before a shading call rewrites them).
 *    A material index d_mat_idx[id] outside 0..num_materials-1 gives none either, in the calls that ask the material;
 *    ugrt_occlusion_rays and ugrt_ao_rays do not read d_mat_idx.
 *  - d_active (the level forms and ugrt_occlusion_rays): a pixel is live where the word is != 0, whatever else it is
 *    (2, -1, INT_MIN, 0x100); the word written is 0 or 1.
 *  - coefficients: d_reflect[m] and d_transmit[m] count where they are > 0: NaN, -0 and negative values do not, a
 *    denormal and +inf do.  A material with both transmits: d_transmit wins over d_reflect.  d_ior[m] <= 0 or NaN counts
 *    as 1; a denormal index makes 1 / ior infinite (total reflection from the front; from the back eta is next to 0 and
 *    the ray leaves along -n), an infinite one the reverse.
 *  - sides: front = !(d.n > 0) for n = normalize(e1 x e2): an edge-on hit (d.n +0, -0 or NaN) counts as front and the
 *    normal is not turned.  k < 0 alone mirrors: k == 0 exactly refracts.
 *  - a degenerate triangle (zero area, a cross product that under- or overflows, a NaN vertex) still gives an ACTIVE ray:
 *    its words are NaN (or infinite; a normal whose squares overflow is a normal of zeros and leaves the ray at
 *    {P, d}).  So do directions whose squared length is 0 or inf in the refracted ray (u is not finite).  A direction
 *    need not be a unit vector: the reflected ray keeps its length, the refracted one is a unit vector.
 *  - words: -0 and +0 are told apart and are as the formulas give them.  A NaN word's sign and payload are NOT pinned:
 *    two of these calls, or a call and its CPU restatement, agree on which words are NaN and on every other bit. */
int ugrt_reflect_rays(ugrt_ctx *ctx, const float *d_cam_position, const float *d_t_value,
		      const float *d_ray_dir, const int *d_intersect_id, const int *d_mat_idx,
		      const float *d_reflect, int num_materials, const float *d_vertlist, const int *d_trilist,
		      float eps, float *d_rays, int *d_active);
/* Amanatides-Woo traversal of the context's uniform grid.  d_rays holds {origin, direction} per pixel; a direction need
 * not be a unit vector: any finite length is taken for which the Moller-Trumbore determinants of the ray against the
 * scene's triangles (d.(e2 x e1), d.(e2 x tvec), d.(tvec x e1)) stay below 1e15 in magnitude, and d_hit_t is the
 * parameter along the direction as given.  The closest hit is the one the exact float test finds over the cells the
 * ray walks: the window kernel's bundle cull only decides which exact tests run, and its margins follow the length of
 * the directions (csrc/ugrt_dda.h). */
int ugrt_trace_dda(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
		   const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
		   const float *d_rays, const int *d_active, float *d_hit_t, int *d_hit_id);
/* lambertian_shade + blend (1-k)*local + k*reflected */
int ugrt_shade_reflect(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
		       const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
		       const int *d_mat_idx, const float *d_mat_list, const float *d_reflect, int num_materials,
		       const float *d_vertlist, const int *d_trilist, const float *d_rays, const int *d_active,
		       const float *d_hit_t, const int *d_hit_id);

/* ---- device: reflections of depth D ----------------
 * Level 1 is ugrt_reflect_rays + ugrt_trace_dda.  Level j+1 (j >= 1) is ugrt_reflect_rays_next from level j's
 * hits + ugrt_trace_dda.  The D levels of a frame lie one behind the other: level j's rays at (j-1)*W*H*6 floats,
 * its active / hit_t / hit_id at (j-1)*W*H entries, each indexed by absolute pixel p = p0 + i as every per-pixel
 * array of the frame; the caller sizes them for `depth` levels. */
#define UGRT_MAX_REFLECT_DEPTH 8
/* The next reflected rays from one level's hits, for the context's band: for a pixel with d_active[p],
 * d_hit_t[p] > 0, d_hit_id[p] >= 0 and d_reflect[d_mat_idx[d_hit_id[p]]] > 0 (material in range), P = o + t*d,
 * n = normalize(e1 x e2) turned so that d.n <= 0, ray {P + eps*n, d - 2(d.n)n} and d_active_next[p] = 1 (the
 * arithmetic of ugrt_reflect_rays with the ray's own origin: fed with rays = {cam, dir}, d_active all ones and the
 * primary t and ids it writes ugrt_reflect_rays' words); every other pixel: six zeros and 0.  d_active[p] counts where it
 * is != 0; t, ids, materials, edge-on hits and degenerate triangles as said in front of ugrt_reflect_rays.  Stage
 * UGRT_ST_REFLECT_GEN.  The ugrt_trace_dda that follows on the same context walks without the split-walk history
 * (option "dda_split"), which stays that of the level-1 launches (ugrt_reflect_rays); results do not change. */
int ugrt_reflect_rays_next(ugrt_ctx *ctx, const float *d_rays, const int *d_active, const float *d_hit_t,
			   const int *d_hit_id, const int *d_mat_idx, const float *d_reflect, int num_materials,
			   const float *d_vertlist, const int *d_trilist, float eps, float *d_rays_next,
			   int *d_active_next);
/* Lambertian shading blended over `depth` (1..UGRT_MAX_REFLECT_DEPTH) reflection levels, d_rays / d_active /
 * d_hit_t / d_hit_id holding levels 1..depth stacked as above.  Front to back from acc = 0, w = 1: a level L_j
 * (clamped Lambert colour of its hit, 0 on a miss) whose pixel goes on to level j+1 adds (w*(1-k_j))*L_j and sets
 * w = w*k_j (k_j: reflect of its material); the first level that does not go on (level depth at the latest) adds
 * w*L_j.  depth 1 gives ugrt_shade_reflect's image byte for byte.  d_intersect_id is rewritten to material indices
 * as ugrt_shade_reflect does.  Stage UGRT_ST_SHADE.  A depth outside 1..8 or a null argument: UGRT_EINVAL. */
int ugrt_shade_reflect_depth(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
			     const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
			     const int *d_mat_idx, const float *d_mat_list, const float *d_reflect,
			     int num_materials, const float *d_vertlist, const int *d_trilist, int depth,
			     const float *d_rays, const int *d_active, const float *d_hit_t, const int *d_hit_id);

/* ---- device: shadows on reflected hits -----------
 * The hits of the reflection levels 1..D are tested against the light: per level ugrt_occlusion_rays +
 * ugrt_trace_dda_any behind the level's ugrt_trace_dda, then ugrt_shade_reflect_depth_occluded instead of
 * ugrt_shade_reflect_depth.  The occlusion flags of the levels are stacked like d_active. */
/* Occlusion rays from one level's hits, for the context's band: for a pixel with d_active[p], d_hit_t[p] > 0 and
 * d_hit_id[p] >= 0 (whatever the hit's material), o' = the origin ugrt_reflect_rays_next gives the next ray
 * (P = o + t*d, n = normalize(e1 x e2) turned so that d.n <= 0, o' = P + eps*n), ray {o', light_pos - o'} (not
 * normalised: the light lies at t = 1) and d_oactive[p] = 1; every other pixel: six zeros and 0.  d_active[p] counts
 * where it is != 0; t, ids, edge-on hits and degenerate triangles as said in front of ugrt_reflect_rays.  A light on o'
 * gives a direction of three +0 words, an infinite light coordinate an infinite direction word.  light_pos is host
 * memory and is passed on by value.  Stage UGRT_ST_REFLECT_GEN.  Unlike ugrt_reflect_rays_next the call says nothing
 * to the ugrt_trace_dda that follows. */
int ugrt_occlusion_rays(ugrt_ctx *ctx, const float *d_rays, const int *d_active, const float *d_hit_t,
			const int *d_hit_id, const float *d_vertlist, const int *d_trilist, const float light_pos[3],
			float eps, float *d_orays, int *d_oactive);
/* Any-hit traversal of the context's uniform grid: d_occluded[p] = 1 for an active pixel of the band iff a triangle
 * in the list of a VISITED cell passes ugrt_trace_dda's exact test with 0 < t < t_max (both strict), else 0.  The
 * visited cells are those of ugrt_trace_dda's walk (same clip, entry cell, stepping and guard), from the entry cell on
 * for as long as a cell's entry parameter -- the entry into the grid, then the exit parameter of the cell before -- is
 * below t_max; a hit need not lie inside the cell whose list holds it.  Inactive pixels of the band get 0, pixels
 * outside it are not written.  t_max <= 0 or NaN, or a null argument: UGRT_EINVAL; without a built uniform grid the
 * error of ugrt_trace_dda.  Options "any_rays_per_wave" 1..64 (0 = default: 32) and "any_coop" (list length from which
 * a ray's cell is tested by the whole wave, default 8) shape the launch, "dda_blocks" caps its waves; none changes a
 * result.  Stages UGRT_ST_WORKLIST / UGRT_ST_TRACE_DDA.  The call leaves the split-walk history of ugrt_trace_dda
 * (option "dda_split") and what ugrt_reflect_rays_next told it alone. */
int ugrt_trace_dda_any(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
		       const unsigned *d_offset, const float *d_vertlist, const int *d_trilist, const float *d_rays,
		       const int *d_active, float t_max, int *d_occluded);
/* ugrt_shade_reflect_depth with shadowed levels: where d_occluded (levels 1..depth stacked like d_active) is 1, the
 * clamped colour L_j of level j >= 1 becomes L_j / 3.0f per component before the level is weighted.  The primary
 * level and ugrt_shade_add_shadows are untouched; with d_occluded all zero the image is ugrt_shade_reflect_depth's
 * byte for byte.  A null d_occluded: UGRT_EINVAL. */
int ugrt_shade_reflect_depth_occluded(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal,
				      const float *d_t_value, const float *d_ray_dir, int *d_intersect_id,
				      const float *d_cam_position, const int *d_mat_idx, const float *d_mat_list,
				      const float *d_reflect, int num_materials, const float *d_vertlist,
				      const int *d_trilist, int depth, const float *d_rays, const int *d_active,
				      const float *d_hit_t, const int *d_hit_id, const int *d_occluded);

/* ---- device: reflections under several lights -----
 * Sections 6.1-6.3 composed: the hits of the reflection levels are tested against every light in one launch per level,
 * and one shading pass blends the levels under every light and averages the lights.  Per level: ugrt_trace_dda, ONE
 * ugrt_occlusion_rays (with any light: only the origins are used), ugrt_trace_dda_any_lights; then
 * ugrt_shade_reflect_lights. */
/* The any-hit walk towards num_lights (1..UGRT_MAX_LIGHTS) points from one set of origins: for light l and pixel p of
 * the band, d_occluded[l * W*H + p] is exactly what ugrt_trace_dda_any(..., t_max = 1) writes for the rays
 * {o, light_pos[l] - o} (the subtraction per component in fp32, as ugrt_occlusion_rays forms it), o = the first three
 * floats of d_orays[6 * p]; the last three are not read.  light_pos is host memory ([3 * num_lights], passed on by
 * value).  Inactive pixels of the band get 0 in all num_lights layers; pixels outside the band and layers >= num_lights
 * are not written.  One prepare launch and one ray list serve all lights; a wave's rays all walk towards one light.
 * Options "any_rays_per_wave", "any_coop" and "dda_blocks" shape the launch as they shape ugrt_trace_dda_any's and
 * change no result.  Stages UGRT_ST_WORKLIST / UGRT_ST_TRACE_DDA.  The call leaves the split-walk history of
 * ugrt_trace_dda and what ugrt_reflect_rays_next told it alone.  num_lights out of range or a null argument:
 * UGRT_EINVAL and nothing is enqueued; without a built uniform grid the error of ugrt_trace_dda. */
int ugrt_trace_dda_any_lights(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
			      const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
			      const float *d_orays, const int *d_oactive, int num_lights, const float *light_pos,
			      int *d_occluded);
/* ugrt_shade_reflect_depth_occluded + ugrt_shade_add_shadows once per light and the mean of the results, in one pass.
 * light_pos is host memory ([3 * num_lights], passed on by value); light l's primary shadow flags are
 * d_is_shadowed[l * W*H + p] (may be NULL: no light is shadowed), the occlusion flag of level j (1..depth) and light l
 * is d_occluded[((j-1) * num_lights + l) * W*H + p] (may be NULL: nothing is occluded).  d_intersect_id is rewritten to
 * material indices as ugrt_shade_reflect_depth does; a pixel whose material index is out of range is black.  Every
 * other pixel walks its level chain once (it does not depend on the light); light l has its own accumulator, which
 * receives ugrt_shade_reflect_depth's operations in its order with the levels' colours taken under light_pos[l]
 * (clamped to 1; for j >= 1 divided by 3.0f where the flag == 1); b_l = its byte, divided by 3 (integer) where
 * d_is_shadowed[l] == 1; the component is (sum over l of b_l) / num_lights in unsigned integers.  num_lights == 1 with
 * ugrt_set_light_position's position gives the bytes of ugrt_shade_reflect_depth_occluded + ugrt_shade_add_shadows
 * (d_occluded NULL: of ugrt_shade_reflect_depth); a frame without an active level-1 ray gives ugrt_shade_lights'.
 * Stage UGRT_ST_SHADE.  depth outside 1..UGRT_MAX_REFLECT_DEPTH, num_lights outside 1..UGRT_MAX_LIGHTS or a null
 * argument other than the two flag arrays: UGRT_EINVAL and nothing is enqueued. */
int ugrt_shade_reflect_lights(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
			      const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
			      const int *d_mat_idx, const float *d_mat_list, const float *d_reflect, int num_materials,
			      const float *d_vertlist, const int *d_trilist, int depth, const float *d_rays,
			      const int *d_active, const float *d_hit_t, const int *d_hit_id, int num_lights,
			      const float *light_pos, const int *d_is_shadowed, const int *d_occluded);

/* ---- device: ambient occlusion --------------------
 * How enclosed a primary hit is: num_dirs short rays over the hemisphere of its normal, walked through the uniform grid
 * with the any-hit walk of section 6.2, and a last integer pass that scales the image by the share of open rays.  Per
 * frame: ugrt_ao_rays + ugrt_trace_dda_any_hemi before the shading call that rewrites the ids, ugrt_shade_ao behind the
 * shading (and ugrt_shade_add_shadows).  All arithmetic is fp32 without contraction. */
#define UGRT_MAX_AO_DIRS 32
/* The hemisphere's origins and normals from the primary hits, for the context's band; the primary arrays are read as
 * ugrt_reflect_rays reads them (triangle ids: before any shading call).  For a pixel with d_t_value[p] > 0 and
 * d_intersect_id[p] >= 0, whatever its material: d_orays[6 * p ..] = {o', n} and d_oactive[p] = 1, with
 * P = cam + t*d, n = normalize(e1 x e2) turned so that d.n <= 0 and o' = P + eps*n (the origin and the flipped normal of
 * ugrt_reflect_rays with d_reflect all 1); every other pixel: six zeros and 0.  t, ids, edge-on hits (the normal is not
 * turned) and degenerate triangles (an active pixel with NaN words) as said in front of ugrt_reflect_rays.  Stage
 * UGRT_ST_REFLECT_GEN.  The call says nothing to the ugrt_trace_dda that follows.  A null argument: UGRT_EINVAL. */
int ugrt_ao_rays(ugrt_ctx *ctx, const float *d_cam_position, const float *d_t_value, const float *d_ray_dir,
		 const int *d_intersect_id, const float *d_vertlist, const int *d_trilist, float eps, float *d_orays,
		 int *d_oactive);
/* The any-hit walk along num_dirs (1..UGRT_MAX_AO_DIRS) directions of the hemisphere over each stored normal: for an
 * active pixel p of the band, bit s of d_mask[p] is exactly what ugrt_trace_dda_any(..., t_max = radius) writes for the
 * ray {o, D_s}; o = floats 0..2 and n = floats 3..5 of d_orays[6 * p].  dirs is host memory ([3 * num_dirs], passed on by
 * value): local directions (x_s, y_s, z_s) with z along the normal.  The basis: a = the index of the smallest |n[k]|
 * (strict <, 1 against 0, then 2 against the winner: ties go to the lowest k); u = n x e_a, i.e. (0, n2, -n1),
 * (-n2, 0, n0) or (n1, -n0, 0); T = u * (1 / sqrt(u0*u0 + u1*u1 + u2*u2)); B = n x T, each component n_i*T_j - n_j*T_i;
 * D_s[k] = (x_s*T[k] + y_s*B[k]) + z_s*n[k].  Directions are not normalised: radius is measured in units of |D_s|.  Bits
 * >= num_dirs are 0, inactive pixels of the band get 0, pixels outside the band are not written.  One prepare launch
 * and one ray list serve all directions; a wave's rays all walk along one local direction; the directions are formed in
 * registers and never stored.  Options "any_rays_per_wave", "any_coop" and "dda_blocks" shape the launch as they shape
 * ugrt_trace_dda_any's and change no result.  Stages UGRT_ST_WORKLIST / UGRT_ST_TRACE_DDA.  The call leaves the split-walk
 * history of ugrt_trace_dda and what ugrt_reflect_rays_next told it alone.  num_dirs out of range, radius <= 0 or NaN, or
 * a null argument: UGRT_EINVAL and nothing is enqueued; without a built uniform grid the error of ugrt_trace_dda. */
int ugrt_trace_dda_any_hemi(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
			    const unsigned *d_offset, const float *d_vertlist, const int *d_trilist, const float *d_orays,
			    const int *d_oactive, int num_dirs, const float *dirs, float radius, unsigned *d_mask);
/* The image scaled by the share of open hemisphere rays, for the context's band: open = num_dirs - popcount(d_mask[p] &
 * the low num_dirs bits), and each of the pixel's three bytes b becomes (b * open) / num_dirs in unsigned 32-bit
 * integers.  A zero mask leaves the pixel as it is.  Stage UGRT_ST_SHADE.  num_dirs outside 1..UGRT_MAX_AO_DIRS or a null
 * argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_shade_ao(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_mask, int num_dirs);

/* ---- device: refraction ---------------------------
 * Transmitted rays in the bounce chain: a level's ray goes THROUGH a hit whose material has transmit > 0 instead of
 * being mirrored, and the any-hit walk of section 6.2 does not count such a material's triangles as occluders.  The
 * levels, ugrt_trace_dda and every shading call are those of sections 6.1-6.5; the shading calls are given
 * continue[m] = transmit[m] > 0 ? transmit[m] : reflect[m] as their d_reflect.  All arithmetic is fp32 without
 * contraction, sqrt and / correctly rounded.
 * The refracted ray of a hit (o, d, t, triangle) of material m: P = o + t*d, n = normalize(e1 x e2), front = d.n <= 0,
 * n turned so that d.n <= 0 (the frame of ugrt_reflect_rays_next); u = d * (1 / sqrt(d.d)), c = -(u.n);
 * ior = ior[m] > 0 ? ior[m] : 1 (a NaN or a non-positive index counts as 1); eta = front ? 1 / ior : ior;
 * k = 1 - (eta*eta) * (1 - c*c).  k < 0 (total internal reflection): the ray of ugrt_reflect_rays_next,
 * {P + eps*n, d - (2*(d.n))*n}.  Otherwise g = eta*c - sqrt(k) and the ray is {P - eps*n, eta*u + g*n}: it starts on
 * the far side.  Which side is the front rests on the winding of the scene's closed solids (outwards); it is not
 * tracked per ray. */
/* ugrt_reflect_rays with glass: under ugrt_reflect_rays' conditions on the pixel (d_t_value[p] > 0, d_intersect_id[p] >= 0,
 * material m in range), d_transmit[m] > 0: the refracted ray above from the camera and active 1; else d_reflect[m] > 0:
 * ugrt_reflect_rays' ray and 1; else six zeros and 0.  A material with both transmits; a NaN in one of the two leaves
 * the decision to the other.  With d_transmit all zero the call writes ugrt_reflect_rays' words (a NaN word where that
 * call writes a NaN word; its sign is not pinned).  The domain is said in front of ugrt_reflect_rays.  It tells the context what ugrt_reflect_rays tells it (level 1: the
 * ugrt_trace_dda that follows uses the split-walk history).  Stage UGRT_ST_REFLECT_GEN.  A null argument: UGRT_EINVAL
 * and nothing is enqueued. */
int ugrt_refract_rays(ugrt_ctx *ctx, const float *d_cam_position, const float *d_t_value, const float *d_ray_dir,
		      const int *d_intersect_id, const int *d_mat_idx, const float *d_reflect, const float *d_transmit,
		      const float *d_ior, int num_materials, const float *d_vertlist, const int *d_trilist, float eps,
		      float *d_rays, int *d_active);
/* ugrt_reflect_rays_next with glass, in the same way: for a pixel with d_active[p], d_hit_t[p] > 0, d_hit_id[p] >= 0
 * and material m in range, d_transmit[m] > 0 gives the refracted ray from the ray's own origin, else d_reflect[m] > 0
 * the reflected one, else six zeros and 0.  With d_transmit all zero the call writes ugrt_reflect_rays_next's words (NaN
 * words as NaN words), and fed with rays = {cam, dir} and d_active all ones it writes ugrt_refract_rays' words.
 * It tells the context what ugrt_reflect_rays_next tells it (the ugrt_trace_dda that follows walks without the
 * split-walk history).  Stage UGRT_ST_REFLECT_GEN.  A null argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_refract_rays_next(ugrt_ctx *ctx, const float *d_rays, const int *d_active, const float *d_hit_t,
			   const int *d_hit_id, const int *d_mat_idx, const float *d_reflect, const float *d_transmit,
			   const float *d_ior, int num_materials, const float *d_vertlist, const int *d_trilist, float eps,
			   float *d_rays_next, int *d_active_next);
/* ugrt_trace_dda_any that sees through glass: a triangle f of a visited cell's list occludes iff it passes
 * ugrt_trace_dda_any's test (exact test, 0 < t < t_max) AND it is not see-through; f is see-through when
 * m = d_mat_idx[f] is in 0..num_materials-1 and d_transmit[m] > 0.  The two loads happen only behind a geometrically
 * accepted test.  Everything else -- visited cells, result layout, prepare launch, ticket, bitmap, options, stages,
 * errors, leaving the split-walk history alone -- is ugrt_trace_dda_any's; with d_transmit all zero the call writes
 * what ugrt_trace_dda_any writes.  A null d_mat_idx or d_transmit: UGRT_EINVAL and nothing is enqueued. */
int ugrt_trace_dda_any_thru(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
			    const unsigned *d_offset, const float *d_vertlist, const int *d_trilist, const float *d_rays,
			    const int *d_active, float t_max, int *d_occluded, const int *d_mat_idx,
			    const float *d_transmit, int num_materials);
/* ugrt_trace_dda_any_lights that sees through glass, in the same way: layer l is what ugrt_trace_dda_any_thru(...,
 * t_max = 1) writes for the rays towards light_pos[l].  With d_transmit all zero the call writes what
 * ugrt_trace_dda_any_lights writes.  (The hemisphere walk of section 6.5 has no such form: glass does enclose.) */
int ugrt_trace_dda_any_lights_thru(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				   const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				   const float *d_orays, const int *d_oactive, int num_lights, const float *light_pos,
				   int *d_occluded, const int *d_mat_idx, const float *d_transmit, int num_materials);

/* ---- device: area lights ---------------------------
 * Soft shadows: num_samples shadow rays per primary hit towards num_samples points of a light's disk, carried by one
 * any-hit walk of section 6.2 through the uniform grid, one mask word per pixel, and a last integer pass that turns the
 * share of lit samples into a penumbra.  Per frame: ugrt_ao_rays (the origins) + ugrt_trace_dda_any_area before the
 * shading call that rewrites the ids, ugrt_shade_area behind the shading, in the place of ugrt_shade_add_shadows.  All
 * arithmetic is fp32 without contraction. */
#define UGRT_MAX_AREA_SAMPLES 32
/* The any-hit walk towards num_samples (1..UGRT_MAX_AREA_SAMPLES) points from each stored origin: for an active pixel
 * p of the band, bit s of d_mask[p] is exactly what ugrt_trace_dda_any(..., t_max = 1) writes for the ray
 * {o, sample_pos[s] - o}; o = floats 0..2 of d_orays[6 * p] (what ugrt_ao_rays writes; floats 3..5 are not read), the
 * subtraction per component in fp32 as ugrt_occlusion_rays forms it: the sample lies at t = 1.  sample_pos is host
 * memory ([3 * num_samples], world positions, passed on by value).  Bits >= num_samples are 0, inactive pixels of the
 * band get 0, pixels outside the band are not written; for num_samples <= UGRT_MAX_LIGHTS bit s equals layer s of
 * ugrt_trace_dda_any_lights on the same origins.  The index space is (pixel group, sample): the num_samples rays of a
 * pixel sit in neighbouring lanes of one wave, which writes the pixel's word whole, with one store.  One prepare launch
 * and one ray list serve the call; it clears the band's words.  Options "any_rays_per_wave" (the lanes of a wave that
 * are given rays; unset: 64), "any_coop" and "dda_blocks" shape the launch and change no result.  Stages
 * UGRT_ST_WORKLIST / UGRT_ST_TRACE_DDA.  The call leaves the split-walk history of ugrt_trace_dda and what
 * ugrt_reflect_rays_next told it alone.  num_samples out of range or a null argument: UGRT_EINVAL and nothing is
 * enqueued; without a built uniform grid the error of ugrt_trace_dda. */
int ugrt_trace_dda_any_area(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
			    const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
			    const float *d_orays, const int *d_oactive, int num_samples, const float *sample_pos,
			    unsigned *d_mask);
/* ugrt_trace_dda_any_area that sees through glass: the rule of ugrt_trace_dda_any_thru and nothing else (a triangle
 * whose material is in range and has transmit > 0 does not occlude; the two loads happen only behind a geometrically
 * accepted test).  With d_transmit all zero the call writes ugrt_trace_dda_any_area's words.  A null d_mat_idx or
 * d_transmit: UGRT_EINVAL and nothing is enqueued. */
int ugrt_trace_dda_any_area_thru(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				 const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				 const float *d_orays, const int *d_oactive, int num_samples, const float *sample_pos,
				 unsigned *d_mask, const int *d_mat_idx, const float *d_transmit, int num_materials);
/* The penumbra, for the context's band: lit = num_samples - popcount(d_mask[p] & the low num_samples bits), and each of
 * the pixel's three bytes b becomes (b * (num_samples + 2 * lit)) / (3 * num_samples) in unsigned 32-bit integers.  A
 * zero mask leaves the pixel as it is, a full one gives b / 3, the byte of ugrt_shade_add_shadows (num_samples = 1 is
 * ugrt_shade_add_shadows with the flag in bit 0).  Stage UGRT_ST_SHADE.  num_samples outside
 * 1..UGRT_MAX_AREA_SAMPLES or a null argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_shade_area(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_mask, int num_samples);

/* ---- device: interleaved sample sets and the edge-aware gather ----
 * Neighbouring pixels aim at different sample sets of the light's disk, and a small gather over pixels of the same
 * surface averages their masks: with a 4x4 tile of sets and a 5x5 gather a pixel sees 16 * num_samples points of the
 * light for num_samples rays and one image pass.  Per frame: ugrt_trace_dda_any_area_sets in the place of
 * ugrt_trace_dda_any_area, ugrt_filter_visibility + ugrt_shade_area_vis in the place of ugrt_shade_area.  All arithmetic
 * is fp32 without contraction or unsigned 32-bit integer. */
#define UGRT_MAX_AREA_SET_TILE 4     /* set_w, set_h */
#define UGRT_MAX_AREA_SET_POINTS 512 /* set_w * set_h * num_samples */
#define UGRT_MAX_FILTER_RADIUS 8
/* ugrt_trace_dda_any_area with one sample set per pixel of a set_w x set_h tile: pixel p of the band has the full-image
 * coordinates x = p % width, y = p / width and the set k(p) = (y % set_h) * set_w + (x % set_w); bit s of d_mask[p] is
 * exactly what ugrt_trace_dda_any(..., t_max = 1) writes for the ray {o, d_sample_pos[3 * (k(p) * num_samples + s) ..] - o}.
 * d_sample_pos is DEVICE memory, [set_w * set_h][num_samples][3] floats (the by-value argument block cannot hold it);
 * every workgroup copies it to LDS once.  Everything else -- bits >= num_samples, inactive pixels, pixels outside the
 * band, the prepare launch, the ticket, the bitmap, the options, the stages, leaving the split-walk history alone -- is
 * ugrt_trace_dda_any_area's, and with set_w = set_h = 1 the call writes that call's words.  set_w or set_h outside
 * 1..UGRT_MAX_AREA_SET_TILE, num_samples outside 1..UGRT_MAX_AREA_SAMPLES, set_w * set_h * num_samples >
 * UGRT_MAX_AREA_SET_POINTS or a null argument: UGRT_EINVAL (the message names the argument) and nothing is enqueued. */
int ugrt_trace_dda_any_area_sets(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				 const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				 const float *d_orays, const int *d_oactive, int num_samples, int set_w, int set_h,
				 const float *d_sample_pos, unsigned *d_mask);
/* ugrt_trace_dda_any_area_sets that sees through glass: the rule of ugrt_trace_dda_any_thru and nothing else. */
int ugrt_trace_dda_any_area_sets_thru(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				      const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				      const float *d_orays, const int *d_oactive, int num_samples, int set_w, int set_h,
				      const float *d_sample_pos, unsigned *d_mask, const int *d_mat_idx,
				      const float *d_transmit, int num_materials);
/* The gather over mask words.  d_orays / d_oactive are what ugrt_ao_rays wrote ({o, n} per pixel); radius R is
 * 0..UGRT_MAX_FILTER_RADIUS, num_bits S 1..32, d_vis unsigned [2 * width * height].  For an active pixel p = (x, y) of
 * the band the sums run over q = (x + dx, y + dy), |dx|, |dy| <= R, q inside the image, inside the band's rows and
 * active; q counts when it is p itself, or when (n_p0*n_q0 + n_p1*n_q1) + n_p2*n_q2 >= normal_cos and
 * |(d0*n_p0 + d1*n_p1) + d2*n_p2| <= plane_tol with d = o_q - o_p per component (a comparison with a NaN rejects q).
 * With w = (R + 1 - |dx|) * (R + 1 - |dy|) and open_q = S - popcount(d_mask[q] & the low S bits):
 * d_vis[2p] = sum of w * open_q, d_vis[2p + 1] = sum of w (at most 32 * 6561 and 6561).  Inactive pixels of the band
 * get (0, 0), pixels outside the band are not written.  Stage UGRT_ST_SHADE.  radius or num_bits out of range, a
 * plane_tol that is negative or a NaN, or a null argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_filter_visibility(ugrt_ctx *ctx, const unsigned *d_mask, int num_bits, const float *d_orays,
			   const int *d_oactive, int radius, float normal_cos, float plane_tol, unsigned *d_vis);
/* The penumbra from the gathered sums, for the context's band: with num = d_vis[2p] and den = d_vis[2p + 1] != 0 each
 * of the pixel's three bytes b becomes (b * (num_samples * den + 2 * num)) / (3 * num_samples * den) in unsigned 32-bit
 * integers (the largest product is 255 * 3 * 32 * 6561); den = 0 leaves the pixel as it is.  Behind a gather of
 * radius 0 the bytes are ugrt_shade_area's.  Stage UGRT_ST_SHADE.  num_samples outside 1..UGRT_MAX_AREA_SAMPLES or a
 * null argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_shade_area_vis(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_vis, int num_samples);

/* ---- device: ambient occlusion over interleaved direction sets ----
 * Section 6.8's two means for the hemisphere rays of section 6.5: neighbouring pixels walk along different sets of local
 * directions, and ugrt_filter_visibility, fed with the hemisphere masks, averages them over pixels of the same surface.
 * Per frame: ugrt_trace_dda_any_hemi_sets in the place of ugrt_trace_dda_any_hemi, ugrt_filter_visibility +
 * ugrt_ao_shade_vis in the place of ugrt_shade_ao.  All arithmetic is fp32 without contraction or unsigned 32-bit
 * integer. */
#define UGRT_MAX_AO_SET_TILE 4   /* set_w, set_h */
#define UGRT_MAX_AO_SET_DIRS 512 /* set_w * set_h * num_dirs */
/* ugrt_trace_dda_any_hemi with one set of directions per pixel of a set_w x set_h tile, in ugrt_trace_dda_any_area's
 * index space: pixel p of the band has the full-image coordinates x = p % width, y = p / width and the set
 * k(p) = (y % set_h) * set_w + (x % set_w); for an active pixel bit s of d_mask[p] is exactly what
 * ugrt_trace_dda_any(..., t_max = radius) writes for the ray {o, D}, o = floats 0..2 and n = floats 3..5 of
 * d_orays[6 * p], D = ugrt_trace_dda_any_hemi's D_s formed from the local direction d_dirs[3 * (k(p) * num_dirs + s) ..]
 * with the same basis rule and the same operation order.  d_dirs is DEVICE memory, [set_w * set_h][num_dirs][3] floats
 * (local directions, z along the normal); every workgroup copies it to LDS once.  Bits >= num_dirs are 0, inactive
 * pixels of the band get 0, pixels outside the band are not written.  The index space is (pixel group, direction): the
 * num_dirs rays of a pixel sit in neighbouring lanes of one wave, which writes the pixel's word whole, with one store and
 * no atomic operation.  One prepare launch and one ray list serve the call; it clears the band's words.  Options
 * "any_rays_per_wave" (the lanes of a wave that are given rays; unset: 64), "any_coop" and "dda_blocks" shape the launch
 * and change no result.  Stages UGRT_ST_WORKLIST / UGRT_ST_TRACE_DDA.  The call leaves the split-walk history of
 * ugrt_trace_dda and what ugrt_reflect_rays_next told it alone.  With set_w = set_h = 1 the words are
 * ugrt_trace_dda_any_hemi's for the same directions.  There is no see-through form (glass does enclose).  num_dirs
 * outside 1..UGRT_MAX_AO_DIRS, set_w or set_h outside 1..UGRT_MAX_AO_SET_TILE, set_w * set_h * num_dirs >
 * UGRT_MAX_AO_SET_DIRS, radius <= 0 or NaN, or a null argument: UGRT_EINVAL (the message names the argument) and nothing
 * is enqueued; without a built uniform grid the error of ugrt_trace_dda. */
int ugrt_trace_dda_any_hemi_sets(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				 const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				 const float *d_orays, const int *d_oactive, int num_dirs, int set_w, int set_h,
				 const float *d_dirs, float radius, unsigned *d_mask);
/* The image scaled by the gathered share of open hemisphere rays, for the context's band: with num = d_vis[2p] and
 * den = d_vis[2p + 1] != 0 (what ugrt_filter_visibility wrote for the hemisphere masks) each of the pixel's three bytes
 * b becomes (b * num) / (num_dirs * den) in unsigned 32-bit integers (the largest product is 255 * 32 * 6561); den = 0
 * leaves the pixel as it is.  Behind a gather of radius 0 the bytes are ugrt_shade_ao's.  Stage UGRT_ST_SHADE.  num_dirs
 * outside 1..UGRT_MAX_AO_DIRS or a null argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_ao_shade_vis(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_vis, int num_dirs);

/* ---- device: indirect diffuse light, one bounce ----
 * A surface lit by the surfaces around it: every primary hit gathers the colour of what its hemisphere rays hit first.
 * Per frame: ugrt_ao_rays, ugrt_gi_gather, the shading calls, ugrt_gi_filter (optional), ugrt_gi_apply.  All arithmetic is
 * fp32 without contraction or unsigned 32-bit integer. */
/* The closest-hit hemisphere gather.  For an active pixel p of the band and sample s < num_dirs the ray {o, D} is exactly
 * ugrt_trace_dda_any_hemi_sets' (same k(p), same basis rule, same operation order; d_dirs is DEVICE memory,
 * [set_w * set_h][num_dirs][3] local directions).  Its hit is ugrt_trace_dda's -- the same cells, list order, a test
 * accepted with 0 < t < best, the walk ended behind the first cell whose exit parameter is not below an accepted t --
 * with two additions: best starts at min(3.0e38f, radius), and the walk also ends behind a cell whose exit parameter is
 * not below radius (the any-hit walk's rule; radius may be +inf).  A miss, or a hit whose material d_mat_idx[hit] is
 * outside 0..num_materials-1, has the colour 0; otherwise the colour is what ugrt_shade_reflect_depth gives a level's hit
 * at {o, D}, t and that triangle: the clamped Lambert term under the context's camera block and ugrt_set_light_position's
 * light.  With shadow_light (host float[3], passed on by value; NULL: no shadow phase) the colour is divided by 3.0f where
 * ugrt_trace_dda_any(t_max = 1) flags the ray ugrt_occlusion_rays forms from {o, D}, t, the triangle, shadow_light and
 * eps; glass is an ordinary surface in both phases.  d_sum, unsigned [4 * width * height], 16-byte aligned:
 * d_sum[4p + k], k = 0..2, is the sum over s of the colour's byte k (as the shading kernels turn a float into a byte; at
 * most 32 * 255) and d_sum[4p + 3] = 1; inactive pixels of the band get four zeros, pixels outside the band are not
 * written.  The index space is ugrt_trace_dda_any_area's (pixel group, sample): a pixel's rays sit in neighbouring lanes
 * of one wave, the ray, its hit, the occlusion ray and the colour stay in registers, the byte sums are added across the
 * lanes and stored with one 16-byte store, without atomic operations.  One prepare launch and one ray list serve the call;
 * the band's words are cleared in stream order.  Options "any_rays_per_wave" (unset: 64), "any_coop" and "dda_blocks"
 * shape the launch and change no word.  Stages UGRT_ST_WORKLIST / UGRT_ST_TRACE_DDA.  The call leaves the split-walk
 * history of ugrt_trace_dda and what ugrt_reflect_rays_next told it alone.  num_dirs outside 1..UGRT_MAX_AO_DIRS, set_w or
 * set_h outside 1..UGRT_MAX_AO_SET_TILE, set_w * set_h * num_dirs > UGRT_MAX_AO_SET_DIRS, radius <= 0 or NaN, eps NaN,
 * num_materials < 1, a d_sum that is not 16-byte aligned, or a null argument other than shadow_light: UGRT_EINVAL (the
 * message names the argument) and nothing is enqueued; without a built uniform grid the error of ugrt_trace_dda. */
int ugrt_gi_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
		   const float *d_vertlist, const int *d_trilist, const float *d_orays, const int *d_oactive, int num_dirs,
		   int set_w, int set_h, const float *d_dirs, float radius, const int *d_mat_idx, const float *d_mat_list,
		   int num_materials, const float *shadow_light, float eps, unsigned *d_sum);
/* ugrt_filter_visibility's gather -- its window, weights and acceptance tests -- over ugrt_gi_gather's sums: for an active
 * pixel d_acc[4p + k], k = 0..2, is the sum of w * d_sum[4q + k] over the accepted q (at most 6561 * 8160) and
 * d_acc[4p + 3] the sum of w (at most 6561); inactive pixels of the band get four zeros, pixels outside the band are not
 * written, radius 0 reproduces d_sum.  d_sum and d_acc are unsigned [4 * width * height], 16-byte aligned.  The stage,
 * the band rule and the errors are ugrt_filter_visibility's. */
int ugrt_gi_filter(ugrt_ctx *ctx, const unsigned *d_sum, const float *d_orays, const int *d_oactive, int radius,
		   float normal_cos, float plane_tol, unsigned *d_acc);
/* The gathered light onto the image, behind the shading call of the frame (d_intersect_id[p] holds the material index m by
 * then; it is only read).  d_acc is ugrt_gi_filter's output or ugrt_gi_gather's sums.  For a pixel of the band with m in
 * 0..num_materials-1 and den = d_acc[4p + 3] != 0, per component k:
 * a = (Kd_k * gain) * ((float)d_acc[4p + k] / (float)(255u * num_dirs * den)), the unsigned product converted once, a
 * clamped to 1 as the shading kernels clamp, and the byte b becomes min(255, b + byte(a)).  Every other pixel is left as
 * it is.  Stage UGRT_ST_SHADE.  gain < 0 or NaN, num_dirs outside 1..UGRT_MAX_AO_DIRS, a d_acc that is not 16-byte
 * aligned or a null argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_gi_apply(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_acc, int num_dirs, float gain,
		  const int *d_intersect_id, const float *d_mat_list, int num_materials);

/* ---- device: glossy reflections, a lobe of rays around the mirror direction ----
 * A reflecting surface whose material is not perfectly sharp averages what a cone of directions around the mirror
 * direction sees.  Per frame: ugrt_reflect_rays, ugrt_ao_rays, ugrt_glossy_gather, the shading call, ugrt_gi_filter
 * (optional, over the glossy sums with the glossy active words), ugrt_glossy_apply.  The library sees spreads as data: the
 * tangent of the lobe's half-angle per material.  All arithmetic is fp32 without contraction or unsigned 32-bit integer,
 * in the stated order. */
#define UGRT_MAX_GLOSSY_SAMPLES 32
#define UGRT_MAX_GLOSSY_SPREAD 1.0f
/* The lobe's closest-hit gather.  d_rays / d_active are ugrt_reflect_rays' {o, R} and active words; d_orays is
 * ugrt_ao_rays' {o', n}, of which only n is read; d_intersect_id holds the primary hits' TRIANGLES (the call runs before
 * the shading call).  For a pixel p of the band with d_active[p] != 0: m = d_mat_idx[d_intersect_id[p]] and
 * a = d_spread[m] where that is > 0 (NaN, zeros and negative values count as 0, values above UGRT_MAX_GLOSSY_SPREAD as
 * it; an id below 0 or an m outside 0..num_materials-1: a = 0).  For sample s < num_samples,
 * (u, v) = d_points[2 * (k(p) * num_samples + s) ..], k(p) = (row % set_h) * set_w + col % set_w (d_points is DEVICE
 * memory, [set_w * set_h][num_samples][2]), each clamped to [-1, 1], a NaN counting as 0.
 * r = R * (1 / sqrt((R0*R0 + R1*R1) + R2*R2)); D[k] = ((a*u)*T[k] + (a*v)*B[k]) + 1.0f*r[k] with T, B of the hemisphere
 * rays' basis rule over r (no special case for a = 0); c = (D0*n0 + D1*n1) + D2*n2, and where c < 0, D[k] becomes
 * D[k] - (2.0f*c)*n[k]: a sample that would enter the surface is mirrored back over it (c >= 0 or a NaN leaves D alone).
 * A D that is not finite is traced as ugrt_trace_dda traces such a ray.  The ray is {o, D}, o = d_rays[6p .. 6p + 2].
 * From there on the call is ugrt_gi_gather: the closest hit below radius (which may be +inf), the colour 0 on a miss or a
 * hit whose material is out of range, otherwise the clamped Lambert term under the context's camera block and
 * ugrt_set_light_position's light, divided by 3.0f where ugrt_trace_dda_any(t_max = 1) flags ugrt_occlusion_rays' ray
 * to shadow_light (host float[3]; NULL: no shadow phase), the bytes, their sums d_sum[4p + k] over s and
 * d_sum[4p + 3] = 1.  Inactive pixels of the band get four zeros, pixels outside the band are not written.  d_sum has
 * ugrt_gi_gather's layout, so ugrt_gi_filter gathers over it unchanged (called with d_active in the place of d_oactive:
 * only pixels that carry a lobe enter a neighbour's mean).  One prepare launch over d_active; the point table and the
 * words only the code between the walks needs are staged in LDS; groups are drawn from a ticket.  Options
 * "any_rays_per_wave", "any_coop" and "dda_blocks" shape the launch and change no word.  Stages UGRT_ST_WORKLIST /
 * UGRT_ST_TRACE_DDA.  The call leaves the split-walk history of ugrt_trace_dda alone.  num_samples outside
 * 1..UGRT_MAX_GLOSSY_SAMPLES, set_w or set_h outside 1..UGRT_MAX_AO_SET_TILE, radius <= 0 or NaN, eps NaN,
 * num_materials < 1, a d_sum that is not 16-byte aligned, or a null argument other than shadow_light: UGRT_EINVAL (the
 * message names the argument) and nothing is enqueued; without a built uniform grid the error of ugrt_trace_dda. */
int ugrt_glossy_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
		       const float *d_vertlist, const int *d_trilist, const float *d_rays, const int *d_active,
		       const float *d_orays, const int *d_intersect_id, const int *d_mat_idx, const float *d_spread,
		       int num_samples, int set_w, int set_h, const float *d_points, float radius, const float *d_mat_list,
		       int num_materials, const float *shadow_light, float eps, unsigned *d_sum);
/* The lobe's mean onto the image, directly behind the shading call of the frame (d_intersect_id[p] holds the material index
 * m by then; it is only read).  d_acc is ugrt_gi_filter's output or ugrt_glossy_gather's sums.  For a pixel of the band
 * with den = d_acc[4p + 3] != 0, m in 0..num_materials-1 and k = d_reflect[m] > 0 (a k above 1 counts as 1), per
 * component c: mean = (float)d_acc[4p + c] / (float)(num_samples * den), the unsigned product converted once, and the
 * byte b becomes min(255, ugrt_floor2i(((1.0f - k) * (float)b + k * mean) + 0.5f)).  Every other pixel is left as it is.
 * Stage UGRT_ST_SHADE.  num_samples outside 1..UGRT_MAX_GLOSSY_SAMPLES, a d_acc that is not 16-byte aligned or a null
 * argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_glossy_apply(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_acc, int num_samples,
		      const int *d_intersect_id, const float *d_reflect, int num_materials);

/* ---- device: Fresnel glass, a reflected and a transmitted ray per glass hit ----
 * The refraction chain follows one ray per hit; here a glass hit splits, and a pixel's rays form a tree of depth `depth`
 * that one launch walks.  Per frame: ugrt_refract_rays, ugrt_fresnel_gather, ugrt_fresnel_shade in the place of
 * ugrt_shade_reflect_depth*.  All arithmetic is fp32 without contraction, in the stated order.
 *
 * A node is a ray {o, d} with a weight w and a level j, and its hit (t, triangle) of material m in range.  The root
 * (level 0) is the primary hit of an active pixel: ray {cam, dir}, w = 1.  k = d_transmit[m] > 0 ? d_transmit[m] :
 * d_reflect[m].  A mirror (d_transmit[m] not > 0, d_reflect[m] > 0) has one child: the reflected ray, weight w*k.  Glass
 * (d_transmit[m] > 0) forms n, front, u, c, ior, eta and k2 = 1 - (eta*eta)*(1 - c*c) as the refracted ray above does; k2 < 0
 * gives one child, the mirrored ray, weight w*k; otherwise r0 = ((1 - ior)/(1 + ior))^2, cs = front ? c : sqrt(k2),
 * x = 1 - cs, F = scale * (r0 + (1 - r0)*(((x*x)*(x*x))*x)), child 0 the transmitted ray with (w*k)*(1 - F) and child 1 the
 * reflected ray with (w*k)*F.  The root's child 0 is d_rays[6p ..] as given.  A child is followed where its weight is
 * > min_weight (a NaN is not).  A node goes on when j < depth and a child is followed: it adds (w*(1 - k))*L, any other
 * node w*L, where L is the clamped Lambert colour of the hit under the context's camera block and light -- 0 on a miss or
 * a material out of range, the stored normal and t > 0 for the root, the triangle's normal for a level, and there divided
 * by 3.0f where the any-hit walk that sees through glass (t_max = 1) flags the occlusion ray of the hit to shadow_light
 * (host float[3]; NULL: no shadow phase).  Leaf b (depth bits; bit j = the child taken at level j's split, 0 where there
 * was none) owns the nodes whose remaining bits are 0 and adds their terms front to back from +0; the pixel's value is the
 * leaves' sum formed for j = depth-1 .. 0 by s[b] = s[b] + s[b + 2^j] (b < 2^j).  With scale = 0 every leaf but 0 holds +0
 * and the bytes are those of the chain of refracted levels shaded at the same depth.
 *
 * The gather: d_rays / d_active are the level-1 rays and words of the refracted rays' first call, d_normal ..
 * d_cam_position the primary arrays (d_intersect_id holds TRIANGLES: the call runs before the shading call).  For an
 * active pixel p of the band d_acc[4p .. 4p + 2] is the value above and d_acc[4p + 3] = 1.0f; inactive pixels of the band
 * get four zeros, pixels outside the band are not written.  2^depth neighbouring lanes are the leaves of a pixel; one
 * prepare launch over d_active, groups drawn from a ticket, one 16-byte store per pixel, no atomics on the sums.  Options
 * "any_rays_per_wave", "any_coop" and "dda_blocks" shape the launch and change no word.  Stages UGRT_ST_WORKLIST /
 * UGRT_ST_TRACE_DDA.  The call leaves the split-walk history of the closest-hit trace alone.  The context's state
 * "fresnel_nodes" gives the nodes the last call walked (it waits for the stream), "fresnel_gathers" counts the calls.
 * depth outside 1..UGRT_MAX_FRESNEL_DEPTH, scale outside [0, 1] or NaN, min_weight < 0 or NaN, eps NaN, num_materials < 1,
 * a d_acc that is not 16-byte aligned, or a null argument other than shadow_light: UGRT_EINVAL and nothing is enqueued;
 * without a built uniform grid the error of the closest-hit trace. */
#define UGRT_MAX_FRESNEL_DEPTH 6 /* 2^6 leaves: one wave */
int ugrt_fresnel_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
			const float *d_vertlist, const int *d_trilist, const float *d_rays, const int *d_active,
			const float *d_normal, const float *d_t_value, const float *d_ray_dir, const int *d_intersect_id,
			const float *d_cam_position, const int *d_mat_idx, const float *d_mat_list, const float *d_reflect,
			const float *d_transmit, const float *d_ior, int num_materials, int depth, float scale, float min_weight,
			const float *shadow_light, float eps, float *d_acc);
/* The shading call of a Fresnel frame (it rewrites d_intersect_id to material indices as the other shading calls do):
 * a pixel of the band with d_acc[4p + 3] != 0 gets the bytes of d_acc[4p .. 4p + 2], every other pixel what the depth
 * shading gives a pixel without a level-1 ray.  Stage UGRT_ST_SHADE.  A d_acc that is not 16-byte aligned or a null
 * argument: UGRT_EINVAL and nothing is enqueued.  (Named fresnel_shade, not shade_fresnel: the ugrt_shade_* family is a
 * closed table that tests/test_shade_calls.py counts.) */
int ugrt_fresnel_shade(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
		       const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position, const int *d_mat_idx,
		       const float *d_mat_list, int num_materials, const float *d_acc);

/* ---- device: smooth shading, crease-aware vertex normals interpolated per pixel ----
 * No reference counterpart: the reference shades every pixel with its triangle's normal.  All arithmetic is fp32, every
 * + - * / sqrt one IEEE operation, CROSS / DOT / NORMALIZE in the reference's operand order; every output is a function of
 * the inputs alone, bit for bit (no float atomics: each sum is formed by one thread in list order).
 *
 * ugrt_smooth_adjacency (topology; again when the face list changes).  Corner c = 3f + k of the face list belongs to
 * vertex v = d_facelist[c]; its key is d_vertex_key ? d_vertex_key[v] : v (d_vertex_key: one int per vertex, or NULL;
 * scenes.weld makes one).  Indices and keys lie in 0..num_vertices-1, as the grid builds require of the indices.  The
 * context keeps the corner indices stably sorted by key -- the corners of a key ascend -- and start[num_vertices + 1]:
 * the corners of key K stand at positions start[K] .. start[K + 1] - 1.  The context's own radix sort on
 * ceil(log2 num_vertices) key bits and one search per key; the call does not wait for the device.  num_faces == 0 is legal
 * (an empty list).  Stage UGRT_ST_BUILD_SORT.  A null d_facelist with faces, faces without a vertex, a negative count or
 * more than 2^30 corners: UGRT_EINVAL and nothing is enqueued.  ugrt_ctx_get_state "smooth_adjacency_builds" counts the
 * calls that built.
 * ugrt_smooth_get_adjacency (tests): the two arrays as device pointers, [3 num_faces] and [num_vertices + 1]; they stand
 * until the next ugrt_smooth_adjacency.  UGRT_EINVAL before the first one.
 *
 * ugrt_smooth_corner_normals (geometry; again when vertices move).  Per face g: A_g = CROSS(v1 - v0, v2 - v0), the
 * area weight, and N_g = NORMALIZE(A_g).  Per corner (f, k) with key K: S, from +0 per component, plus A_g for the
 * faces g = corner / 3 of K's list in list order (a face that stands twice in the list is added twice) for which
 * g == f or (N_f[0] * N_g[0] + N_f[1] * N_g[1]) + N_f[2] * N_g[2] >= crease_cos (a NaN rejects); the corner's normal
 * d_corner_normals[3c ..] is NORMALIZE(S), or N_f as it is where a component of that is not finite.  crease_cos <= -1:
 * every face of the list counts; crease_cos > 1: the corner's own face only.  One thread per corner: a vertex shared by
 * k faces costs k * k additions.  d_corner_normals: [9 num_faces] floats.  Stage UGRT_ST_BUILD_FILL.  UGRT_EINVAL and
 * nothing enqueued: crease_cos NaN, a null argument with faces, no adjacency, or one built for another num_faces.
 * ugrt_ctx_get_state "smooth_normal_builds" counts the calls that built.
 *
 * ugrt_smooth_normals (per pixel of the context's band, before the shading call: d_intersect_id holds triangle ids).
 * A pixel with id < 0 or !(t > 0) copies d_normal_in.  Otherwise, with tvec = d_cam_position - v0, e1 = v1 - v0,
 * e2 = v2 - v0 of triangle id and d the pixel's stored direction: pvec = CROSS(d, e2), det = DOT(e1, pvec) (inside
 * (-1e-21, 1e-21): failed), inv = 1 / det, u = DOT(tvec, pvec) * inv, v = DOT(d, CROSS(tvec, e1)) * inv -- the
 * intersection test's own, not clamped --, w = (1 - u) - v, n = NORMALIZE((w * n0 + u * n1) + v * n2) per component from
 * the triangle's three corner normals, ng = NORMALIZE(CROSS(e1, e2)).  The pixel gets ng where the determinant failed,
 * where n has a component that is not finite or where !(DOT(n, ng) > 0), else n; with fold != 0 each component c becomes
 * c < 0 ? c * -1 : c, as the primary tracer stores its normals.  d_normal_out == d_normal_in is allowed; pixels outside
 * the band are not written.  Stage UGRT_ST_SHADE.  A null argument: UGRT_EINVAL and nothing is enqueued. */
int ugrt_smooth_adjacency(ugrt_ctx *ctx, const int *d_facelist, int num_faces, int num_vertices, const int *d_vertex_key);
int ugrt_smooth_get_adjacency(ugrt_ctx *ctx, const unsigned **d_corners, const unsigned **d_start);
int ugrt_smooth_corner_normals(ugrt_ctx *ctx, const int *d_facelist, const float *d_vertlist, int num_faces,
			       float crease_cos, float *d_corner_normals);
int ugrt_smooth_normals(ugrt_ctx *ctx, const float *d_t_value, const float *d_ray_dir, const int *d_intersect_id,
			const float *d_cam_position, const float *d_vertlist, const int *d_trilist,
			const float *d_corner_normals, const float *d_normal_in, int fold, float *d_normal_out);

/* ---- device: texture mapping, a mip-mapped anisotropic albedo per pixel ----
 * No reference counterpart: the reference parses texture coordinates and a texture name and shades with Kd alone.
 * ugrt_texture_set builds a mip atlas on the device, ugrt_texture_albedo writes three floats per pixel -- the diffuse
 * colour of the pixel's primary hit --, ugrt_texture_shade / ugrt_texture_shade_lights shade with them in the place of the
 * material's Kd.  All float arithmetic is fp32, every + - * / sqrt floor one IEEE operation in the order written here, no
 * contraction; the mip chain is exact in integers.  Every output is a function of the inputs alone, bit for bit.
 *
 * ugrt_texture_set(ctx, n, wh, rgb_host).  n = 0..UGRT_MAX_TEXTURES textures; texture i is wh[2i] texels wide and
 * wh[2i + 1] high (each 1..UGRT_MAX_TEXTURE_DIM), rgb_host[i] points to its 3 * w * h bytes in HOST memory, row 0 first (the
 * row of v = 0), R G B per texel; all textures together hold at most UGRT_MAX_TEXTURE_TEXELS texels.  The context keeps one
 * device array of packed words r | g << 8 | b << 16 | 255 << 24 for every level of every texture (row-major) and a table
 * {width, height, word offset, levels} per (texture, level).  Level l + 1 of a texture has max(1, w_l >> 1) x
 * max(1, h_l >> 1) texels; its texel (x, y) is per channel (a + b + c + d + 2) >> 2 of the level-l texels at the columns
 * min(2x, w_l - 1), min(2x + 1, w_l - 1) and the rows min(2y, h_l - 1), min(2y + 1, h_l - 1); alpha stays 255.  The chain
 * ends at 1 x 1, so a texture has 1 + floor(log2(max(w, h))) levels, at most UGRT_MAX_TEXTURE_LEVELS.  Level 0 is copied
 * to the device, every further level is built there by one kernel launch per level over all textures; the call does not
 * wait for the device (rgb_host may be released when it returns; a call that follows another waits for that one's two
 * copies, whose host sources it writes again).  A call replaces the atlas of the call before; n = 0 drops it: it waits
 * for the context's stream and frees the device arrays.  Stage UGRT_ST_BUILD_FILL.  ugrt_ctx_get_state "texture_builds" counts the calls that succeeded with n > 0,
 * "texture_count" is n of the last call.  UGRT_EINVAL, and the atlas of the call before stands: n out of range, a null
 * wh or rgb_host or rgb_host[i] with n > 0, a dimension or the texel total out of range.  Any other failure (UGRT_ENOMEM
 * for the device arrays, UGRT_EHIP) leaves the context without an atlas -- "texture_count" 0, "texture_builds" as it was --,
 * never with a half-written one.
 * ugrt_texture_get_level (tests): width, height and the device pointer of the words of level `level` of texture `tex`;
 * they stand until the next ugrt_texture_set.  UGRT_EINVAL: no such texture or level.
 *
 * ugrt_texture_albedo: d_albedo[3p ..] for every pixel p = row * width + col of the context's band, before the shading
 * call (d_intersect_id holds triangle ids); it reads the context's current camera (ugrt_upload_camera).
 *   id < 0, !(t > 0), or m = d_mat_idx[id] outside 0..num_materials-1: three +0.
 *   Otherwise Kd = d_mat_list[6m + 3 ..], T = d_mat_texture[m] (device, one int per material; < 0: none) and the pixel gets
 *   Kd where T < 0 (or T >= the atlas's count, which the host check below excludes), where one of the three
 *   d_uv_facelist[3 id + k] lies outside 0..num_uvs-1, where the centre's determinant fails or where a component of the
 *   centre's uv is not finite.  Otherwise it gets Kd[c] * (filtered[c] / 255) per channel c.
 *   A ray's uv: tvec = d_cam_position - v0, e1 = v1 - v0, e2 = v2 - v0 of triangle id and a direction d; pvec = CROSS(d, e2),
 *   det = DOT(e1, pvec) (inside (-1e-21, 1e-21): failed), inv = 1 / det, u = DOT(tvec, pvec) * inv,
 *   v = DOT(d, CROSS(tvec, e1)) * inv -- ugrt_smooth_normals' own, not clamped --, w = (1 - u) - v, and per component
 *   uv = (w * uv0 + u * uv1) + v * uv2 of the corners' d_uvlist entries.  The centre's d is the pixel's stored direction
 *   d_ray_dir[3p ..]; the two neighbours' are the eye rays the primary pass forms at the image positions
 *   ((float)(col + 1), (float)row) and ((float)col, (float)(row + 1)) from the camera's node table (with
 *   UGRT_FLAG_STRICT_TEXTURE: through its filter rule), formed anew: nothing is read from another pixel, and the last
 *   column, the last row and a band's edge are pixels like the others.
 *   Footprint: W0 x H0 = level 0 of T.  dx = ((uvX[0] - uv[0]) * (float)W0, (uvX[1] - uv[1]) * (float)H0), dy likewise from
 *   the second neighbour; Lx = sqrt(dx[0] * dx[0] + dx[1] * dx[1]), Ly likewise.  major = dy where Ly > Lx, else dx;
 *   Lmax its length, Lmin the other's.  Where a neighbour's determinant failed or !(Lx < LIM) or !(Ly < LIM),
 *   LIM = 2 * UGRT_MAX_TEXTURE_DIM * 16 (a NaN or an infinite length lands here): N = 1, the last level, fraction 0 and
 *   major = (+0, +0) -- one tap at the centre on the 1 x 1 level.
 *   Otherwise N = the smallest integer in 1..max_aniso with Lmin * (float)N >= Lmax, or max_aniso where there is none;
 *   lambda = (Lmax / (float)N) * lod_bias_scale with lod_bias_scale = 2^lod_bias formed on the host; !(lambda > 1):
 *   level e = 0 and fraction f = 0; else e = lambda's unbiased exponent read from its bits and f = lambda / 2^e - 1 (the
 *   piecewise-linear log2); e >= the last level: the last level and f = 0.
 *   Tap i = 0..N-1: s = (float)(2i + 1) / (float)(2N) - 0.5, at (uv[0] + (s * major[0]) / (float)W0,
 *   uv[1] + (s * major[1]) / (float)H0); its value per channel is A = the bilinear value on level e, and where f != 0
 *   (1 - f) * A + f * B with B the bilinear value on level e + 1.
 *   Bilinear at (a, b) on a level of w x h: a' = a - floor(a), x = a' * (float)w - 0.5, x0 = floor(x), fx = x - x0, the
 *   columns (int)x0 and (int)x0 + 1, each c < 0 ? c + w : c, then c >= w ? c - w : c (the texture repeats; a' may be
 *   exactly 1 for a tiny negative a and stays inside; float to int as ugrt_f2i; an index that were still outside 0..w-1
 *   reads column 0); b, h and the rows likewise.  With the four texels' channel as floats 0..255:
 *   (c00 * (1 - fx) + c10 * fx) * (1 - fy) + (c01 * (1 - fx) + c11 * fx) * fy, c10 the next column, c01 the next row.
 *   filtered = the taps' values added in the order i = 0..N-1, from +0, divided by (float)N.
 *   max_aniso 1..UGRT_MAX_TEXTURE_ANISO (1: isotropic trilinear), lod_bias -16..16.  mat_texture_host is the host copy of
 *   d_mat_texture, read by the call's check only.  One thread per pixel; pixels outside the band are not written.  Stage
 *   UGRT_ST_SHADE.  UGRT_EINVAL and nothing enqueued: a null argument (d_uvlist may be null where num_uvs is 0),
 *   num_uvs or num_materials negative, a mat_texture_host entry >= the atlas's count (0 where there is no atlas: a material
 *   that names a texture needs one), max_aniso or lod_bias out of range.
 *
 * ugrt_texture_shade / ugrt_texture_shade_spotlight / ugrt_texture_shade_lights: ugrt_shade_simple / ugrt_shade_spotlight
 * (d_dump may be null) / ugrt_shade_lights with one more argument.  The Kd
 * that the shading of pixel p reads (twice: shader_kernel.cu:180-186) is d_albedo[3p ..] in the place of
 * d_mat_list[6m + 3 ..]; the id rewrite, the guards, the clamps and the bytes' rule are the same.  Where d_albedo holds
 * the material's Kd the image is that of the call without it, bit for bit. */
#define UGRT_MAX_TEXTURES 64
#define UGRT_MAX_TEXTURE_LEVELS 13          /* 1 + log2(UGRT_MAX_TEXTURE_DIM) */
#define UGRT_MAX_TEXTURE_TEXELS (1u << 26)  /* level 0 of all textures together */
#define UGRT_MAX_TEXTURE_ANISO 16
int ugrt_texture_set(ugrt_ctx *ctx, int n, const int *wh, const unsigned char *const *rgb_host);
int ugrt_texture_get_level(ugrt_ctx *ctx, int tex, int level, int *width, int *height, const unsigned **d_words);
int ugrt_texture_albedo(ugrt_ctx *ctx, const float *d_t_value, const float *d_ray_dir, const int *d_intersect_id,
			const float *d_cam_position, const float *d_vertlist, const int *d_facelist, const float *d_uvlist,
			int num_uvs, const int *d_uv_facelist, const int *d_mat_idx, const float *d_mat_list, int num_materials,
			const int *d_mat_texture, const int *mat_texture_host, int max_aniso, int lod_bias, float *d_albedo);
int ugrt_texture_shade(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
		      const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position, const int *d_mat_idx,
		      const float *d_mat_list, int num_materials, const float *d_albedo);
int ugrt_texture_shade_spotlight(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
				const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position, const int *d_mat_idx,
				const float *d_mat_list, int num_materials, float *d_dump, const float *d_albedo);
int ugrt_texture_shade_lights(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
			     const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position, const int *d_mat_idx,
			     const float *d_mat_list, int num_materials, int num_lights, const float *light_pos,
			     const int *d_is_shadowed, const float *d_albedo);

/* ---- device: adaptive anti-aliasing, sub-pixel eye rays on edge pixels ----
 * The frame takes one eye ray per pixel, through the pixel's corner.  ugrt_aa_edges finds the pixels that lie on an edge,
 * ugrt_aa_gather sends num_samples sub-pixel eye rays through each of them and through the uniform grid and shades every
 * sample as the frame shades a primary hit, ugrt_aa_resolve puts the mean into the image.  A sample with the offset (0, 0)
 * IS the pixel's primary hit, so supersampled and untouched pixels join without a seam.  Per frame: the primary pass and
 * the shadow stage, ugrt_aa_edges, the uniform grid, ugrt_aa_gather, the shading calls, ugrt_aa_resolve.  All arithmetic
 * is fp32 without contraction or unsigned 32-bit integer. */
#define UGRT_MAX_AA_SAMPLES 32
#define UGRT_MAX_AA_SET_TILE 4 /* set_w, set_h */
/* The edge flags, for the context's band; called BEFORE the frame's shading call, while d_intersect_id holds triangle ids.
 * With hit(x) = d_t_value[x] > 0 && d_intersect_id[x] >= 0, P_x = d_cam_position + d_t_value[x] * d_ray_dir[3x ..] per
 * component and n_x = d_normal[3x ..] as stored (component-wise absolute): d_edge[p] = 1 when for one of the up to eight
 * neighbours q of p inside the image (rows outside the band are read)
 *   hit(p) != hit(q), or
 *   both hit, the triangle ids differ and one of: d_mat_idx of the two ids differs;
 *     (n_p0*n_q0 + n_p1*n_q1) + n_p2*n_q2 < normal_cos;
 *     fabsf((n_p0*(P_q0-P_p0) + n_p1*(P_q1-P_p1)) + n_p2*(P_q2-P_p2)) > plane_tol, or
 *   d_is_shadowed (may be NULL) is given and d_is_shadowed[p] != d_is_shadowed[q];
 * otherwise d_edge[p] = 0 (a miss among misses gets 0).  Pixels outside the band are not written.  Stage UGRT_ST_SHADE.
 * A tolerance that is a NaN or a null argument other than d_is_shadowed: UGRT_EINVAL and nothing is enqueued. */
int ugrt_aa_edges(ugrt_ctx *ctx, const float *d_normal, const float *d_t_value, const float *d_ray_dir,
		  const int *d_intersect_id, const float *d_cam_position, const int *d_mat_idx, const int *d_is_shadowed,
		  float normal_cos, float plane_tol, int *d_edge);
/* The sub-pixel eye rays of the pixels of the band with d_edge[p] != 0.  eye_camcoords is the EYE's camera block (host
 * memory, float[64]): when a frame shades, the context's current block is the light camera's, which the shading below
 * reads; the directions and the depth gate need the eye's.  Sample s of pixel p = (col, row) = (p % width, p / width):
 * the origin is eye_camcoords[0..2]; the direction is the primary pass's (the 5x5 node table of
 * ugrt_camera_direction_table(eye_camcoords), UGRT_FLAG_STRICT_TEXTURE included) with (float)col + sx and (float)row + sy
 * in the place of (float)col and (float)row, (sx, sy) = d_offsets[2 * (k(p) * num_samples + s) ..], k(p) =
 * (row % set_h) * set_w + (col % set_w); d_offsets is DEVICE memory, [set_w * set_h][num_samples][2] floats in
 * [-0.5, 0.5) (a value outside [-0.5, 0.5] is clamped to it, a NaN counts as -0.5).  The hit is ugrt_trace_dda's -- the same cells, list order, a test accepted with 0 < t < best, the same end
 * of the walk -- and counts only where the primary epilogue's depth gate passes under the eye's MVP.  A miss, or a hit
 * whose material d_mat_idx[hit] is outside 0..num_materials-1, has the colour 0; otherwise the bytes are what
 * ugrt_shade_simple gives a primary hit of that triangle at {eye, direction, t}: the normal as ugrt_trace_primary stores it,
 * the point eye + t * direction, the Lambert term under the context's CURRENT camera block and ugrt_set_light_position's
 * light, clamped.  With shadow_light (host float[3]; NULL: no shadow phase) each byte b becomes b / 3 where
 * ugrt_trace_dda_any(t_max = 1) flags the ray ugrt_occlusion_rays forms from {eye, direction}, t, the triangle,
 * shadow_light and eps.  d_sum, unsigned [4 * width * height], 16-byte aligned: for a flagged pixel d_sum[4p + k],
 * k = 0..2, is the sum over s of byte k and d_sum[4p + 3] = 1; the other pixels of the band get four zeros, pixels outside
 * the band are not written.  The index space, the prepare launch, the ray list, the store, the options
 * ("any_rays_per_wave", "any_coop", "dda_blocks": no word changes), the stages and leaving the split-walk history alone
 * are ugrt_gi_gather's.  num_samples outside 1..UGRT_MAX_AA_SAMPLES, set_w or set_h outside 1..UGRT_MAX_AA_SET_TILE, eps
 * NaN, num_materials < 1, a d_sum that is not 16-byte aligned, or a null argument other than shadow_light: UGRT_EINVAL
 * (the message names the argument) and nothing is enqueued; without a built uniform grid the error of ugrt_trace_dda. */
int ugrt_aa_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
		   const float *d_vertlist, const int *d_trilist, const float *eye_camcoords, const int *d_edge,
		   int num_samples, int set_w, int set_h, const float *d_offsets, const int *d_mat_idx,
		   const float *d_mat_list, int num_materials, const float *shadow_light, float eps, unsigned *d_sum);
/* The supersampled pixels onto the image, behind the frame's shading calls (and ugrt_shade_add_shadows) and before
 * ambient occlusion scales the image: for a pixel of the band with d_sum[4p + 3] != 0 byte k becomes
 * (d_sum[4p + k] + num_samples / 2) / num_samples in unsigned integers; every other pixel is left as it is.  Stage
 * UGRT_ST_SHADE.  num_samples outside 1..UGRT_MAX_AA_SAMPLES, a d_sum that is not 16-byte aligned or a null argument:
 * UGRT_EINVAL and nothing is enqueued. */
int ugrt_aa_resolve(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_sum, int num_samples);

/* ---- device: depth of field, thin-lens eye rays on the pixels whose blur matters ----
 * The frame's camera is a pinhole.  ugrt_dof_pixels finds the pixels that a circle of confusion reaches, ugrt_dof_gather
 * sends num_samples rays from points of a lens through each of them and shades every sample as the frame shades a primary
 * hit, ugrt_aa_resolve puts the mean into the image.  A sample from the lens's centre IS ugrt_aa_gather's sample.  Per
 * frame: the primary pass and the shadow stage, ugrt_dof_pixels, the uniform grid, ugrt_dof_gather, the shading calls,
 * ugrt_aa_resolve.  All arithmetic is fp32 without contraction, in the stated order, or 32-bit integer. */
#define UGRT_MAX_DOF_WINDOW 8 /* radius of ugrt_dof_pixels */
/* The lens flags, for the context's band; called BEFORE the frame's shading call, while d_intersect_id holds triangle ids.
 * axis is HOST memory, float[3]: A, the unit view axis.  For a pixel q with hit(q) = d_t_value[q] > 0 &&
 * d_intersect_id[q] >= 0:
 *   z_q = d_t_value[q] * ((dir_q0*A_0 + dir_q1*A_1) + dir_q2*A_2), dir_q = d_ray_dir[3q ..];
 *   coc_q = (coc_scale * fabsf(z_q - focus)) / z_q for a hit with z_q > 0, and 0 otherwise (a miss, a NaN t).
 * d_flags[p] = 1 when some q inside the image (rows outside the band are read) with m = max(|dx|, |dy|) <= radius, p
 * itself included, has coc_q >= coc_min and coc_q >= (float)m; otherwise 0 (a coc_q that is a NaN meets neither).
 * Pixels outside the band are not written.  coc_scale is the caller's: lens radius * focal length in pixels / focus.
 * Stage UGRT_ST_SHADE, one launch.  A NaN in axis, focus, coc_scale or coc_min, radius outside 0..UGRT_MAX_DOF_WINDOW or a
 * null argument: UGRT_EINVAL (the message names the argument) and nothing is enqueued. */
int ugrt_dof_pixels(ugrt_ctx *ctx, const float *d_t_value, const float *d_ray_dir, const int *d_intersect_id,
		    const float *axis, float focus, float coc_scale, float coc_min, int radius, int *d_flags);
/* The lens rays of the pixels of the band with d_flags[p] != 0 (ugrt_dof_pixels', or any caller's).  The arguments are
 * ugrt_aa_gather's, with d_flags where d_edge stands, and lens, HOST memory, float[10]: lens[0..2] = U and lens[3..5] = V,
 * world vectors along the lens's two axes whose length is the lens radius; lens[6..8] = A, the unit view axis; lens[9] =
 * F, the focus distance along A.  d_table is DEVICE memory, [set_w * set_h][num_samples][4] floats (sx, sy, lu, lv);
 * sample s of pixel p = (col, row) reads entry k(p) * num_samples + s, k(p) as in ugrt_aa_gather, and is formed in this
 * order:
 *   sx, sy clamped as ugrt_aa_gather clamps them; lu, lv each clamped to [-1, 1], a NaN counts as 0;
 *   d0 = ugrt_aa_gather's direction at ((float)col + sx, (float)row + sy), UGRT_FLAG_STRICT_TEXTURE included;
 *   c = (d0_0*A_0 + d0_1*A_1) + d0_2*A_2;  s_f = F / c;  L_k = lu*U_k + lv*V_k;
 *   !(c > 0): the pinhole ray, o = eye, d = d0;  otherwise o_k = eye_k + L_k, d_k = d0_k - L_k / s_f.
 * d is not normalised again: t keeps the pinhole ray's scale, and all lens rays of one image point meet on the plane
 * A . (P - eye) = F.  With lu = lv = 0, or U = V = 0, the ray is ugrt_aa_gather's.  Everything behind the ray is
 * ugrt_aa_gather's on {o, d}: the closest hit, the depth gate under the eye's MVP at P = o + t * d, the primary hit's
 * shading at P, the occlusion ray towards shadow_light and the / 3, d_sum's four words per pixel, the zeros of the band's
 * other pixels, the index space, the options and the stages.  Every case that is UGRT_EINVAL for ugrt_aa_gather, a null
 * lens, a U, V or A that is not finite, an F that is not finite or F <= 0: UGRT_EINVAL (the message names the argument)
 * and nothing is enqueued. */
int ugrt_dof_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
		    const float *d_vertlist, const int *d_trilist, const float *eye_camcoords, const float *lens,
		    const int *d_flags, int num_samples, int set_w, int set_h, const float *d_table, const int *d_mat_idx,
		    const float *d_mat_list, int num_materials, const float *shadow_light, float eps, unsigned *d_sum);

/* ---- device: temporal accumulation, DESIGN.md section 6.12 ----
 * A sequence of frames gives frame f a different sample set and carries a per-pixel running mean of the share of open
 * rays (ambient occlusion, area light) or of the indirect light's colour from frame to frame: after N frames a pixel has
 * seen N * S samples for the price of S per frame.  Under a moving camera the mean is fetched where the pixel's surface
 * point lay in the previous frame, and dropped where the previous frame saw another surface there.  Per frame and effect:
 * the walk, the gather (radius 0 when no gather is wanted: it forms the pair), ugrt_temporal_visibility or
 * ugrt_temporal_gi, then the shading call of the gather's output on the temporal output.  All arithmetic is fp32 without
 * contraction, in the stated order, or 32-bit integer. */
#define UGRT_MAX_TEMPORAL_FRAMES 64
#define UGRT_TEMPORAL_DEN 256u
/* d_vis is what ugrt_filter_visibility wrote for this frame, d_orays / d_oactive this frame's {o, n} per pixel
 * (ugrt_ao_rays), d_prev_orays / d_prev_oactive the previous frame's, prev_camcoords the EYE's camera block of the previous
 * frame (host memory, float[64]; its modelview and projection rows are passed on by value), d_hist_in the history the
 * previous frame's call wrote, float [2 * width * height]: (share, frames) per pixel; zeros start a sequence.  For an
 * active pixel p = (x, y) of the band with (num, den) = d_vis[2p ..], den != 0 (an active pixel with den == 0 is treated
 * as inactive), S = num_bits:
 *   input share  c = (float)num / (float)(S * den), the unsigned product converted once.
 *   reprojection the reference's vertex transform (MV, divide, P, divide; the arithmetic of the screen-grid binning) of
 *     o_p = floats 0..2 of d_orays[6p] under prev_camcoords gives (ndc0, ndc1) and the projective w of the second divide;
 *     fx = ((ndc0 + 1.0f) / 2.0f) * (float)width, fy = ((ndc1 + 1.0f) / 2.0f) * (float)height, the binning's mapping,
 *     unflipped: it sends the hit point of pixel (col, row) under its own camera to (col, row).  No history when w is not
 *     > 0, when fx, fy or w is a NaN, or unless -1 < fx < width and -1 < fy < height.
 *   taps  X = ugrt_floor2i(fx * 16.0f + 0.5f), ix = X >> 4, ax = X & 15, Y, iy, ay likewise; the taps are
 *     q = (ix + i, iy + j), i, j in {0, 1}, in the order (0,0), (1,0), (0,1), (1,1), with the integer weights
 *     w = (i ? ax : 16 - ax) * (j ? ay : 16 - ay).  A tap of weight 0 is not read.  A tap counts when q is inside the
 *     image and inside the band's rows, d_prev_oactive[q] != 0, its stored frames_q >= 1, its stored share h_q is in
 *     [0, 1] (a NaN rejects), (n_p0*n_q0 + n_p1*n_q1) + n_p2*n_q2 >= normal_cos and
 *     |(d0*n_p0 + d1*n_p1) + d2*n_p2| <= plane_tol with d = o_q(previous) - o_p: ugrt_filter_visibility's two tests.
 *   blend  no tap counts: h = c, n = 1.  Otherwise hp = (sum of (float)w * h_q, from 0.0f in tap order) / (float)(sum of
 *     w), n = min(min over the counted taps of frames_q + 1.0f, (float)max_frames), h = hp + (c - hp) / n; n = 1
 *     (max_frames = 1) gives h = c itself, not hp + (c - hp), which may miss c by an ulp.
 *   output  d_hist_out[2p ..] = (h, n); d_vis_out[2p] = min(S * 256, ugrt_floor2i(h * (float)(S * 256u) + 0.5f)),
 *     d_vis_out[2p + 1] = UGRT_TEMPORAL_DEN.
 * Inactive pixels of the band get zeros in both outputs (frame count 0), pixels outside the band are not written;
 * max_frames = 1 gives back the quantised input.  The pair is what ugrt_shade_area_vis and ugrt_ao_shade_vis consume:
 * with den = 256 and num <= 32 * 256 their largest products are 255 * 3 * 32 * 256 and 255 * 32 * 256, below the
 * bounds they document for the gather's den <= 6561.  One launch, a 32 x 8 tile per workgroup, no LDS, no atomic
 * operation.  Stage UGRT_ST_SHADE.  max_frames outside 1..UGRT_MAX_TEMPORAL_FRAMES, num_bits outside 1..32, a plane_tol
 * that is negative or a NaN, a NaN normal_cos, d_hist_in == d_hist_out, d_vis == d_vis_out (neighbours are read) or a
 * null argument: UGRT_EINVAL (the message names the argument) and nothing is enqueued. */
int ugrt_temporal_visibility(ugrt_ctx *ctx, const unsigned *d_vis, int num_bits, const float *d_orays, const int *d_oactive,
			     const float *prev_camcoords, const float *d_prev_orays, const int *d_prev_oactive,
			     const float *d_hist_in, int max_frames, float normal_cos, float plane_tol, float *d_hist_out,
			     unsigned *d_vis_out);
/* The same over ugrt_gi_filter's sums (radius 0 reproduces ugrt_gi_gather's): d_acc, d_acc_out unsigned and d_hist_in,
 * d_hist_out float [4 * width * height], all 16-byte aligned; the history is (r, g, b shares, frames) per pixel.  With
 * den = d_acc[4p + 3] and S = num_dirs: c_k = (float)d_acc[4p + k] / (float)(255u * S * den); a tap counts when all three
 * stored shares are in [0, 1]; every channel is blended with the same taps, weights and n; d_acc_out[4p + k] =
 * min(255 * S * 256, ugrt_floor2i(h_k * (float)(255u * S * 256u) + 0.5f)), d_acc_out[4p + 3] = UGRT_TEMPORAL_DEN.  That is
 * what ugrt_gi_apply consumes: its divisor 255 * num_dirs * den is at most 255 * 32 * 256.  Everything else, the errors
 * included (num_dirs in the place of num_bits; also a buffer of the four that is not 16-byte aligned), is
 * ugrt_temporal_visibility's. */
int ugrt_temporal_gi(ugrt_ctx *ctx, const unsigned *d_acc, int num_dirs, const float *d_orays, const int *d_oactive,
		     const float *prev_camcoords, const float *d_prev_orays, const int *d_prev_oactive, const float *d_hist_in,
		     int max_frames, float normal_cos, float plane_tol, float *d_hist_out, unsigned *d_acc_out);

/* ---- device: animation (scene.h:122,336) -------------------------------- */
/* Model::rotate_bunny(float) -> copy_data_transform, transformation_kernel.cu:4 */
int ugrt_animate(ugrt_ctx *ctx, float *d_vertlist, const float *d_orig_list, int size, int offset,
		 float rot_factor);

/* ---- profiling ---------------------------------------------------------- */
/* hipEvent pairs around stages, on the context's stream.  on = 0: off; 1: every stage; otherwise a
 * mask in which bit (s + 1) selects stage UGRT_ST_s */
int ugrt_prof_enable(ugrt_ctx *ctx, int on);
int ugrt_prof_reset(ugrt_ctx *ctx);
/* total milliseconds and number of timed launches of a stage since the reset
 * (synchronises the stream) */
int ugrt_prof_get(ugrt_ctx *ctx, int stage, double *ms_total, int *launches);
/* counters of the last tracer launches (synchronises the stream): [0] primary work-item
 * capacity, [1] shadow beams, [2] shadow chunks traced, [6] shadow cull pass: (triangle, beam)
 * tests, [7] shadow exact pass: candidates staged (candidate pairs x 64-ray sub-groups);
 * with UGRT_FLAG_COUNT_WORK also [3] DDA candidates tested, [4] DDA cells visited, [5] DDA active rays */
int ugrt_stats_get(ugrt_ctx *ctx, unsigned long long stats[8]);
/* how the beam kernel of ugrt_trace_dda shared its work in the last counting launch (UGRT_FLAG_COUNT_WORK):
 * [0] wave iterations (4 steps each), [1] cell groups processed, [2] rays in those groups, [3] cull batches,
 * [4] triangles culled against a ray bundle, [5] exact-test rounds (one broadcast triangle), [6] rays that ran
 * those rounds, [7] exact tests of lone rays, [8..23] waves by log2(shader cycles / 4096), [24] sum and
 * [25] maximum of the waves' cycles; entries past n are not written, entries past 25 are 0 */
int ugrt_stats_dda(ugrt_ctx *ctx, unsigned long long *stats, int n);
/* split walks of the context's last ugrt_trace_dda (option "dda_split"; synchronises the stream): [0] segments the
 * cut ray groups were listed as, [1] jobs of the launch before, [2] cut groups some of whose rays had to be walked
 * again in one piece, [3] those rays */
int ugrt_stats_dda_split(ugrt_ctx *ctx, unsigned out[4]);
/* The same for the primary tracer: [0] work items (tile x list segment), [1] batches of 64 references culled,
 * [2] batches with a survivor of the tile's box, [3] references, [4] survivors of the tile's box, [5] survivors of a
 * quadrant's box (staged in LDS), [6] jobs (survivor x quadrant), [7] flushes, [8] exact rounds (4 jobs x 16 rays),
 * [9] rounds that reach the division, [10] the v test, [11] t, [12] (ray, triangle) tests, [13] accepted hits */
int ugrt_stats_primary(ugrt_ctx *ctx, unsigned long long *stats, int n);

#ifdef __cplusplus
}
#endif
#endif /* UGRT_H */
