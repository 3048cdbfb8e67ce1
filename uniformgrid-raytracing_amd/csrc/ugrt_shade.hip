// ugrt_shade.hip -- per-pixel stages: light-space ray mapping, ray re-ordering, every shader (the reference's, and the
// passes that blend reflection levels, lights and mask words into the image), vertex animation.  (The rays those levels
// come from: ugrt_bounce.hip; the gather in front of ugrt_shade_area_vis: ugrt_filter.hip.)
#include "ugrt_dev.h"
#include "ugrt_scan.h"

// mapSort_Effective_kernel, misc_kernel.cu:255-296 (cam = LIGHT camera).
// The reference launches one 8x8 block per tile; per-pixel work has no tile
// structure, so this is a flat, fully coalesced pass over the band's pixels.
__global__ __launch_bounds__(PX_THREADS) void k_map_rays(CamBlock cam, const float *__restrict__ t_value_list,
							  const float *__restrict__ ray_direction,
							  u32 *__restrict__ d_map, const float *__restrict__ cmPt,
							  float xM, float yM, int lnbx, int lnby, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelId = p0 + i;
	float tVal = t_value_list[pixelId];
	float pI[3], lrd[3];
	pI[0] = cmPt[0] + tVal * ray_direction[pixelId * 3 + 0];
	pI[1] = cmPt[1] + tVal * ray_direction[pixelId * 3 + 1];
	pI[2] = cmPt[2] + tVal * ray_direction[pixelId * 3 + 2];
	lrd[0] = pI[0] - cam.cc[0];
	lrd[1] = pI[1] - cam.cc[1];
	lrd[2] = pI[2] - cam.cc[2];
	D_NORMALIZE(lrd);
	int blx = (int)d_effective_x(cam, lrd, xM, lnbx / 2);
	int bly = (int)d_effective_y(cam, lrd, yM, lnby / 2);
	int blockIndex;
	if (blx >= 0 && blx < lnbx && bly >= 0 && bly < lnby)
		blockIndex = blx * lnby + bly;
	else
		blockIndex = lnbx * lnby;
	d_map[i] = (u32)pixelId;
	d_map[n + i] = (u32)blockIndex;
}

// getEffectiveRayGridMapping, per_frame_funcs.h:97-114
extern "C" int ugrt_map_rays_to_light(ugrt_ctx *ctx, const float *d_t_value, const float *d_ray_dir, unsigned *d_map,
				      const float *d_cam_position, float xM, float yM)
{
	if (!ctx || !d_t_value || !d_ray_dir || !d_map || !d_cam_position)
		return ugrt_fail(UGRT_EINVAL, "map_rays_to_light: null argument");
	return ugrt_launch_pixels(ctx, UGRT_ST_MAP_RAYS, k_map_rays, ctx->cam, d_t_value, d_ray_dir, d_map, d_cam_position, xM,
				  yM, ctx->cfg.light_nbx, ctx->cfg.light_nby);
}

// ---------------------------------------------------------------------------
// processData, per_frame_funcs.h:116-137.  Reference: 15-bit radix sort of N
// rays, then five N-sized passes (blockScan, cudppSegmentedScan,
// preStreamCompaction, tag_thread, cudppCompact: decision_data.h:171-271) to
// find the first ray of every 64-ray chunk.  Here: the same stable sort, ONE
// N-sized pass that records where each light cell's run starts and ends, and
// the chunk starts are then generated per CELL (run start + 64*j), which is
// the same ascending list.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PX_THREADS) void k_ray_runs(const u32 *__restrict__ keys, u32 n, u32 *__restrict__ rstart,
							  u32 *__restrict__ rend)
{
	u32 i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	u32 k = keys[i];
	if (i == 0 || keys[i - 1] != k)
		rstart[k] = i;
	if (i == n - 1 || keys[i + 1] != k)
		rend[k] = i + 1;
}

// chunks per light cell, formed where the scan of the counts loads them (ugrt_scan.h)
struct ChunkLoad {
	const u32 *rstart, *rend;
	__device__ __forceinline__ void operator()(u32 base, u32 n, u32 (&v)[SC_ITEMS]) const
	{
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++) {
			const u32 c = base + (u32)k;
			v[k] = c < n ? (rend[c] - rstart[c] + 63u) / 64u : 0u;
		}
	}
};

// one thread per CHUNK (a cell with thousands of rays would otherwise serialise one thread)
__global__ __launch_bounds__(PX_THREADS) void k_chunk_emit(const u32 *__restrict__ rstart,
							    const u32 *__restrict__ rend,
							    const u32 *__restrict__ incl, u32 ncell, u32 cap,
							    u32 *__restrict__ prefix, u32 *__restrict__ host_total)
{
	const u32 total = incl[ncell - 1];
	u32 k = blockIdx.x * PX_THREADS + threadIdx.x;
	if (k == 0u)
		*host_total = total; // h_numCudaBlocks, decision_data.h:264: straight into the pinned host word
	if (k >= total || k >= cap)
		return;
	u32 lo = 0, hi = ncell - 1; // smallest c with incl[c] > k
	while (lo < hi) {
		u32 mid = (lo + hi) >> 1;
		if (incl[mid] > k)
			hi = mid;
		else
			lo = mid + 1;
	}
	const u32 c = lo;
	const u32 j = k - (incl[c] - (rend[c] - rstart[c] + 63u) / 64u);
	prefix[k] = rstart[c] + 64u * j;
}

static int key_bits(u32 nkeys)
{
	int b = 1;
	while (b < 32 && (1ull << b) < (unsigned long long)nkeys)
		b++;
	return b;
}

// the sort, the runs per light cell and the chunk starts (enqueued; the chunk count goes to the pinned host word)
static int sort_rays_now(ugrt_ctx *ctx, unsigned *d_map, unsigned *d_prefix_map, unsigned prefix_capacity)
{
	hipStream_t st = ctx->stream;
	const u32 n = (u32)ctx->npix;
	const u32 ncell = (u32)ctx->cfg.light_nbx * (u32)ctx->cfg.light_nby + 1u; // + sentinel
	int rc;
	if ((rc = ugrt_buf_reserve(ctx, ctx->rmap[0], (size_t)n * 8)))
		return rc;
	if ((rc = ugrt_buf_reserve(ctx, ctx->rstart, (size_t)ncell * 8))) // run starts, then run ends
		return rc;
	if ((rc = ugrt_buf_reserve(ctx, ctx->cbase, (size_t)ncell * 4)))
		return rc;
	u32 *tmp = (u32 *)ctx->rmap[0].p;
	ugrt_prof_begin(ctx, UGRT_ST_SORT_RAYS);
	// cudppSort(sortPlan, &d_map[IMAGE_SIZE], &d_map[0], 15, IMAGE_SIZE), decision_data.h:177: in place.  With an even
	// number of passes the built-in sort reads its input in the first pass only (and in the histogram kernel before
	// it), writes its own buffers there, and may write the caller's arrays in its last pass; otherwise sort into a
	// copy and copy back.
	const int kb = key_bits(ncell);
	if (((kb + 7) / 8) % 2 == 0 && ctx->opt[UGRT_OPT_SORT_LIBRARY] != 1 && n <= (1u << 30)) {
		rc = ugrt_sort_pairs_u32(ctx, d_map + n, d_map + n, d_map, d_map, n, kb);
		if (rc)
			return rc;
	} else {
		rc = ugrt_prim_sort_pairs(ctx, d_map + n, tmp + n, d_map, tmp, n, kb);
		if (rc)
			return rc;
		UGRT_HIP(hipMemcpyAsync(d_map, tmp, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
	}
	u32 *rstart = (u32 *)ctx->rstart.p, *rend = rstart + ncell;
	UGRT_HIP(hipMemsetAsync(rstart, 0, (size_t)ncell * 8, st));
	hipLaunchKernelGGL(k_ray_runs, dim3((n + PX_THREADS - 1) / PX_THREADS), dim3(PX_THREADS), 0, st,
			   (const u32 *)(d_map + n), n, rstart, rend);
	UGRT_HIP(hipGetLastError());
	{
		const ChunkLoad load = { rstart, rend };
		if ((rc = ugrt_scan_launch<true>(ctx, load, (u32 *)ctx->cbase.p, ncell, ScanTailNone())))
			return rc;
	}
	{
		// at most n/64 + ncell chunks exist; the kernel reads the exact count on the device
		u32 maxchunks = n / 64u + ncell;
		if (maxchunks > prefix_capacity)
			maxchunks = prefix_capacity;
		hipLaunchKernelGGL(k_chunk_emit, dim3((maxchunks + PX_THREADS - 1) / PX_THREADS), dim3(PX_THREADS), 0, st,
				   (const u32 *)rstart, (const u32 *)rend, (const u32 *)ctx->cbase.p,
				   ncell, prefix_capacity, d_prefix_map, ctx->h_pinned + UGRT_PIN_CHUNKS);
	}
	UGRT_HIP(hipGetLastError());
	ugrt_prof_end(ctx, UGRT_ST_SORT_RAYS);
	ctx->ray_sort_pending = false;
	return UGRT_OK;
}

extern "C" int ugrt_sort_rays(ugrt_ctx *ctx, unsigned *d_map, unsigned *d_prefix_map, unsigned prefix_capacity,
			      unsigned *num_chunks)
{
	if (!ctx || !d_map || !d_prefix_map)
		return ugrt_fail(UGRT_EINVAL, "sort_rays: null argument");
	UGRT_HIP(hipSetDevice(ctx->device));
	ctx->chunk_capacity = prefix_capacity;
	ctx->chunk_prefix = d_prefix_map;
	ctx->chunk_map = d_map;
	// Deferred form under UGRT_FLAG_SHADOW_ALL_CHUNKS: the chunk list only says WHICH rays the reference's launch traces,
	// and with that flag it is all of them -- the shadow tracer reads (pixel, light cell) pairs in any order and puts them
	// in (cell, direction) order itself.  The sort is then carried out when its results are asked for
	// (ugrt_sort_rays_chunks), not before: two radix passes and five more launches that a frame does not need.
	if (!num_chunks && (ctx->cfg.flags & UGRT_FLAG_SHADOW_ALL_CHUNKS) && ctx->opt[UGRT_OPT_RAY_SORT] != 1) {
		ctx->ray_sort_pending = true;
		return UGRT_OK;
	}
	int rc = sort_rays_now(ctx, d_map, d_prefix_map, prefix_capacity);
	if (rc || !num_chunks)
		return rc; // deferred: the count stays on the device (UGRT_CHUNKS_ON_DEVICE) until ugrt_sort_rays_chunks
	return ugrt_sort_rays_chunks(ctx, num_chunks);
}

extern "C" int ugrt_sort_rays_chunks(ugrt_ctx *ctx, unsigned *num_chunks)
{
	if (!ctx || !num_chunks)
		return ugrt_fail(UGRT_EINVAL, "sort_rays_chunks: null argument");
	UGRT_HIP(hipSetDevice(ctx->device));
	if (ctx->ray_sort_pending) { // the sort that ugrt_sort_rays(..., NULL) put off: its arrays still hold the unsorted map
		int rc = sort_rays_now(ctx, const_cast<unsigned *>(ctx->chunk_map), const_cast<unsigned *>(ctx->chunk_prefix), ctx->chunk_capacity);
		if (rc)
			return rc;
	}
	UGRT_HIP(hipStreamSynchronize(ctx->stream));
	*num_chunks = ctx->h_pinned[UGRT_PIN_CHUNKS];
	if (*num_chunks > ctx->chunk_capacity)
		return ugrt_fail(UGRT_EINVAL, "sort_rays: %u chunks do not fit prefix_capacity %u", *num_chunks,
				 ctx->chunk_capacity);
	return UGRT_OK;
}

// ---------------------------------------------------------------------------
// shading: lambertian_shade :165-221, spot_shade :275-345, shadow_kernel :347
// ---------------------------------------------------------------------------
// shader_kernel.cu:223-273 get_along_x / get_along_y
__device__ __forceinline__ float d_along_x(const CamBlock &cam, const float *vec)
{
	const float *cc = cam.cc;
	float upDotValue = vec[0] * cc[16 + 1] + vec[1] * cc[16 + 5] + vec[2] * cc[16 + 9];
	float tmp[3];
	tmp[0] = vec[0] - upDotValue * cc[16 + 1];
	tmp[1] = vec[1] - upDotValue * cc[16 + 5];
	tmp[2] = vec[2] - upDotValue * cc[16 + 9];
	float val = d_magnitude(tmp);
	tmp[0] /= val;
	tmp[1] /= val;
	tmp[2] /= val;
	float forwardDotValue = tmp[0] * cc[16 + 2] + tmp[1] * cc[16 + 6] + tmp[2] * cc[16 + 10];
	float angle = ugrt_acosf(forwardDotValue);
	float rightDotValue = tmp[0] * cc[16 + 0] + tmp[1] * cc[16 + 4] + tmp[2] * cc[16 + 8];
	return (rightDotValue > 0) ? angle : -1.0f * angle;
}
__device__ __forceinline__ float d_along_y(const CamBlock &cam, const float *vec)
{
	const float *cc = cam.cc;
	float rightDotValue = vec[0] * cc[16 + 0] + vec[1] * cc[16 + 4] + vec[2] * cc[16 + 8];
	float tmp[3];
	tmp[0] = vec[0] - rightDotValue * cc[16 + 0];
	tmp[1] = vec[1] - rightDotValue * cc[16 + 4];
	tmp[2] = vec[2] - rightDotValue * cc[16 + 8];
	float val = d_magnitude(tmp);
	tmp[0] /= val;
	tmp[1] /= val;
	tmp[2] /= val;
	float upDotValue = tmp[0] * cc[16 + 1] + tmp[1] * cc[16 + 5] + tmp[2] * cc[16 + 9];
	float forwardDotValue = tmp[0] * cc[16 + 2] + tmp[1] * cc[16 + 6] * tmp[2] * cc[16 + 10];
	float angle = ugrt_acosf(forwardDotValue);
	return (upDotValue > 0) ? angle : -1.0f * angle;
}

// (d_clamp1, d_material_kd: ugrt_dev.h)

// The primary hit of a pixel, as the kernels that shade one read it.  Each step reads what it names and nothing else, and
// a kernel takes the steps inside its own guards (`in range`, `t_value > 0`, the spot light's none), so a miss reads no
// material and no normal.
struct PrimaryHit {
	const float *__restrict__ dd_normal, *__restrict__ dd_t_value, *__restrict__ dd_dir;
	int *__restrict__ dd_intersect_id;
	const float *__restrict__ d_cam_pos;
	const int *__restrict__ mat_idx;
	const float *__restrict__ mat_list;
	int mat_count, pixelID;

	// the triangle id becomes the material id and is written back; returns it, or -1 where it is out of range.  The
	// reference reads mat_idx[-2] for a miss (shader_kernel.cu:170); a miss keeps its id and shades black.
	__device__ __forceinline__ int material_id() const
	{
		int tri_intersected = dd_intersect_id[pixelID];
		int idx = tri_intersected >= 0 ? mat_idx[tri_intersected] : tri_intersected;
		dd_intersect_id[pixelID] = idx;
		return idx >= 0 && idx < mat_count ? idx : -1;
	}
	__device__ __forceinline__ float t_value() const { return dd_t_value[pixelID]; }
	__device__ __forceinline__ void point(float t, float *p) const
	{
#pragma unroll
		for (int k = 0; k < 3; k++)
			p[k] = d_cam_pos[k] + t * dd_dir[pixelID * 3 + k];
	}
	__device__ __forceinline__ void normal(float *nrm) const
	{
#pragma unroll
		for (int k = 0; k < 3; k++)
			nrm[k] = dd_normal[pixelID * 3 + k];
	}
};

// Kd of the pixel, twice, where the shading reads it from the per-pixel albedo (ugrt_texture_albedo) and not from the
// material: d_material_kd's counterpart
__device__ __forceinline__ void d_albedo_kd(const float *__restrict__ albedo, int pixelID, float *material)
{
#pragma unroll
	for (int k = 0; k < 3; k++) {
		material[k] = albedo[pixelID * 3 + k];
		material[3 + k] = albedo[pixelID * 3 + k];
	}
}

// k_shade's pixel; ALBEDO: Kd is the pixel's albedo[3 pixelID ..] (k_texture_shade), else the material's and albedo is not read
template <bool SPOT, bool ALBEDO>
__device__ __forceinline__ void d_shade_pixel(const CamBlock &cam, unsigned char *__restrict__ d_img,
					      const float *__restrict__ dd_normal, const float *__restrict__ dd_t_value,
					      const float *__restrict__ dd_dir, int *__restrict__ dd_intersect_id,
					      const float *__restrict__ d_cam_pos, const int *__restrict__ mat_idx,
					      const float *__restrict__ mat_list, int mat_count, float *__restrict__ dump,
					      const float *__restrict__ albedo, int pixelID)
{
	float color[3] = { 0.0f, 0.0f, 0.0f }, drop_off = 1.0f, point[3];
	const PrimaryHit hit = { dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list, mat_count, pixelID };
	const int idx = hit.material_id();
	const float t_value = hit.t_value();
	hit.point(t_value, point);
	if (SPOT) {
		float lrd[3];
		lrd[0] = point[0] - cam.cc[0];
		lrd[1] = point[1] - cam.cc[1];
		lrd[2] = point[2] - cam.cc[2];
		D_NORMALIZE(lrd);
		float x = d_along_x(cam, lrd), y = d_along_y(cam, lrd);
		if (dump) {
			dump[pixelID * 2 + 0] = x;
			dump[pixelID * 2 + 1] = y;
		}
		const float qpi = (float)(3.14159265358979323846 / 4);
		drop_off = (x < qpi && x > -qpi && y < qpi && y > -qpi) ? 1.0f : 0.25f;
	}
	if (idx >= 0 && (SPOT || t_value > 0)) {
		float material[6], nrm[3];
		if (ALBEDO)
			d_albedo_kd(albedo, pixelID, material);
		else
			d_material_kd(mat_list, idx, material);
		hit.normal(nrm);
		d_lambert<SPOT>(cam, point, nrm, color, material, drop_off);
		d_clamp1(color);
	}
	d_img[pixelID * 3 + 0] = d_to_u8(color[0]);
	d_img[pixelID * 3 + 1] = d_to_u8(color[1]);
	d_img[pixelID * 3 + 2] = d_to_u8(color[2]);
}

template <bool SPOT>
__global__ __launch_bounds__(PX_THREADS) void k_shade(CamBlock cam, unsigned char *__restrict__ d_img,
						       const float *__restrict__ dd_normal,
						       const float *__restrict__ dd_t_value, const float *__restrict__ dd_dir,
						       int *__restrict__ dd_intersect_id, const float *__restrict__ d_cam_pos,
						       const int *__restrict__ mat_idx, const float *__restrict__ mat_list,
						       int mat_count, float *__restrict__ dump, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	d_shade_pixel<SPOT, false>(cam, d_img, dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list, mat_count,
				   dump, nullptr, p0 + i);
}

// k_shade<false> with the pixel's albedo in the place of the material's Kd
__global__ __launch_bounds__(PX_THREADS) void k_texture_shade(CamBlock cam, unsigned char *__restrict__ d_img,
							      const float *__restrict__ dd_normal,
							      const float *__restrict__ dd_t_value, const float *__restrict__ dd_dir,
							      int *__restrict__ dd_intersect_id, const float *__restrict__ d_cam_pos,
							      const int *__restrict__ mat_idx, const float *__restrict__ mat_list,
							      int mat_count, const float *__restrict__ albedo, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	d_shade_pixel<false, true>(cam, d_img, dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list, mat_count,
				   nullptr, albedo, p0 + i);
}

// the null check of every export that takes the primary arrays
static int shade_args_ok(ugrt_ctx *ctx, const void *a, const void *b, const void *c, const void *d, const void *e,
			 const void *f, const void *g, const void *h, const char *who)
{
	if (!ctx || !a || !b || !c || !d || !e || !f || !g || !h)
		return ugrt_fail(UGRT_EINVAL, "%s: null argument", who);
	return UGRT_OK;
}

// Shader::simpleShade, shader.h:68-86
extern "C" int ugrt_shade_simple(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
				 const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
				 const int *d_mat_idx, const float *d_mat_list, int num_materials)
{
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, "shade_simple");
	if (rc)
		return rc;
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade<false>, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, (float *)nullptr);
}

// k_shade<true> with the pixel's albedo in the place of the material's Kd
__global__ __launch_bounds__(PX_THREADS) void k_texture_shade_spot(CamBlock cam, unsigned char *__restrict__ d_img,
								    const float *__restrict__ dd_normal,
								    const float *__restrict__ dd_t_value, const float *__restrict__ dd_dir,
								    int *__restrict__ dd_intersect_id, const float *__restrict__ d_cam_pos,
								    const int *__restrict__ mat_idx, const float *__restrict__ mat_list,
								    int mat_count, float *__restrict__ dump,
								    const float *__restrict__ albedo, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	d_shade_pixel<true, true>(cam, d_img, dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list, mat_count,
				  dump, albedo, p0 + i);
}

extern "C" int ugrt_texture_shade_spotlight(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
					    const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
					    const int *d_mat_idx, const float *d_mat_list, int num_materials, float *d_dump,
					    const float *d_albedo)
{
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, "texture_shade_spotlight");
	if (rc)
		return rc;
	if (!d_albedo)
		return ugrt_fail(UGRT_EINVAL, "texture_shade_spotlight: null argument");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_texture_shade_spot, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, d_dump, d_albedo);
}

extern "C" int ugrt_texture_shade(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
				 const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
				 const int *d_mat_idx, const float *d_mat_list, int num_materials, const float *d_albedo)
{
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, "texture_shade");
	if (rc)
		return rc;
	if (!d_albedo)
		return ugrt_fail(UGRT_EINVAL, "texture_shade: null argument");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_texture_shade, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, d_albedo);
}

// Shader::spotlight_shade, shader.h:88-113 (d_dump may be null; the reference
// copies it back and prints one line per pixel, shader.h:108-112)
extern "C" int ugrt_shade_spotlight(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal,
				    const float *d_t_value, const float *d_ray_dir, int *d_intersect_id,
				    const float *d_cam_position, const int *d_mat_idx, const float *d_mat_list,
				    int num_materials, float *d_dump)
{
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, "shade_spotlight");
	if (rc)
		return rc;
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade<true>, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, d_dump);
}

// shadow_kernel, shader_kernel.cu:347-359
__global__ __launch_bounds__(PX_THREADS) void k_add_shadows(unsigned char *__restrict__ d_img,
							     const int *__restrict__ is_shadowed, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	if (is_shadowed[pixelID] == 1) {
		d_img[pixelID * 3 + 0] /= 3;
		d_img[pixelID * 3 + 1] /= 3;
		d_img[pixelID * 3 + 2] /= 3;
	}
}

// Shader::add_shadows, shader.h:58-66
extern "C" int ugrt_shade_add_shadows(ugrt_ctx *ctx, unsigned char *d_img, const int *d_is_shadowed)
{
	if (!ctx || !d_img || !d_is_shadowed)
		return ugrt_fail(UGRT_EINVAL, "shade_add_shadows: null argument");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_add_shadows, d_img, d_is_shadowed);
}

// ---------------------------------------------------------------------------
// The integer passes over the image that stand in k_add_shadows' place where a pixel has several occlusion rays (not in
// the reference): each of the pixel's bytes becomes byte * a / b.
// ---------------------------------------------------------------------------
template <class I> __device__ __forceinline__ void d_scale_bytes(unsigned char *__restrict__ d_img, I pixelID, u32 a, u32 b)
{
#pragma unroll
	for (int k = 0; k < 3; k++)
		d_img[pixelID * 3 + k] = (unsigned char)(((u32)d_img[pixelID * 3 + k] * a) / b);
}

static u32 low_bits_of(int num_bits) { return num_bits == 32 ? 0xFFFFFFFFu : (1u << num_bits) - 1u; }

// Ambient occlusion.  bit s of mask = hemisphere ray s is occluded; each byte is scaled by the
// share of open rays.
__global__ __launch_bounds__(PX_THREADS) void k_shade_ao(unsigned char *__restrict__ d_img, const u32 *__restrict__ mask,
							  u32 num_dirs, u32 low_bits, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	const u32 m = mask[pixelID] & low_bits;
	if (m != 0u)
		d_scale_bytes(d_img, pixelID, num_dirs - (u32)__popc(m), num_dirs);
}

extern "C" int ugrt_shade_ao(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_mask, int num_dirs)
{
	if (!ctx || !d_img || !d_mask)
		return ugrt_fail(UGRT_EINVAL, "shade_ao: null argument");
	if (num_dirs < 1 || num_dirs > UGRT_MAX_AO_DIRS)
		return ugrt_fail(UGRT_EINVAL, "shade_ao: num_dirs %d is not in 1..%d", num_dirs, UGRT_MAX_AO_DIRS);
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade_ao, d_img, d_mask, (u32)num_dirs, low_bits_of(num_dirs));
}

// Area lights.  bit s of mask = the shadow ray towards sample s of the light's disk is occluded;
// a byte goes from b (every sample lit) to b / 3 (none).
__global__ __launch_bounds__(PX_THREADS) void k_shade_area(unsigned char *__restrict__ d_img, const u32 *__restrict__ mask,
							    u32 num_samples, u32 low_bits, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	const u32 m = mask[pixelID] & low_bits;
	if (m != 0u) {
		const u32 lit = num_samples - (u32)__popc(m);
		d_scale_bytes(d_img, pixelID, num_samples + 2u * lit, 3u * num_samples);
	}
}

extern "C" int ugrt_shade_area(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_mask, int num_samples)
{
	if (!ctx || !d_img || !d_mask)
		return ugrt_fail(UGRT_EINVAL, "shade_area: null argument");
	if (num_samples < 1 || num_samples > UGRT_MAX_AREA_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "shade_area: num_samples %d is not in 1..%d", num_samples, UGRT_MAX_AREA_SAMPLES);
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade_area, d_img, d_mask, (u32)num_samples, low_bits_of(num_samples));
}

// the pass in the place of k_shade_area behind the edge-aware gather (ugrt_filter.hip): num / den
// is the gathered share of open samples
__global__ __launch_bounds__(PX_THREADS) void k_shade_area_vis(unsigned char *__restrict__ d_img, const u32 *__restrict__ vis,
								u32 num_samples, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const size_t pixelID = (size_t)(p0 + i);
	const u32 num = vis[2 * pixelID], den = vis[2 * pixelID + 1];
	if (den != 0u)
		d_scale_bytes(d_img, pixelID, num_samples * den + 2u * num, 3u * num_samples * den);
}

extern "C" int ugrt_shade_area_vis(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_vis, int num_samples)
{
	if (!ctx || !d_img || !d_vis)
		return ugrt_fail(UGRT_EINVAL, "shade_area_vis: null argument");
	if (num_samples < 1 || num_samples > UGRT_MAX_AREA_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "shade_area_vis: num_samples %d is not in 1..%d", num_samples, UGRT_MAX_AREA_SAMPLES);
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade_area_vis, d_img, d_vis, (u32)num_samples);
}

// the pass in the place of k_shade_ao behind the gather over the hemisphere masks: num / den is the
// gathered share of open rays
__global__ __launch_bounds__(PX_THREADS) void k_shade_ao_vis(unsigned char *__restrict__ d_img, const u32 *__restrict__ vis,
							      u32 num_dirs, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const size_t pixelID = (size_t)(p0 + i);
	const u32 num = vis[2 * pixelID], den = vis[2 * pixelID + 1];
	if (den != 0u)
		d_scale_bytes(d_img, pixelID, num, num_dirs * den);
}

extern "C" int ugrt_ao_shade_vis(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_vis, int num_dirs)
{
	if (!ctx || !d_img || !d_vis)
		return ugrt_fail(UGRT_EINVAL, "ao_shade_vis: null argument");
	if (num_dirs < 1 || num_dirs > UGRT_MAX_AO_DIRS)
		return ugrt_fail(UGRT_EINVAL, "ao_shade_vis: num_dirs %d is not in 1..%d", num_dirs, UGRT_MAX_AO_DIRS);
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade_ao_vis, d_img, d_vis, (u32)num_dirs);
}

// Indirect diffuse light onto the image, behind the shading call: intersect_id holds the
// material index m by then and is only read.  acc is what ugrt_gi_filter wrote, or ugrt_gi_gather's sums themselves (den
// 1): the mean byte of the gathered samples over 255 is the incoming light, Kd * gain of it is added to the pixel.
__global__ __launch_bounds__(PX_THREADS) void k_gi_apply(unsigned char *__restrict__ d_img, const u32 *__restrict__ acc,
							  u32 num_dirs, float gain, const int *__restrict__ intersect_id,
							  const float *__restrict__ mat_list, int mat_count, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const size_t pixelID = (size_t)(p0 + i);
	const int m = intersect_id[pixelID];
	const uint4 sums = *(const uint4 *)(acc + 4 * pixelID);
	if (m < 0 || m >= mat_count || sums.w == 0u)
		return;
	const float over = (float)(255u * num_dirs * sums.w);
	float a[3] = { (float)sums.x / over, (float)sums.y / over, (float)sums.z / over };
#pragma unroll
	for (int k = 0; k < 3; k++)
		a[k] = (mat_list[m * 6 + 3 + k] * gain) * a[k];
	d_clamp1(a);
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const u32 b = (u32)d_img[pixelID * 3 + k] + (u32)d_to_u8(a[k]);
		d_img[pixelID * 3 + k] = (unsigned char)(b > 255u ? 255u : b);
	}
}

extern "C" int ugrt_gi_apply(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_acc, int num_dirs, float gain,
			     const int *d_intersect_id, const float *d_mat_list, int num_materials)
{
	if (!ctx || !d_img || !d_acc || !d_intersect_id || !d_mat_list)
		return ugrt_fail(UGRT_EINVAL, "gi_apply: null argument");
	if (num_dirs < 1 || num_dirs > UGRT_MAX_AO_DIRS)
		return ugrt_fail(UGRT_EINVAL, "gi_apply: num_dirs %d is not in 1..%d", num_dirs, UGRT_MAX_AO_DIRS);
	if (!(gain >= 0.0f))
		return ugrt_fail(UGRT_EINVAL, "gi_apply: gain must be 0 or greater");
	if (((size_t)d_acc & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "gi_apply: d_acc is not 16-byte aligned");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_gi_apply, d_img, (const u32 *)d_acc, (u32)num_dirs, gain, d_intersect_id,
				  d_mat_list, num_materials);
}

// Anti-aliasing, behind the frame's shading and shadow calls: a pixel ugrt_aa_gather has
// supersampled (count word != 0) takes the rounded mean of its samples' bytes, every other pixel stays as it is.
__global__ __launch_bounds__(PX_THREADS) void k_aa_resolve(unsigned char *__restrict__ d_img, const u32 *__restrict__ sum,
							    u32 num_samples, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const size_t pixelID = (size_t)(p0 + i);
	const uint4 sums = *(const uint4 *)(sum + 4 * pixelID);
	if (sums.w == 0u)
		return;
	d_img[pixelID * 3 + 0] = (unsigned char)((sums.x + num_samples / 2u) / num_samples);
	d_img[pixelID * 3 + 1] = (unsigned char)((sums.y + num_samples / 2u) / num_samples);
	d_img[pixelID * 3 + 2] = (unsigned char)((sums.z + num_samples / 2u) / num_samples);
}

extern "C" int ugrt_aa_resolve(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_sum, int num_samples)
{
	if (!ctx || !d_img || !d_sum)
		return ugrt_fail(UGRT_EINVAL, "aa_resolve: null argument");
	if (num_samples < 1 || num_samples > UGRT_MAX_AA_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "aa_resolve: num_samples %d is not in 1..%d", num_samples, UGRT_MAX_AA_SAMPLES);
	if (((size_t)d_sum & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "aa_resolve: d_sum is not 16-byte aligned");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_aa_resolve, d_img, (const u32 *)d_sum, (u32)num_samples);
}

// ---------------------------------------------------------------------------
// several lights (the reference's loop over h_numLights, main.cu:148-203, runs with one and
// its shading kernels index light 0): k_shade<false> and k_add_shadows once per light and the mean of the bytes, in
// one pass over the per-pixel arrays.
// ---------------------------------------------------------------------------
struct LightsIn {
	float pos[3 * UGRT_MAX_LIGHTS]; // by value: uniform over the launch, read from the kernarg segment
	int count;
};

// the lights of export `who`: the range check, then the by-value block
static int lights_in(const char *who, int num_lights, const float *light_pos, LightsIn *lights)
{
	if (num_lights < 1 || num_lights > UGRT_MAX_LIGHTS)
		return ugrt_fail(UGRT_EINVAL, "%s: num_lights %d is not in 1..%d", who, num_lights, UGRT_MAX_LIGHTS);
	*lights = {};
	for (int k = 0; k < 3 * num_lights; k++)
		lights->pos[k] = light_pos[k];
	lights->count = num_lights;
	return UGRT_OK;
}

// k_shade_lights' pixel; ALBEDO as in d_shade_pixel
template <bool ALBEDO>
__device__ __forceinline__ void d_shade_lights_pixel(const CamBlock &cam, unsigned char *__restrict__ d_img,
						     const float *__restrict__ dd_normal, const float *__restrict__ dd_t_value,
						     const float *__restrict__ dd_dir, int *__restrict__ dd_intersect_id,
						     const float *__restrict__ d_cam_pos, const int *__restrict__ mat_idx,
						     const float *__restrict__ mat_list, int mat_count, const LightsIn &lights,
						     const int *__restrict__ is_shadowed, size_t level,
						     const float *__restrict__ albedo, int pixelID)
{
	u32 sum[3] = { 0u, 0u, 0u };
	const PrimaryHit hit = { dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list, mat_count, pixelID };
	const int idx = hit.material_id();
	const float t_value = hit.t_value();
	if (idx >= 0 && t_value > 0) {
		float material[6], point[3], nrm[3], pv[3], nv[3];
		hit.point(t_value, point);
		hit.normal(nrm);
		if (ALBEDO)
			d_albedo_kd(albedo, pixelID, material);
		else
			d_material_kd(mat_list, idx, material);
		d_lambert_view(cam, point, nrm, pv, nv);
		for (int l = 0; l < lights.count; l++) {
			float color[3] = { 0.0f, 0.0f, 0.0f };
			d_lambert_from(cam, &lights.pos[3 * l], pv, nv, color, material);
			d_clamp1(color);
			const bool dark = is_shadowed && is_shadowed[(size_t)l * level + (size_t)pixelID] == 1;
#pragma unroll
			for (int k = 0; k < 3; k++) {
				unsigned char b = d_to_u8(color[k]);
				sum[k] += dark ? (u32)(b / 3) : (u32)b;
			}
		}
	}
	d_img[pixelID * 3 + 0] = (unsigned char)(sum[0] / (u32)lights.count);
	d_img[pixelID * 3 + 1] = (unsigned char)(sum[1] / (u32)lights.count);
	d_img[pixelID * 3 + 2] = (unsigned char)(sum[2] / (u32)lights.count);
}

__global__ __launch_bounds__(PX_THREADS) void k_shade_lights(CamBlock cam, unsigned char *__restrict__ d_img,
							      const float *__restrict__ dd_normal,
							      const float *__restrict__ dd_t_value,
							      const float *__restrict__ dd_dir,
							      int *__restrict__ dd_intersect_id,
							      const float *__restrict__ d_cam_pos,
							      const int *__restrict__ mat_idx,
							      const float *__restrict__ mat_list, int mat_count,
							      LightsIn lights, const int *__restrict__ is_shadowed,
							      size_t level, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	d_shade_lights_pixel<false>(cam, d_img, dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list,
				    mat_count, lights, is_shadowed, level, nullptr, p0 + i);
}

// k_shade_lights with the pixel's albedo in the place of the material's Kd
__global__ __launch_bounds__(PX_THREADS) void k_texture_shade_lights(CamBlock cam, unsigned char *__restrict__ d_img,
								     const float *__restrict__ dd_normal,
								     const float *__restrict__ dd_t_value,
								     const float *__restrict__ dd_dir,
								     int *__restrict__ dd_intersect_id,
								     const float *__restrict__ d_cam_pos,
								     const int *__restrict__ mat_idx,
								     const float *__restrict__ mat_list, int mat_count,
								     LightsIn lights, const int *__restrict__ is_shadowed,
								     size_t level, const float *__restrict__ albedo, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	d_shade_lights_pixel<true>(cam, d_img, dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list,
				   mat_count, lights, is_shadowed, level, albedo, p0 + i);
}

extern "C" int ugrt_texture_shade_lights(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
					const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
					const int *d_mat_idx, const float *d_mat_list, int num_materials, int num_lights,
					const float *light_pos, const int *d_is_shadowed, const float *d_albedo)
{
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, "texture_shade_lights");
	if (rc)
		return rc;
	if (!light_pos || !d_albedo)
		return ugrt_fail(UGRT_EINVAL, "texture_shade_lights: null argument");
	LightsIn lights;
	if ((rc = lights_in("texture_shade_lights", num_lights, light_pos, &lights)))
		return rc;
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_texture_shade_lights, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, lights, d_is_shadowed,
				  (size_t)ctx->cfg.width * (size_t)ctx->cfg.height, d_albedo);
}

extern "C" int ugrt_shade_lights(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
				 const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
				 const int *d_mat_idx, const float *d_mat_list, int num_materials, int num_lights,
				 const float *light_pos, const int *d_is_shadowed)
{
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, "shade_lights");
	if (rc)
		return rc;
	if (!light_pos)
		return ugrt_fail(UGRT_EINVAL, "shade_lights: null argument");
	LightsIn lights;
	if ((rc = lights_in("shade_lights", num_lights, light_pos, &lights)))
		return rc;
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade_lights, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, lights, d_is_shadowed,
				  (size_t)ctx->cfg.width * (size_t)ctx->cfg.height);
}

// shader_kernel.cu:4-44 Noise / InterPolation / PerlinNoise with octaves = 1
__device__ __forceinline__ float d_noise(int x)
{
	u32 ux = (u32)x;
	ux = (ux << 13) ^ ux;
	ux = (ux * (ux * ux * 15731u + 789221u) + 1376312589u) & 0x7fffffffu;
	return (float)(int)ux / 2147483648.0f;
}
__device__ __forceinline__ float d_interp(float a, float b, float c) { return a + (b - a) * c * c * (3 - 2 * c); }
__device__ __forceinline__ float d_perlin(float x, float y, int width, int seed, float periode)
{
	float freq = 1.0f / periode;
	int num = ugrt_f2i((float)width * freq);
	int step_x = ugrt_f2i(x * freq), step_y = ugrt_f2i(y * freq);
	float zone_x = x * freq - (float)step_x;
	float zone_y = y * freq - (float)step_y;
	int noisedata = step_x + step_y * num + seed;
	float a = d_interp(d_noise(noisedata), d_noise(noisedata + 1), zone_x);
	float b = d_interp(d_noise(noisedata + num), d_noise(noisedata + 1 + num), zone_x);
	return d_interp(a, b, zone_y) * 324.0f;
}

// perlin_noise_shade, shader_kernel.cu:505-547
__global__ __launch_bounds__(PX_THREADS) void k_shade_perlin(unsigned char *__restrict__ d_img,
							      const int *__restrict__ dd_intersect_id, int W, int p0,
							      int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	float x = (float)(pixelID % W), y = (float)(pixelID / W);
	float v1 = d_perlin(x, y, 12413, 63, 100.0f), v2 = d_perlin(x, y, 12413, 63, 25.0f);
	float v3 = d_perlin(x, y, 12413, 63, 12.5f), v4 = d_perlin(x, y, 12413, 63, 6.25f);
	float v5 = d_perlin(x, y, 12413, 63, 3.125f), v6 = d_perlin(x, y, 12413, 63, 1.56f);
	float tmp = (float)(ugrt_f2i(v1) + ugrt_f2i(v2 * 0.25f) + ugrt_f2i(v3 * 0.125f) + ugrt_f2i(v4 * 0.0625f) +
			    ugrt_f2i(v5 * 0.03125f) + ugrt_f2i(v6 * 0.0156f));
	int r = ugrt_f2i(tmp * (1 - 0.0f) + 0.0f * 0.0f);
	int g = ugrt_f2i(0.0f * (1 - 0.0f) + tmp * 0.0f);
	int b = ugrt_f2i(0.0f * (1 - tmp) + 0.0f * tmp);
	r = r > 255 ? 255 : r;
	g = g > 255 ? 255 : g;
	b = b > 255 ? 255 : b;
	bool hit = dd_intersect_id[pixelID] >= 0;
	d_img[pixelID * 3 + 0] = hit ? (unsigned char)r : 0;
	d_img[pixelID * 3 + 1] = hit ? (unsigned char)g : 0;
	d_img[pixelID * 3 + 2] = hit ? (unsigned char)b : 0;
}

// Shader::perlinShade, shader.h:115-131 (t, dir and camera are unused by the kernel, as in the reference)
extern "C" int ugrt_shade_perlin(ugrt_ctx *ctx, unsigned char *d_img, const float *d_t_value, const float *d_ray_dir,
				 const float *d_cam_position, const int *d_intersect_id)
{
	(void)d_t_value;
	(void)d_ray_dir;
	(void)d_cam_position;
	if (!ctx || !d_img || !d_intersect_id)
		return ugrt_fail(UGRT_EINVAL, "shade_perlin: null argument");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade_perlin, d_img, d_intersect_id, ctx->cfg.width);
}

// ---------------------------------------------------------------------------
// reflections (not in the reference): the levels' hits blended front to back.  Their rays
// are the secondary-ray generators' (ugrt_bounce.hip), which also says how a frame's levels lie in the arrays.
// ---------------------------------------------------------------------------
struct DepthIn {
	const float *reflect;
	const float *verts;
	const int *tris;
	const float *rays;  // level j at (j-1) * level * 6
	const int *active;  // level j at (j-1) * level
	const float *hit_t;
	const int *hit_id;
	size_t level;       // W*H
	int depth;
	const int *occluded; // level j at (j-1) * level (ugrt_shade_reflect_depth_occluded; otherwise null and never read)
};

// the levels of export `who`: the null and range checks, then the by-value block
static int depth_in(ugrt_ctx *ctx, const char *who, const float *d_reflect, const float *d_vertlist, const int *d_trilist,
		    int depth, const float *d_rays, const int *d_active, const float *d_hit_t, const int *d_hit_id,
		    const int *d_occluded, DepthIn *in)
{
	if (!d_reflect || !d_vertlist || !d_trilist || !d_rays || !d_active || !d_hit_t || !d_hit_id)
		return ugrt_fail(UGRT_EINVAL, "%s: null argument", who);
	if (depth < 1 || depth > UGRT_MAX_REFLECT_DEPTH)
		return ugrt_fail(UGRT_EINVAL, "%s: depth %d outside 1..%d", who, depth, UGRT_MAX_REFLECT_DEPTH);
	*in = { d_reflect, d_vertlist, d_trilist, d_rays, d_active, d_hit_t, d_hit_id,
		(size_t)ctx->cfg.width * (size_t)ctx->cfg.height, depth, d_occluded };
	return UGRT_OK;
}

// The hit of level j, whose arrays lie at q = (j-1) * level + pixel.  False for a miss or a material out of range: it has
// no colour and leaves *kr.  Otherwise *kr is the hit material's reflect (read only where the level goes on, i.e. it is
// in range), `material` its Kd twice, hp the hit point on the level's ray and nn the triangle's unit normal.
// (k_shade_reflect and k_shade_reflect_lights have this body written out, for their speed and register count: see there.)
__device__ __forceinline__ bool d_level_hit(const DepthIn &in, const int *__restrict__ mat_idx,
					    const float *__restrict__ mat_list, int mat_count, size_t q, float *kr,
					    float *material, float *hp, float *nn)
{
	int hid = in.hit_id[q];
	if (hid < 0)
		return false;
	int hm = mat_idx[hid];
	if (hm < 0 || hm >= mat_count)
		return false;
	float t9[9];
	float ht = in.hit_t[q];
	*kr = in.reflect[hm];
	d_stage_triangle(in.verts, in.tris, (u32)hid, 0.0f, 0.0f, 0.0f, t9);
	float *e1 = &t9[3], *e2 = &t9[6];
#pragma unroll
	for (int k = 0; k < 3; k++)
		hp[k] = in.rays[q * 6 + k] + ht * in.rays[q * 6 + 3 + k];
	d_material_kd(mat_list, hm, material);
	D_NORMALIZE(e1);
	D_NORMALIZE(e2);
	D_CROSS(nn, e1, e2);
	D_NORMALIZE(nn);
	return true;
}

// the clamped Lambert colour of level j's hit (as k_shade shades the primary hit); 0 where the level has no colour
__device__ __forceinline__ void d_level_color(const CamBlock &cam, const DepthIn &in, const int *__restrict__ mat_idx,
					      const float *__restrict__ mat_list, int mat_count, size_t q, float *rc,
					      float *kr)
{
	float hmat[6], hp[3], nn[3];
	rc[0] = rc[1] = rc[2] = 0.0f;
	if (!d_level_hit(in, mat_idx, mat_list, mat_count, q, kr, hmat, hp, nn))
		return;
	d_lambert<false>(cam, hp, nn, rc, hmat, 1.0f);
	d_clamp1(rc);
}

// The first bounce alone: (1 - k) * primary colour + k * level 1's colour where the pixel has a level-1
// ray.  These are k_shade_reflect_depth<false>'s bytes at depth 1 (tests/test_reflect_depth.py pins the two).  The frame
// with one bounce, the benchmark's, keeps this kernel and its written-out body: through the depth kernel it shades 2 to 4 %
// slower there, and written with PrimaryHit and d_level_color 0.9 % slower (profiles/shade_refactor.txt).
struct ReflIn {
	const float *reflect;
	const float *verts;
	const int *tris;
	const float *rays;
	const int *active;
	const float *hit_t;
	const int *hit_id;
};

__global__ __launch_bounds__(PX_THREADS) void k_shade_reflect(CamBlock cam, unsigned char *__restrict__ d_img,
							       const float *__restrict__ dd_normal,
							       const float *__restrict__ dd_t_value,
							       const float *__restrict__ dd_dir,
							       int *__restrict__ dd_intersect_id,
							       const float *__restrict__ d_cam_pos,
							       const int *__restrict__ mat_idx,
							       const float *__restrict__ mat_list, int mat_count, ReflIn in,
							       int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	float color[3] = { 0.0f, 0.0f, 0.0f };
	int tri = dd_intersect_id[pixelID];
	int idx = tri >= 0 ? mat_idx[tri] : tri;
	dd_intersect_id[pixelID] = idx;
	if (idx >= 0 && idx < mat_count) {
		float t_value = dd_t_value[pixelID];
		float material[6];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			material[k] = mat_list[idx * 6 + 3 + k];
			material[3 + k] = mat_list[idx * 6 + 3 + k];
		}
		if (t_value > 0) {
			float point[3], nrm[3];
#pragma unroll
			for (int k = 0; k < 3; k++) {
				point[k] = d_cam_pos[k] + t_value * dd_dir[pixelID * 3 + k];
				nrm[k] = dd_normal[pixelID * 3 + k];
			}
			d_lambert<false>(cam, point, nrm, color, material, 1.0f);
#pragma unroll
			for (int k = 0; k < 3; k++)
				color[k] = color[k] > 1.0f ? 1.0f : color[k];
		}
		if (in.active[pixelID]) {
			float kr = in.reflect[idx], rc[3] = { 0.0f, 0.0f, 0.0f };
			int hid = in.hit_id[pixelID];
			if (hid >= 0) {
				int hm = mat_idx[hid];
				if (hm >= 0 && hm < mat_count) {
					float t9[9], nn[3], hp[3], hmat[6];
					float ht = in.hit_t[pixelID];
					d_stage_triangle(in.verts, in.tris, (u32)hid, 0.0f, 0.0f, 0.0f, t9);
					float *e1 = &t9[3], *e2 = &t9[6];
#pragma unroll
					for (int k = 0; k < 3; k++) {
						hp[k] = in.rays[pixelID * 6 + k] + ht * in.rays[pixelID * 6 + 3 + k];
						hmat[k] = mat_list[hm * 6 + 3 + k];
						hmat[3 + k] = mat_list[hm * 6 + 3 + k];
					}
					D_NORMALIZE(e1);
					D_NORMALIZE(e2);
					D_CROSS(nn, e1, e2);
					D_NORMALIZE(nn);
					d_lambert<false>(cam, hp, nn, rc, hmat, 1.0f);
#pragma unroll
					for (int k = 0; k < 3; k++)
						rc[k] = rc[k] > 1.0f ? 1.0f : rc[k];
				}
			}
#pragma unroll
			for (int k = 0; k < 3; k++)
				color[k] = (1.0f - kr) * color[k] + kr * rc[k];
		}
	}
	d_img[pixelID * 3 + 0] = d_to_u8(color[0]);
	d_img[pixelID * 3 + 1] = d_to_u8(color[1]);
	d_img[pixelID * 3 + 2] = d_to_u8(color[2]);
}

// acc = 0, w = 1; level j that goes on (active_{j+1}): acc += (w*(1-k_j))*L_j, w *= k_j; the first level that does not
// (level `depth` at the latest): acc += w*L_j.  At depth 1 this is k_shade_reflect operation for operation.  A
// pixel reads the levels it reaches and no others.  OCC: a level j >= 1 whose hit is occluded (in.occluded) is darkened
// to L_j / 3, the float counterpart of add_shadows' /= 3, before it is weighted.
template <bool OCC>
__global__ __launch_bounds__(PX_THREADS) void k_shade_reflect_depth(CamBlock cam, unsigned char *__restrict__ d_img,
								     const float *__restrict__ dd_normal,
								     const float *__restrict__ dd_t_value,
								     const float *__restrict__ dd_dir,
								     int *__restrict__ dd_intersect_id,
								     const float *__restrict__ d_cam_pos,
								     const int *__restrict__ mat_idx,
								     const float *__restrict__ mat_list, int mat_count,
								     DepthIn in, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	float acc[3] = { 0.0f, 0.0f, 0.0f };
	const PrimaryHit hit = { dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list, mat_count, pixelID };
	const int idx = hit.material_id();
	if (idx >= 0) {
		float color[3] = { 0.0f, 0.0f, 0.0f }, material[6];
		const float t_value = hit.t_value();
		d_material_kd(mat_list, idx, material);
		if (t_value > 0) {
			float point[3], nrm[3];
			hit.point(t_value, point);
			hit.normal(nrm);
			d_lambert<false>(cam, point, nrm, color, material, 1.0f);
			d_clamp1(color);
		}
		float w = 1.0f, kr = in.reflect[idx];
		// level j (0 = the primary hit) goes on when active_{j+1}, which lies at j * level
		for (int j = 0;; j++) {
			const size_t q = (size_t)j * in.level + (size_t)pixelID;
			if (j >= in.depth || !in.active[q]) {
#pragma unroll
				for (int k = 0; k < 3; k++)
					acc[k] = acc[k] + w * color[k];
				break;
			}
#pragma unroll
			for (int k = 0; k < 3; k++)
				acc[k] = acc[k] + (w * (1.0f - kr)) * color[k];
			w = w * kr;
			d_level_color(cam, in, mat_idx, mat_list, mat_count, q, color, &kr);
			if (OCC && in.occluded[q] == 1) {
#pragma unroll
				for (int k = 0; k < 3; k++)
					color[k] = color[k] / 3.0f;
			}
		}
	}
	d_img[pixelID * 3 + 0] = d_to_u8(acc[0]);
	d_img[pixelID * 3 + 1] = d_to_u8(acc[1]);
	d_img[pixelID * 3 + 2] = d_to_u8(acc[2]);
}

// both exports: d_occluded null = ugrt_shade_reflect_depth
static int shade_reflect_depth(ugrt_ctx *ctx, const char *who, unsigned char *d_img, const float *d_normal,
			       const float *d_t_value, const float *d_ray_dir, int *d_intersect_id,
			       const float *d_cam_position, const int *d_mat_idx, const float *d_mat_list,
			       const float *d_reflect, int num_materials, const float *d_vertlist, const int *d_trilist,
			       int depth, const float *d_rays, const int *d_active, const float *d_hit_t, const int *d_hit_id,
			       const int *d_occluded)
{
	DepthIn in;
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, who);
	if (rc || (rc = depth_in(ctx, who, d_reflect, d_vertlist, d_trilist, depth, d_rays, d_active, d_hit_t, d_hit_id,
				 d_occluded, &in)))
		return rc;
	const auto kernel = d_occluded ? k_shade_reflect_depth<true> : k_shade_reflect_depth<false>;
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, kernel, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
				  d_mat_list, num_materials, in);
}

extern "C" int ugrt_shade_reflect(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
				  const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
				  const int *d_mat_idx, const float *d_mat_list, const float *d_reflect, int num_materials,
				  const float *d_vertlist, const int *d_trilist, const float *d_rays, const int *d_active,
				  const float *d_hit_t, const int *d_hit_id)
{
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, "shade_reflect");
	if (rc)
		return rc;
	if (!d_reflect || !d_vertlist || !d_trilist || !d_rays || !d_active || !d_hit_t || !d_hit_id)
		return ugrt_fail(UGRT_EINVAL, "shade_reflect: null argument");
	const ReflIn in = { d_reflect, d_vertlist, d_trilist, d_rays, d_active, d_hit_t, d_hit_id };
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade_reflect, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, in);
}

extern "C" int ugrt_shade_reflect_depth(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal,
					const float *d_t_value, const float *d_ray_dir, int *d_intersect_id,
					const float *d_cam_position, const int *d_mat_idx, const float *d_mat_list,
					const float *d_reflect, int num_materials, const float *d_vertlist,
					const int *d_trilist, int depth, const float *d_rays, const int *d_active,
					const float *d_hit_t, const int *d_hit_id)
{
	return shade_reflect_depth(ctx, "shade_reflect_depth", d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id,
				   d_cam_position, d_mat_idx, d_mat_list, d_reflect, num_materials, d_vertlist, d_trilist, depth,
				   d_rays, d_active, d_hit_t, d_hit_id, nullptr);
}

extern "C" int ugrt_shade_reflect_depth_occluded(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal,
						 const float *d_t_value, const float *d_ray_dir, int *d_intersect_id,
						 const float *d_cam_position, const int *d_mat_idx, const float *d_mat_list,
						 const float *d_reflect, int num_materials, const float *d_vertlist,
						 const int *d_trilist, int depth, const float *d_rays, const int *d_active,
						 const float *d_hit_t, const int *d_hit_id, const int *d_occluded)
{
	if (!d_occluded)
		return ugrt_fail(UGRT_EINVAL, "shade_reflect_depth_occluded: null argument");
	return shade_reflect_depth(ctx, "shade_reflect_depth_occluded", d_img, d_normal, d_t_value, d_ray_dir,
				   d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, d_reflect, num_materials, d_vertlist,
				   d_trilist, depth, d_rays, d_active, d_hit_t, d_hit_id, d_occluded);
}

// Fresnel glass: ugrt_fresnel_gather's sums into the image, in the place of
// ugrt_shade_reflect_depth*.  A pixel that carries a tree (acc[4p + 3] != 0) gets the bytes of its three sums; every other
// pixel what k_shade_reflect_depth gives a pixel without a level-1 ray: acc = 0 + 1 * the primary colour.
__global__ __launch_bounds__(PX_THREADS) void k_fresnel_shade(CamBlock cam, unsigned char *__restrict__ d_img,
							       const float *__restrict__ dd_normal,
							       const float *__restrict__ dd_t_value,
							       const float *__restrict__ dd_dir, int *__restrict__ dd_intersect_id,
							       const float *__restrict__ d_cam_pos, const int *__restrict__ mat_idx,
							       const float *__restrict__ mat_list, int mat_count,
							       const float *__restrict__ sums, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	float acc[3] = { 0.0f, 0.0f, 0.0f };
	const PrimaryHit hit = { dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list, mat_count, pixelID };
	const int idx = hit.material_id();
	const float4 s = *(const float4 *)(sums + 4 * (size_t)pixelID);
	if (s.w != 0.0f) {
		acc[0] = s.x;
		acc[1] = s.y;
		acc[2] = s.z;
	} else if (idx >= 0) {
		float color[3] = { 0.0f, 0.0f, 0.0f }, material[6];
		const float t_value = hit.t_value();
		d_material_kd(mat_list, idx, material);
		if (t_value > 0) {
			float point[3], nrm[3];
			hit.point(t_value, point);
			hit.normal(nrm);
			d_lambert<false>(cam, point, nrm, color, material, 1.0f);
			d_clamp1(color);
		}
#pragma unroll
		for (int k = 0; k < 3; k++)
			acc[k] = acc[k] + 1.0f * color[k];
	}
	d_img[pixelID * 3 + 0] = d_to_u8(acc[0]);
	d_img[pixelID * 3 + 1] = d_to_u8(acc[1]);
	d_img[pixelID * 3 + 2] = d_to_u8(acc[2]);
}

extern "C" int ugrt_fresnel_shade(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
				  const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position, const int *d_mat_idx,
				  const float *d_mat_list, int num_materials, const float *d_acc)
{
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx, d_mat_list,
			       "fresnel_shade");
	if (rc)
		return rc;
	if (!d_acc)
		return ugrt_fail(UGRT_EINVAL, "fresnel_shade: null argument");
	if (((size_t)d_acc & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "fresnel_shade: d_acc is not 16-byte aligned");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_fresnel_shade, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, d_acc);
}

// ---------------------------------------------------------------------------
// reflections under several lights: the depth composition of k_shade_reflect_depth<OCC> and
// k_add_shadows once per light and the mean of the bytes, in one pass.  The level chain (active_{j+1}, k_j, w) does not
// know the light: it is walked once, every level's hit is fetched once and brought to view space once (d_lambert_view),
// and shaded per light from registers (d_lambert_from) into the light's own accumulator.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PX_THREADS) void k_shade_reflect_lights(CamBlock cam, unsigned char *__restrict__ d_img,
								      const float *__restrict__ dd_normal,
								      const float *__restrict__ dd_t_value,
								      const float *__restrict__ dd_dir,
								      int *__restrict__ dd_intersect_id,
								      const float *__restrict__ d_cam_pos,
								      const int *__restrict__ mat_idx,
								      const float *__restrict__ mat_list, int mat_count,
								      DepthIn in, LightsIn lights,
								      const int *__restrict__ is_shadowed, // [count][level], or null
								      const int *__restrict__ occluded, // [depth][count][level], or null
								      int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	u32 sum[3] = { 0u, 0u, 0u };
	const PrimaryHit hit = { dd_normal, dd_t_value, dd_dir, dd_intersect_id, d_cam_pos, mat_idx, mat_list, mat_count, pixelID };
	const int idx = hit.material_id();
	if (idx >= 0) {
		// the hit of the level at hand: lit = it has a colour at all; view-space point and normal; Kd
		float pv[3] = { 0.0f, 0.0f, 0.0f }, nv[3] = { 0.0f, 0.0f, 0.0f }, kd[3];
		const float t_value = hit.t_value();
		bool lit = t_value > 0;
#pragma unroll
		for (int k = 0; k < 3; k++)
			kd[k] = mat_list[idx * 6 + 3 + k];
		if (lit) {
			float point[3], nrm[3];
			hit.point(t_value, point);
			hit.normal(nrm);
			d_lambert_view(cam, point, nrm, pv, nv);
		}
		float acc[UGRT_MAX_LIGHTS][3];
#pragma unroll
		for (int l = 0; l < UGRT_MAX_LIGHTS; l++)
			acc[l][0] = acc[l][1] = acc[l][2] = 0.0f;
		float w = 1.0f, kr = in.reflect[idx];
		// level j (0 = the primary hit) goes on when active_{j+1}, which lies at j * level
		for (int j = 0;; j++) {
			const size_t q = (size_t)j * in.level + (size_t)pixelID;
			const bool goes_on = j < in.depth && in.active[q];
			const float wt = goes_on ? w * (1.0f - kr) : w;
			const float material[6] = { kd[0], kd[1], kd[2], kd[0], kd[1], kd[2] };
			// (the lights unrolled with a uniform guard: acc stays in registers)
#pragma unroll
			for (int l = 0; l < UGRT_MAX_LIGHTS; l++) {
				if (l < lights.count) {
					float color[3] = { 0.0f, 0.0f, 0.0f };
					if (lit) {
						d_lambert_from(cam, &lights.pos[3 * l], pv, nv, color, material);
						const bool dark = j >= 1 && occluded &&
								  occluded[((size_t)(j - 1) * (size_t)lights.count + (size_t)l) * in.level + (size_t)pixelID] == 1;
#pragma unroll
						for (int k = 0; k < 3; k++) {
							color[k] = color[k] > 1.0f ? 1.0f : color[k];
							if (dark)
								color[k] = color[k] / 3.0f;
						}
					}
#pragma unroll
					for (int k = 0; k < 3; k++)
						acc[l][k] = acc[l][k] + wt * color[k];
				}
			}
			if (!goes_on)
				break;
			w = w * kr;
			// level j + 1's hit: d_level_hit written out.  As a call of it the compiler needs 101 to 105 vector
			// registers for this kernel instead of 91, one wave per SIMD fewer (profiles/shade_refactor.txt).
			lit = false;
			int hid = in.hit_id[q];
			if (hid >= 0) {
				int hm = mat_idx[hid];
				if (hm >= 0 && hm < mat_count) {
					float t9[9], nn[3], hp[3];
					float ht = in.hit_t[q];
					kr = in.reflect[hm];
					d_stage_triangle(in.verts, in.tris, (u32)hid, 0.0f, 0.0f, 0.0f, t9);
					float *e1 = &t9[3], *e2 = &t9[6];
#pragma unroll
					for (int k = 0; k < 3; k++) {
						hp[k] = in.rays[q * 6 + k] + ht * in.rays[q * 6 + 3 + k];
						kd[k] = mat_list[hm * 6 + 3 + k];
					}
					D_NORMALIZE(e1);
					D_NORMALIZE(e2);
					D_CROSS(nn, e1, e2);
					D_NORMALIZE(nn);
					d_lambert_view(cam, hp, nn, pv, nv);
					lit = true;
				}
			}
		}
#pragma unroll
		for (int l = 0; l < UGRT_MAX_LIGHTS; l++) {
			if (l < lights.count) {
				const bool dark = is_shadowed && is_shadowed[(size_t)l * in.level + (size_t)pixelID] == 1;
#pragma unroll
				for (int k = 0; k < 3; k++) {
					unsigned char b = d_to_u8(acc[l][k]);
					sum[k] += dark ? (u32)(b / 3) : (u32)b;
				}
			}
		}
	}
	d_img[pixelID * 3 + 0] = (unsigned char)(sum[0] / (u32)lights.count);
	d_img[pixelID * 3 + 1] = (unsigned char)(sum[1] / (u32)lights.count);
	d_img[pixelID * 3 + 2] = (unsigned char)(sum[2] / (u32)lights.count);
}

extern "C" int ugrt_shade_reflect_lights(ugrt_ctx *ctx, unsigned char *d_img, const float *d_normal, const float *d_t_value,
					 const float *d_ray_dir, int *d_intersect_id, const float *d_cam_position,
					 const int *d_mat_idx, const float *d_mat_list, const float *d_reflect, int num_materials,
					 const float *d_vertlist, const int *d_trilist, int depth, const float *d_rays,
					 const int *d_active, const float *d_hit_t, const int *d_hit_id, int num_lights,
					 const float *light_pos, const int *d_is_shadowed, const int *d_occluded)
{
	const char *who = "shade_reflect_lights";
	DepthIn in;
	LightsIn lights;
	int rc = shade_args_ok(ctx, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position, d_mat_idx,
			       d_mat_list, who);
	if (rc)
		return rc;
	if (!light_pos)
		return ugrt_fail(UGRT_EINVAL, "%s: null argument", who);
	if ((rc = depth_in(ctx, who, d_reflect, d_vertlist, d_trilist, depth, d_rays, d_active, d_hit_t, d_hit_id, nullptr, &in)) ||
	    (rc = lights_in(who, num_lights, light_pos, &lights)))
		return rc;
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_shade_reflect_lights, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir,
				  d_intersect_id, d_cam_position, d_mat_idx, d_mat_list, num_materials, in, lights, d_is_shadowed,
				  d_occluded);
}

// ---------------------------------------------------------------------------
// copy_data_transform, transformation_kernel.cu:4-18.  cosf/sinf of the frame's
// angle are evaluated once on the host (the reference evaluates them per vertex
// per component) and enter the kernel as scalars.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PX_THREADS) void k_animate(float *__restrict__ vertexlist,
							 const float *__restrict__ orig_list, int size, int offset,
							 float cr, float sr)
{
	int vert = blockIdx.x * PX_THREADS + threadIdx.x;
	if (vert >= size)
		return;
	float x = ((orig_list[vert * 3 + 0] - 12.0f) / 12.0f);
	float y = ((orig_list[vert * 3 + 1] - 11.0f) / 12.0f);
	float z = ((orig_list[vert * 3 + 2] - 4.5f) / 12.0f);
	vertexlist[(offset + vert) * 3 + 0] = (x * cr - y * sr) * 9.0f + 14.5f;
	vertexlist[(offset + vert) * 3 + 1] = (x * sr + y * cr) * 9.0f + 13.0f;
	vertexlist[(offset + vert) * 3 + 2] = z * 9.0f + 4.0f;
}

// Model::rotate_bunny, scene.h:122-139
extern "C" int ugrt_animate(ugrt_ctx *ctx, float *d_vertlist, const float *d_orig_list, int size, int offset,
			    float rot_factor)
{
	if (!ctx || !d_vertlist || !d_orig_list || size < 0 || offset < 0)
		return ugrt_fail(UGRT_EINVAL, "animate: bad argument");
	if (size == 0)
		return UGRT_OK;
	float c, s;
	ugrt_rot_cos_sin(rot_factor, &c, &s);
	ctx->rec_valid = false; // vertices change: the triangle records are stale until the next grid build
	ctx->geom_gen++;        // and whatever else was kept of the old ones (the uniform grid) is stale for good
	UGRT_HIP(hipSetDevice(ctx->device));
	ugrt_prof_begin(ctx, UGRT_ST_ANIMATE);
	hipLaunchKernelGGL(k_animate, dim3((size + PX_THREADS - 1) / PX_THREADS), dim3(PX_THREADS), 0, ctx->stream,
			   d_vertlist, d_orig_list, size, offset, c, s);
	ugrt_prof_end(ctx, UGRT_ST_ANIMATE);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}
