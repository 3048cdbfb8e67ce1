// ugrt_glossy.hip -- glossy reflections: a lobe of closest-hit rays around the mirror direction (not in the reference;
// DESIGN.md section 6.13).
//
// Spec: an active pixel p of ugrt_reflect_rays' {o, R} sends S rays from o.  Sample s takes the point (u, v) of set k(p)
// of a table of points in the unit disk, the spread a of the primary hit's material, and the direction
// D = d_hemi_dir(normalize(R), a*u, a*v, 1): the mirror direction tilted by at most atan(a).  A D that would enter the
// surface (D.n < 0, n of ugrt_ao_rays) is mirrored back over it.  From {o, D} on everything is ugrt_gi_gather's, word for
// word: the closest hit below `radius` (d_closest_walk<., true>), d_hit_color, the division by 3 where the any-hit walk
// flags the occlusion ray to the shadow light, d_to_u8, the sum across the pixel's S lanes and one 16-byte store.
//   * the index space is ugrt_trace_dda_any_area's (pixel group, sample): the S rays of a pixel in neighbouring lanes.
//     The lobe is narrow, so those lanes walk the same cells and test the same lists;
//   * the point table and the words that only the code around the walks reads are staged in LDS (ugrt_gi.hip's reason:
//     kept in scalar registers over both walks they spill);
//   * groups of pixels are drawn from a ticket.
// ugrt_glossy_apply blends the mean byte of the lobe into the image with the material's reflect as the weight.
#include "ugrt_walks.h"

// words staged in LDS behind the table: cc[16..27], the context's light, the shadow light, eps; then (GL_LATE_F on) as
// 32-bit halves the material arrays, their count, `sum`, the ticket, the normals' rays, the primary ids and the spreads
#define GL_LATE_F 19
#define GL_LATE_W 15
#define GL_LATE 36

// ugrt_dda.hip
int ugrt_dda_prepare(ugrt_ctx *ctx, const DGrid &g, const int *d_active, float *d_hit_t, int *d_hit_id, const u32 *d_span,
		     bool with_bitmap, u32 *chunk, u32 **list_out, u32 **dcount_out);

struct GlossyArg {
	const float *points; // device memory [set_w * set_h][S][2] points of the unit disk
	int count;           // S
	u32 set_w, set_h;    // 1..4 each
	u32 width;           // of the full image
	float radius;
	const float *orays;  // {o', n} of ugrt_ao_rays: n is read
	const int *ids;      // the primary hits' triangles
	const float *spread; // per material
	const int *mat_idx;
	const float *mat_list;
	int mat_count;
	float light[3];      // the shadow light (SHADOW only)
	float eps;
};

// (dynamic LDS, its base 16-byte aligned: the point table)
extern __shared__ __attribute__((aligned(16))) float s_gl_points[];

__device__ __forceinline__ const void *d_gl_ptr(const u32 *w, int i)
{
	return (const void *)(((size_t)w[i + 1] << 32) | (size_t)w[i]);
}

// a point's coordinate: clamped to [-1, 1], a NaN counts as 0
__device__ __forceinline__ float d_gl_coord(float x)
{
	x = x == x ? x : 0.0f;
	return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
}

// `sum` of the band was cleared in stream order before the launch: only the words of active pixels are written
template <bool REC, bool SHADOW>
__global__ __launch_bounds__(64) void k_glossy_gather(DGrid g, const u32 *__restrict__ value_list, const u32 *__restrict__ span,
						      const u32 *__restrict__ offset, const u32 *__restrict__ bitmap,
						      const float *__restrict__ verts, const int *__restrict__ tris,
						      const float4 *__restrict__ rec, const float *__restrict__ rays,
						      const u32 *__restrict__ list, const u32 *__restrict__ count_p,
						      const GlossyArg a, const CamBlock cam, u32 *__restrict__ sum, u32 PPW, u32 COOP,
						      u32 *__restrict__ ticket)
{
	const int lane = threadIdx.x;
	const u32 count = *count_p;
	const u32 S = (u32)a.count;
	{
		// the table in LDS: 2 * K * S floats, float4 per lane while four are left (a 16-byte aligned table), then single floats
		const u32 total = 2u * S * a.set_w * a.set_h;
		u32 done = 0u;
		if (((size_t)a.points & 15u) == 0u) {
			for (u32 i = 4u * (u32)lane; i + 4u <= total; i += 256u)
				*(float4 *)(s_gl_points + i) = *(const float4 *)(a.points + i);
			done = total & ~3u;
		}
		for (u32 i = done + (u32)lane; i < total; i += 64u)
			s_gl_points[i] = a.points[i];
		float *late = s_gl_points + ((total + 3u) & ~3u);
#pragma unroll
		for (int i = 0; i < GL_LATE_F; i++) {
			const float v = i < 12 ? cam.cc[16 + i] : (i < 15 ? cam.light[i - 12] : (i < 18 ? a.light[i - 15] : a.eps));
			if (lane == 0)
				late[i] = v;
		}
		if (lane == 0) {
			u32 *w = (u32 *)late + GL_LATE_F;
			w[0] = (u32)(size_t)a.mat_idx;
			w[1] = (u32)((size_t)a.mat_idx >> 32);
			w[2] = (u32)(size_t)a.mat_list;
			w[3] = (u32)((size_t)a.mat_list >> 32);
			w[4] = (u32)a.mat_count;
			w[5] = (u32)(size_t)sum;
			w[6] = (u32)((size_t)sum >> 32);
			w[7] = (u32)(size_t)ticket;
			w[8] = (u32)((size_t)ticket >> 32);
			w[9] = (u32)(size_t)a.orays;
			w[10] = (u32)((size_t)a.orays >> 32);
			w[11] = (u32)(size_t)a.ids;
			w[12] = (u32)((size_t)a.ids >> 32);
			w[13] = (u32)(size_t)a.spread;
			w[14] = (u32)((size_t)a.spread >> 32);
		}
		__syncthreads();
	}
	// groups of PPW pixels, the first gridDim.x by workgroup id, the others drawn from the ticket
	for (u32 grp = blockIdx.x; grp * PPW < count;) {
		u32 apix, asmp;
		d_area_lane(lane, S, apix, asmp);
		const u32 slot = grp * PPW + apix;
		bool inb = apix < PPW && slot < count;
		const int p = inb ? (int)list[slot] : 0;
		inb = inb && p != -1; // (padding: k_dda_prepare)
		{
			// the lane's sample becomes its index into the table: set k(p), sample asmp
			u32 width = a.width, set_w = a.set_w, set_h = a.set_h;
			asm volatile("" : "+s"(width), "+s"(set_w), "+s"(set_h));
			const u32 y = (u32)p / width, x = (u32)p - y * width;
			asmp += ((y % set_h) * set_w + x % set_w) * S;
		}
		const float *late = s_gl_points + ((2u * S * a.set_w * a.set_h + 3u) & ~3u);
		const u32 *late_w = (const u32 *)late + GL_LATE_F;
		// ---- phase A: the closest hit of {o, D} below radius (k_trace_dda_ray's loop) ----
		float o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 }, res_t;
		int res_id;
		if (inb) {
			const float *orays = (const float *)d_gl_ptr(late_w, 9);
			const int *ids = (const int *)d_gl_ptr(late_w, 11);
			float R[3], nrm[3];
#pragma unroll
			for (int k = 0; k < 3; k++) {
				o[k] = rays[p * 6 + k];
				R[k] = rays[p * 6 + 3 + k];
				nrm[k] = orays[p * 6 + 3 + k];
			}
			// the spread of the primary hit's material: NaN, zeros and negative values count as 0, values above the maximum as it
			float spr = 0.0f;
			const int id = ids[p];
			if (id >= 0) {
				const int m = ((const int *)d_gl_ptr(late_w, 0))[id];
				if (m >= 0 && m < (int)late_w[4]) {
					const float sp = ((const float *)d_gl_ptr(late_w, 13))[m];
					if (sp > 0.0f)
						spr = sp > UGRT_MAX_GLOSSY_SPREAD ? UGRT_MAX_GLOSSY_SPREAD : sp;
				}
			}
			const float u = d_gl_coord(s_gl_points[2u * asmp]), v = d_gl_coord(s_gl_points[2u * asmp + 1u]);
			const float len2 = (R[0] * R[0] + R[1] * R[1]) + R[2] * R[2];
			const float inv = 1.0f / __builtin_sqrtf(len2);
#pragma unroll
			for (int k = 0; k < 3; k++)
				R[k] = R[k] * inv;
			d_hemi_dir(R, spr * u, spr * v, 1.0f, d);
			// the horizon: a sample that would enter the surface is mirrored back over it
			const float c = (d[0] * nrm[0] + d[1] * nrm[1]) + d[2] * nrm[2];
			if (c < 0.0f) {
#pragma unroll
				for (int k = 0; k < 3; k++)
					d[k] = d[k] - (2.0f * c) * nrm[k];
			}
		}
		d_closest_walk<REC, true>(g, value_list, span, offset, bitmap, verts, tris, rec, o, d, a.radius, inb, COOP, lane, res_t,
					  res_id);
		// ---- the hit's colour and its occlusion ray, formed here so that phase B holds neither o nor D ----
		float L[3] = { 0.0f, 0.0f, 0.0f }, o2[3] = { 0.0f, 0.0f, 0.0f }, d2[3] = { 0.0f, 0.0f, 0.0f };
		bool lit_hit = false; // a hit with a colour: a miss and a material out of range stay 0, occluded or not
		if (res_id >= 0) {
			const int *mat_idx = (const int *)d_gl_ptr(late_w, 0);
			const float *mat_list = (const float *)d_gl_ptr(late_w, 2);
			const int hm = mat_idx[res_id];
			if (hm >= 0 && hm < (int)late_w[4]) {
				float t9[9];
				d_stage_triangle(verts, tris, (u32)res_id, 0.0f, 0.0f, 0.0f, t9);
				if constexpr (SHADOW) {
					// k_occlusion_rays' ray: d_reflect_ray's origin, the direction light - o'' not normalised
					float out[6];
					d_reflect_ray(o, d, res_t, t9, late[18], out);
#pragma unroll
					for (int k = 0; k < 3; k++) {
						o2[k] = out[k];
						d2[k] = late[15 + k] - out[k];
					}
				}
				CamBlock view; // (d_lambert reads the rotation and the light, nothing else)
#pragma unroll
				for (int i = 0; i < 12; i++)
					view.cc[16 + i] = late[i];
#pragma unroll
				for (int k = 0; k < 3; k++)
					view.light[k] = late[12 + k];
				d_hit_color(view, o, d, res_t, t9, mat_list, hm, L);
				lit_hit = true;
			}
		}
		// ---- phase B: is the shadow light hidden from the hit (k_trace_dda_any's loop, the light at t = 1) ----
		if constexpr (SHADOW) {
			const bool occ = d_any_walk<REC>(g, value_list, span, offset, bitmap, verts, tris, rec, o2, d2, 1.0f, lit_hit,
							    COOP, lane);
			if (occ) {
#pragma unroll
				for (int k = 0; k < 3; k++)
					L[k] = L[k] / 3.0f;
			}
		}
		// ---- bytes, summed over the pixel's S neighbouring lanes (idle and padding lanes hold zeros) ----
		u32 rg = 0u, bb = 0u; // r | g << 16, b: a sum is at most 32 * 255 < 2^13
		if (lit_hit) {
			rg = (u32)d_to_u8(L[0]) | ((u32)d_to_u8(L[1]) << 16);
			bb = (u32)d_to_u8(L[2]);
		}
		d_area_lane(lane, S, apix, asmp);
		// lane i of a pixel holds the sum over its lanes i .. min(i + 2 * off - 1, S - 1) after the step with `off`
		for (u32 off = 1u; off < S; off <<= 1) {
			const u32 org = (u32)__shfl_down((int)rg, off), obb = (u32)__shfl_down((int)bb, off);
			if (asmp + off < S) {
				rg += org;
				bb += obb;
			}
		}
		if (inb && asmp == 0u) {
			u32 *out = (u32 *)d_gl_ptr(late_w, 5);
			*(uint4 *)(out + 4u * (size_t)p) = make_uint4(rg & 0xFFFFu, rg >> 16, bb, 1u);
		}
		if (lane == 0)
			grp = gridDim.x + atomicAdd((u32 *)d_gl_ptr(late_w, 7), 1u);
		grp = (u32)__builtin_amdgcn_readfirstlane((int)grp);
	}
}

extern "C" int ugrt_glossy_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
				  const float *d_vertlist, const int *d_trilist, const float *d_rays, const int *d_active,
				  const float *d_orays, const int *d_intersect_id, const int *d_mat_idx, const float *d_spread,
				  int num_samples, int set_w, int set_h, const float *d_points, float radius, const float *d_mat_list,
				  int num_materials, const float *shadow_light, float eps, unsigned *d_sum)
{
	if (!ctx || !d_value_list || !d_span || !d_offset || !d_vertlist || !d_trilist || !d_rays || !d_active || !d_orays ||
	    !d_intersect_id || !d_mat_idx || !d_spread || !d_points || !d_mat_list || !d_sum)
		return ugrt_fail(UGRT_EINVAL, "glossy_gather: null argument");
	if (num_samples < 1 || num_samples > UGRT_MAX_GLOSSY_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "glossy_gather: num_samples %d is not in 1..%d", num_samples, UGRT_MAX_GLOSSY_SAMPLES);
	if (set_w < 1 || set_w > UGRT_MAX_AO_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "glossy_gather: set_w %d is not in 1..%d", set_w, UGRT_MAX_AO_SET_TILE);
	if (set_h < 1 || set_h > UGRT_MAX_AO_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "glossy_gather: set_h %d is not in 1..%d", set_h, UGRT_MAX_AO_SET_TILE);
	if (!(radius > 0.0f))
		return ugrt_fail(UGRT_EINVAL, "glossy_gather: radius must be greater than 0");
	if (eps != eps)
		return ugrt_fail(UGRT_EINVAL, "glossy_gather: eps is not a number");
	if (num_materials < 1)
		return ugrt_fail(UGRT_EINVAL, "glossy_gather: num_materials %d is less than 1", num_materials);
	if (((size_t)d_sum & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "glossy_gather: d_sum is not 16-byte aligned");
	Grid &G = ctx->grid[UGRT_GRID_UNIFORM];
	if (!G.valid)
		return ugrt_fail(UGRT_EINVAL, "trace_dda: build the uniform grid first (it defines the cell geometry)");
	UGRT_HIP(hipSetDevice(ctx->device));
	const DGrid g = ugrt_dgrid_of(G);
	const float4 *rec = ugrt_trirec_of(ctx, d_vertlist, d_trilist);
	GlossyArg a = {};
	a.points = d_points;
	a.count = num_samples;
	a.set_w = (u32)set_w;
	a.set_h = (u32)set_h;
	a.width = (u32)ctx->cfg.width;
	a.radius = radius;
	a.orays = d_orays;
	a.ids = d_intersect_id;
	a.spread = d_spread;
	a.mat_idx = d_mat_idx;
	a.mat_list = d_mat_list;
	a.mat_count = num_materials;
	for (int k = 0; k < 3; k++)
		a.light[k] = shadow_light ? shadow_light[k] : 0.0f;
	a.eps = eps;
	// launch shape (ugrt_ctx_set_option; no effect on results): ugrt_trace_dda_any_area's
	const u32 L = ctx->opt[UGRT_OPT_ANY_RPW] > 0 ? (ctx->opt[UGRT_OPT_ANY_RPW] < 64 ? (u32)ctx->opt[UGRT_OPT_ANY_RPW] : 64u) : 64u;
	const u32 PPW = L / (u32)num_samples > 0u ? L / (u32)num_samples : 1u;
	const u32 COOP = ctx->opt[UGRT_OPT_ANY_COOP] > 0 ? (u32)ctx->opt[UGRT_OPT_ANY_COOP] : 8u;
	// at most 8 * 16 * 32 bytes of points (4 KiB) and the late words
	const size_t lds = (((size_t)8 * (size_t)(set_w * set_h * num_samples) + 15u) & ~(size_t)15u) + ((GL_LATE * 4 + 15) & ~15);
	// One prepare launch and one ray list, as ugrt_gi_gather takes them: the form that writes no hit defaults is handed the
	// band's own words to clear one int per pixel into, and the whole band is cleared behind it, in stream order.
	u32 *list, *dcount;
	ugrt_prof_begin(ctx, UGRT_ST_WORKLIST);
	const int rc = ugrt_dda_prepare(ctx, g, d_active, nullptr, (int *)d_sum + (size_t)3 * (size_t)ctx->p0, d_span, true, nullptr,
					&list, &dcount);
	hipError_t he = hipSuccess;
	if (!rc)
		he = hipMemsetAsync(d_sum + (size_t)4 * (size_t)ctx->p0, 0, (size_t)ctx->npix * 16u, ctx->stream);
	ugrt_prof_end(ctx, UGRT_ST_WORKLIST);
	if (rc)
		return rc;
	UGRT_HIP(he);
	int blocks = launch_blocks_for((u32)ctx->npix / PPW + 1u);
	if (ctx->opt[UGRT_OPT_DDA_BLOCKS] > 0 && blocks > ctx->opt[UGRT_OPT_DDA_BLOCKS])
		blocks = ctx->opt[UGRT_OPT_DDA_BLOCKS];
	const auto kernel = shadow_light ? (rec ? k_glossy_gather<true, true> : k_glossy_gather<false, true>)
					 : (rec ? k_glossy_gather<true, false> : k_glossy_gather<false, false>);
	ugrt_prof_begin(ctx, UGRT_ST_TRACE_DDA);
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, ctx->stream, g, d_value_list, d_span, d_offset,
			   (const u32 *)ctx->ubitmap.p, d_vertlist, d_trilist, rec, d_rays, (const u32 *)list, (const u32 *)dcount, a,
			   ctx->cam, d_sum, PPW, COOP, ctx->d_small + UGRT_DSMALL_TICKET);
	ugrt_prof_end(ctx, UGRT_ST_TRACE_DDA);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}

// The lobe's mean onto the image, directly behind the shading call: intersect_id holds the
// material index m by then and is only read.  acc is what ugrt_gi_filter wrote over the glossy sums, or the sums themselves
// (den 1).  The byte becomes the blend the mirror frame makes on floats, here on bytes: (1 - k) * b + k * mean, rounded.
__global__ __launch_bounds__(PX_THREADS) void k_glossy_apply(unsigned char *__restrict__ d_img, const u32 *__restrict__ acc,
							      u32 num_samples, const int *__restrict__ intersect_id,
							      const float *__restrict__ reflect, int mat_count, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const size_t pixelID = (size_t)(p0 + i);
	const int m = intersect_id[pixelID];
	const uint4 sums = *(const uint4 *)(acc + 4 * pixelID);
	if (m < 0 || m >= mat_count || sums.w == 0u)
		return;
	float k = reflect[m];
	if (!(k > 0.0f))
		return;
	k = k > 1.0f ? 1.0f : k;
	const float over = (float)(num_samples * sums.w);
	const float mean[3] = { (float)sums.x / over, (float)sums.y / over, (float)sums.z / over };
#pragma unroll
	for (int c = 0; c < 3; c++) {
		const float b = (float)d_img[pixelID * 3 + c];
		const int v = ugrt_floor2i(((1.0f - k) * b + k * mean[c]) + 0.5f);
		d_img[pixelID * 3 + c] = (unsigned char)(v > 255 ? 255 : v);
	}
}

extern "C" int ugrt_glossy_apply(ugrt_ctx *ctx, unsigned char *d_img, const unsigned *d_acc, int num_samples,
				 const int *d_intersect_id, const float *d_reflect, int num_materials)
{
	if (!ctx || !d_img || !d_acc || !d_intersect_id || !d_reflect)
		return ugrt_fail(UGRT_EINVAL, "glossy_apply: null argument");
	if (num_samples < 1 || num_samples > UGRT_MAX_GLOSSY_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "glossy_apply: num_samples %d is not in 1..%d", num_samples, UGRT_MAX_GLOSSY_SAMPLES);
	if (((size_t)d_acc & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "glossy_apply: d_acc is not 16-byte aligned");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_glossy_apply, d_img, (const u32 *)d_acc, (u32)num_samples, d_intersect_id,
				  d_reflect, num_materials);
}
