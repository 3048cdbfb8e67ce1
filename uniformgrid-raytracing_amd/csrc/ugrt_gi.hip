// ugrt_gi.hip -- indirect diffuse light: a closest-hit hemisphere gather per pixel (not in the reference; DESIGN.md
// section 6.10).
//
// Spec: pixel p sends the S rays of ugrt_trace_dda_any_hemi_sets -- {o', n} of ugrt_ao_rays, set k(p) of the direction
// table, d_hemi_dir's basis -- and each ray asks ugrt_trace_dda's question, "what is the first thing there", no further
// than `radius`.  The hit is shaded as a level's hit is shaded (d_level_color's Lambert term under the context's light),
// darkened to a third where the hit does not see the shadow light (the any-hit walk of section 6.2 on the occlusion ray
// of ugrt_occlusion_rays), turned into bytes, and the bytes of a pixel's S rays are summed.  Per sample the composition
// of existing calls is three launches and a 24-byte ray; here the ray, its hit, the occlusion ray and the colour stay in
// registers of one lane and only 16 bytes per pixel are written.
//   * the index space is ugrt_trace_dda_any_area's (pixel group, sample): the S rays of a pixel in neighbouring lanes;
//   * phase A is k_trace_dda_ray's loop -- d_dda_clip, d_dda_axes, d_dda_step, the dims-sum guard, list order, strict
//     acceptance, the 64-bit wave minimum of the cooperative rounds -- planned WALK_AHEAD cells at a time with the any-hit
//     kernel's bitmap look-up in front of the headers; best_t starts at min(3.0e38f, radius) and the walk also ends behind
//     a cell whose exit parameter is not below radius (d_closest_walk<., true> of ugrt_walks.h, shared with ugrt_aa.hip);
//   * behind it a lane forms what the later phases need from {o, D, t, id} (the occlusion origin, the colour) and lets
//     those go: phase B, k_trace_dda_any's loop with t_max = 1 (d_any_walk of ugrt_walks.h), holds its own ray only;
//   * the three byte sums are added across the pixel's S lanes and stored with the count word by the pixel's first lane.
#include "ugrt_walks.h"

// words staged in LDS behind the table, which only the code between and behind the walks reads: cc[16..27], the
// context's light, the shadow light, eps; then (GI_LATE_F on) the material arrays, their count, `sum` and the ticket as 32-bit halves
#define GI_LATE_F 19
#define GI_LATE 28

// ugrt_dda.hip
int ugrt_dda_prepare(ugrt_ctx *ctx, const DGrid &g, const int *d_active, float *d_hit_t, int *d_hit_id, const u32 *d_span,
		     bool with_bitmap, u32 *chunk, u32 **list_out, u32 **dcount_out);

struct GiArg {
	const float *dirs;  // device memory [set_w * set_h][S][3] local directions
	int count;          // S
	u32 set_w, set_h;   // 1..4 each
	u32 width;          // of the full image
	float radius;
	const int *mat_idx;
	const float *mat_list;
	int mat_count;
	float light[3];     // the shadow light (SHADOW only)
	float eps;
};

// (dynamic LDS, its base 16-byte aligned: the direction table)
extern __shared__ __attribute__((aligned(16))) float s_gi_dirs[];

// `sum` of the band was cleared in stream order before the launch: only the words of active pixels are written
template <bool REC, bool SHADOW>
__global__ __launch_bounds__(64) void k_gi_gather(DGrid g, const u32 *__restrict__ value_list, const u32 *__restrict__ span,
						  const u32 *__restrict__ offset, const u32 *__restrict__ bitmap,
						  const float *__restrict__ verts, const int *__restrict__ tris,
						  const float4 *__restrict__ rec, const float *__restrict__ rays,
						  const u32 *__restrict__ list, const u32 *__restrict__ count_p, const GiArg a,
						  const CamBlock cam, u32 *__restrict__ sum, u32 PPW, u32 COOP,
						  u32 *__restrict__ ticket)
{
	const int lane = threadIdx.x;
	const u32 count = *count_p;
	const u32 S = (u32)a.count;
	{
		// the table in LDS: 3 * K * S floats, float4 per lane while four are left (a 16-byte aligned table), then single floats
		const u32 total = 3u * S * a.set_w * a.set_h;
		u32 done = 0u;
		if (((size_t)a.dirs & 15u) == 0u) {
			for (u32 i = 4u * (u32)lane; i + 4u <= total; i += 256u)
				*(float4 *)(s_gi_dirs + i) = *(const float4 *)(a.dirs + i);
			done = total & ~3u;
		}
		for (u32 i = done + (u32)lane; i < total; i += 64u)
			s_gi_dirs[i] = a.dirs[i];
		// What only the code between and behind the walks reads -- the view rotation, the two lights, eps, the material
		// arrays, `sum`, the ticket -- goes behind the table (uniform indices: scalar loads): kept in scalar registers over
		// both walks it cost 12 to 23 spilled ones.
		float *late = s_gi_dirs + ((total + 3u) & ~3u);
#pragma unroll
		for (int i = 0; i < GI_LATE_F; i++) {
			const float v = i < 12 ? cam.cc[16 + i] : (i < 15 ? cam.light[i - 12] : (i < 18 ? a.light[i - 15] : a.eps));
			if (lane == 0)
				late[i] = v;
		}
		if (lane == 0) {
			u32 *w = (u32 *)late + GI_LATE_F;
			w[0] = (u32)(size_t)a.mat_idx;
			w[1] = (u32)((size_t)a.mat_idx >> 32);
			w[2] = (u32)(size_t)a.mat_list;
			w[3] = (u32)((size_t)a.mat_list >> 32);
			w[4] = (u32)a.mat_count;
			w[5] = (u32)(size_t)sum;
			w[6] = (u32)((size_t)sum >> 32);
			w[7] = (u32)(size_t)ticket;
			w[8] = (u32)((size_t)ticket >> 32);
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
		// ---- phase A: the closest hit of {o, D} below radius (k_trace_dda_ray's loop) ----
		float o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 }, res_t;
		int res_id;
		if (inb) {
			float nrm[3];
#pragma unroll
			for (int k = 0; k < 3; k++) {
				o[k] = rays[p * 6 + k];
				nrm[k] = rays[p * 6 + 3 + k];
			}
			d_hemi_dir(nrm, s_gi_dirs[3u * asmp], s_gi_dirs[3u * asmp + 1u], s_gi_dirs[3u * asmp + 2u], d);
		}
		d_closest_walk<REC, true>(g, value_list, span, offset, bitmap, verts, tris, rec, o, d, a.radius, inb, COOP, lane, res_t,
					  res_id);
		// ---- the hit's colour and its occlusion ray, formed here so that phase B holds neither o nor D ----
		float L[3] = { 0.0f, 0.0f, 0.0f }, o2[3] = { 0.0f, 0.0f, 0.0f }, d2[3] = { 0.0f, 0.0f, 0.0f };
		bool lit_hit = false; // a hit with a colour: a miss and a material out of range stay 0, occluded or not
		const float *late = s_gi_dirs + ((3u * S * a.set_w * a.set_h + 3u) & ~3u);
		const u32 *late_w = (const u32 *)late + GI_LATE_F;
		if (res_id >= 0) {
			const int *mat_idx = (const int *)(((size_t)late_w[1] << 32) | (size_t)late_w[0]);
			const float *mat_list = (const float *)(((size_t)late_w[3] << 32) | (size_t)late_w[2]);
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
			u32 *out = (u32 *)(((size_t)late_w[6] << 32) | (size_t)late_w[5]);
			*(uint4 *)(out + 4u * (size_t)p) = make_uint4(rg & 0xFFFFu, rg >> 16, bb, 1u);
		}
		if (lane == 0)
			grp = gridDim.x + atomicAdd((u32 *)(((size_t)late_w[8] << 32) | (size_t)late_w[7]), 1u);
		grp = (u32)__builtin_amdgcn_readfirstlane((int)grp);
	}
}

extern "C" int ugrt_gi_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
			      const float *d_vertlist, const int *d_trilist, const float *d_orays, const int *d_oactive,
			      int num_dirs, int set_w, int set_h, const float *d_dirs, float radius, const int *d_mat_idx,
			      const float *d_mat_list, int num_materials, const float *shadow_light, float eps, unsigned *d_sum)
{
	if (!ctx || !d_value_list || !d_span || !d_offset || !d_vertlist || !d_trilist || !d_orays || !d_oactive || !d_dirs ||
	    !d_mat_idx || !d_mat_list || !d_sum)
		return ugrt_fail(UGRT_EINVAL, "gi_gather: null argument");
	if (num_dirs < 1 || num_dirs > UGRT_MAX_AO_DIRS)
		return ugrt_fail(UGRT_EINVAL, "gi_gather: num_dirs %d is not in 1..%d", num_dirs, UGRT_MAX_AO_DIRS);
	if (set_w < 1 || set_w > UGRT_MAX_AO_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "gi_gather: set_w %d is not in 1..%d", set_w, UGRT_MAX_AO_SET_TILE);
	if (set_h < 1 || set_h > UGRT_MAX_AO_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "gi_gather: set_h %d is not in 1..%d", set_h, UGRT_MAX_AO_SET_TILE);
	if (set_w * set_h * num_dirs > UGRT_MAX_AO_SET_DIRS)
		return ugrt_fail(UGRT_EINVAL, "gi_gather: set_w * set_h * num_dirs = %d is more than %d", set_w * set_h * num_dirs,
				 UGRT_MAX_AO_SET_DIRS);
	if (!(radius > 0.0f))
		return ugrt_fail(UGRT_EINVAL, "gi_gather: radius must be greater than 0");
	if (eps != eps)
		return ugrt_fail(UGRT_EINVAL, "gi_gather: eps is not a number");
	if (num_materials < 1)
		return ugrt_fail(UGRT_EINVAL, "gi_gather: num_materials %d is less than 1", num_materials);
	if (((size_t)d_sum & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "gi_gather: d_sum is not 16-byte aligned");
	Grid &G = ctx->grid[UGRT_GRID_UNIFORM];
	if (!G.valid)
		return ugrt_fail(UGRT_EINVAL, "trace_dda: build the uniform grid first (it defines the cell geometry)");
	UGRT_HIP(hipSetDevice(ctx->device));
	const DGrid g = ugrt_dgrid_of(G);
	const float4 *rec = ugrt_trirec_of(ctx, d_vertlist, d_trilist);
	GiArg a = {};
	a.dirs = d_dirs;
	a.count = num_dirs;
	a.set_w = (u32)set_w;
	a.set_h = (u32)set_h;
	a.width = (u32)ctx->cfg.width;
	a.radius = radius;
	a.mat_idx = d_mat_idx;
	a.mat_list = d_mat_list;
	a.mat_count = num_materials;
	for (int k = 0; k < 3; k++)
		a.light[k] = shadow_light ? shadow_light[k] : 0.0f;
	a.eps = eps;
	// launch shape (ugrt_ctx_set_option; no effect on results): ugrt_trace_dda_any_area's
	const u32 L = ctx->opt[UGRT_OPT_ANY_RPW] > 0 ? (ctx->opt[UGRT_OPT_ANY_RPW] < 64 ? (u32)ctx->opt[UGRT_OPT_ANY_RPW] : 64u) : 64u;
	const u32 PPW = L / (u32)num_dirs > 0u ? L / (u32)num_dirs : 1u;
	const u32 COOP = ctx->opt[UGRT_OPT_ANY_COOP] > 0 ? (u32)ctx->opt[UGRT_OPT_ANY_COOP] : 8u;
	const size_t lds = (((size_t)12 * (size_t)(set_w * set_h * num_dirs) + 15u) & ~(size_t)15u) + ((GI_LATE * 4 + 15) & ~15);
	// One prepare launch and one ray list, in the form that writes no hit defaults, with the bitmap workgroups and without
	// the split walks' chunk table.  That form clears one int per pixel of the band at [pixel]; the band's words here lie at
	// [4 * pixel .. 4 * pixel + 3], so it is handed the band's own words to write into (d_sum + 3 * p0 + pixel lies inside
	// them for every pixel of the band) and the whole band is cleared behind it, in stream order.
	u32 *list, *dcount;
	ugrt_prof_begin(ctx, UGRT_ST_WORKLIST);
	const int rc = ugrt_dda_prepare(ctx, g, d_oactive, nullptr, (int *)d_sum + (size_t)3 * (size_t)ctx->p0, d_span, true, nullptr,
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
	const auto kernel = shadow_light ? (rec ? k_gi_gather<true, true> : k_gi_gather<false, true>)
					 : (rec ? k_gi_gather<true, false> : k_gi_gather<false, false>);
	ugrt_prof_begin(ctx, UGRT_ST_TRACE_DDA);
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, ctx->stream, g, d_value_list, d_span, d_offset,
			   (const u32 *)ctx->ubitmap.p, d_vertlist, d_trilist, rec, d_orays, (const u32 *)list, (const u32 *)dcount, a,
			   ctx->cam, d_sum, PPW, COOP, ctx->d_small + UGRT_DSMALL_TICKET);
	ugrt_prof_end(ctx, UGRT_ST_TRACE_DDA);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}
