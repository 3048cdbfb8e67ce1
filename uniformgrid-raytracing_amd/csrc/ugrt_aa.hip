// ugrt_aa.hip -- adaptive anti-aliasing: sub-pixel eye rays on edge pixels (not in the reference).
//
// Spec: ugrt_aa_edges flags the pixels whose 3x3 neighbourhood holds a silhouette, a material border, a crease, a depth
// step or a shadow edge.  ugrt_aa_gather sends S eye rays through each flagged pixel -- d_ray_dir's arithmetic at
// (col + sx, row + sy), the offsets of set k(p) of a table in LDS --, finds each ray's closest hit as ugrt_trace_dda finds
// it, gates it as the primary epilogue gates a hit (d_finish_pixel), shades it as k_shade<false> shades a primary hit,
// darkens the bytes to a third where the shadow light is hidden (k_add_shadows' integer division), and sums the bytes of
// the pixel's S rays.  ugrt_aa_resolve (ugrt_shade.hip) writes the rounded mean over the pixel.
//   * the index space is ugrt_gi_gather's (pixel group, sample): the S rays of a pixel in neighbouring lanes, one
//     prepare launch, one ray list, the groups behind the first gridDim.x drawn from the ticket;
//   * the two walks are ugrt_walks.h's, shared with ugrt_gi.hip: d_closest_walk without a radius, d_any_walk with the
//     light at t = 1;
//   * no ray array is read or written: the lane forms its ray from (p, s), and ray, hit, occlusion ray and colour stay
//     in its registers;
//   * the three byte sums are added across the pixel's S lanes and stored with the count word by the pixel's first lane.
#include "ugrt_walks.h"

// words staged in LDS behind the offset table and the eye's 5x5x4 node table, which only the code in front of, between
// and behind the walks reads: the eye, rows 2 and 3 of its MVP, the current camera block's rotation and light, the shadow
// light, eps; then (AA_LATE_F on) the material arrays, their count, `sum` and the ticket as 32-bit halves, W, H, strict
#define AA_LATE_F 30
#define AA_LATE 44
#define AA_TEX 100

// ugrt_dda.hip
int ugrt_dda_prepare(ugrt_ctx *ctx, const DGrid &g, const int *d_active, float *d_hit_t, int *d_hit_id, const u32 *d_span,
		     bool with_bitmap, u32 *chunk, u32 **list_out, u32 **dcount_out);

struct AaArg {
	const float *offsets; // device memory [set_w * set_h][S][2] sub-pixel offsets
	int count;            // S
	u32 set_w, set_h;     // 1..4 each
	float tex[AA_TEX];    // the eye's node table (ugrt_camera_direction_table)
	float eye[3];
	float mvp[8];         // the eye's MVP: what rows 2 and 3 of D_MULMV_ROW(m, 48, ...) read
	float view[12];       // the context's current block, cc[16..27], and its light: d_lambert's
	float clight[3];
	int W, H, strict_tex;
	const int *mat_idx;
	const float *mat_list;
	int mat_count;
	float light[3];       // the shadow light (SHADOW only)
	float eps;
};

// (dynamic LDS, its base 16-byte aligned: the offset table)
extern __shared__ __attribute__((aligned(16))) float s_aa[];

// `sum` of the band was cleared in stream order before the launch: only the words of flagged pixels are written
template <bool REC, bool SHADOW>
__global__ __launch_bounds__(64) void k_aa_gather(DGrid g, const u32 *__restrict__ value_list, const u32 *__restrict__ span,
						  const u32 *__restrict__ offset, const u32 *__restrict__ bitmap,
						  const float *__restrict__ verts, const int *__restrict__ tris,
						  const float4 *__restrict__ rec, const u32 *__restrict__ list,
						  const u32 *__restrict__ count_p, const AaArg a, u32 *__restrict__ sum, u32 PPW,
						  u32 COOP, u32 *__restrict__ ticket)
{
	const int lane = threadIdx.x;
	const u32 count = *count_p;
	const u32 S = (u32)a.count;
	const u32 table = (2u * S * a.set_w * a.set_h + 3u) & ~3u; // floats of the offset table, padded
	{
		const u32 total = 2u * S * a.set_w * a.set_h;
		u32 done = 0u;
		if (((size_t)a.offsets & 15u) == 0u) {
			for (u32 i = 4u * (u32)lane; i + 4u <= total; i += 256u)
				*(float4 *)(s_aa + i) = *(const float4 *)(a.offsets + i);
			done = total & ~3u;
		}
		for (u32 i = done + (u32)lane; i < total; i += 64u)
			s_aa[i] = a.offsets[i];
		float *tex = s_aa + table;
#pragma unroll
		for (int i = 0; i < AA_TEX; i += 64)
			if (i + lane < AA_TEX)
				tex[i + lane] = a.tex[i + lane];
		float *late = tex + AA_TEX;
#pragma unroll
		for (int i = 0; i < AA_LATE_F; i++) {
			const float v = i < 3 ? a.eye[i]
					      : (i < 11 ? a.mvp[i - 3]
							: (i < 23 ? a.view[i - 11]
								  : (i < 26 ? a.clight[i - 23] : (i < 29 ? a.light[i - 26] : a.eps))));
			if (lane == 0)
				late[i] = v;
		}
		if (lane == 0) {
			u32 *w = (u32 *)late + AA_LATE_F;
			w[0] = (u32)(size_t)a.mat_idx;
			w[1] = (u32)((size_t)a.mat_idx >> 32);
			w[2] = (u32)(size_t)a.mat_list;
			w[3] = (u32)((size_t)a.mat_list >> 32);
			w[4] = (u32)a.mat_count;
			w[5] = (u32)(size_t)sum;
			w[6] = (u32)((size_t)sum >> 32);
			w[7] = (u32)(size_t)ticket;
			w[8] = (u32)((size_t)ticket >> 32);
			w[9] = (u32)a.W;
			w[10] = (u32)a.H;
			w[11] = (u32)a.strict_tex;
		}
		__syncthreads();
	}
	const float *tex = s_aa + table;
	const float *late = tex + AA_TEX;
	const u32 *late_w = (const u32 *)late + AA_LATE_F;
	// groups of PPW pixels, the first gridDim.x by workgroup id, the others drawn from the ticket
	for (u32 grp = blockIdx.x; grp * PPW < count;) {
		u32 apix, asmp;
		d_area_lane(lane, S, apix, asmp);
		const u32 slot = grp * PPW + apix;
		bool inb = apix < PPW && slot < count;
		const int p = inb ? (int)list[slot] : 0;
		inb = inb && p != -1; // (padding: k_dda_prepare)
		// ---- the lane's ray: the eye, d_ray_dir at (col + sx, row + sy) with entry asmp of set k(p) ----
		float o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 }, res_t;
		int res_id;
		if (inb) {
			const u32 width = late_w[9], set_w = a.set_w, set_h = a.set_h;
			const u32 y = (u32)p / width, x = (u32)p - y * width;
			const u32 at = 2u * (((y % set_h) * set_w + x % set_w) * S + asmp);
			CamBlock eye; // (d_ray_dir_at reads the eye, W, H and the strict flag, nothing else)
			eye.W = (int)width;
			eye.H = (int)late_w[10];
			eye.strict_tex = __builtin_amdgcn_readfirstlane((int)late_w[11]);
#pragma unroll
			for (int k = 0; k < 3; k++)
				eye.cc[k] = o[k] = late[k];
			// (the table is the caller's data: an offset outside [-0.5, 0.5] is clamped, a NaN becomes -0.5, so that the
			// node index of d_ray_dir_at stays inside the table whatever it holds)
			const float sx = fminf(fmaxf(s_aa[at], -0.5f), 0.5f), sy = fminf(fmaxf(s_aa[at + 1u], -0.5f), 0.5f);
			d_ray_dir_at(eye, tex, (float)x + sx, (float)y + sy, d);
		}
		// ---- phase A: the closest hit of {eye, d} (k_trace_dda_ray's loop) ----
		d_closest_walk<REC, false>(g, value_list, span, offset, bitmap, verts, tris, rec, o, d, 0.0f, inb, COOP, lane, res_t,
					   res_id);
		// ---- the depth gate, the hit's bytes and its occlusion ray, formed here so that phase B holds neither o nor d ----
		float o2[3] = { 0.0f, 0.0f, 0.0f }, d2[3] = { 0.0f, 0.0f, 0.0f };
		u32 rg = 0u, bb = 0u; // r | g << 16, b: a sum is at most 32 * 255 < 2^13
		bool lit_hit = false; // a hit with a colour: a miss and a material out of range stay 0, occluded or not
		if (res_id >= 0) {
			// d_finish_pixel's gate with the eye's MVP
			float P[3];
#pragma unroll
			for (int k = 0; k < 3; k++)
				P[k] = o[k] + res_t * d[k];
			float hz = late[3] * P[0] + late[4] * P[1] + late[5] * P[2] + late[6] * 1.0f;
			const float hw = late[7] * P[0] + late[8] * P[1] + late[9] * P[2] + late[10] * 1.0f;
			hz /= hw;
			const int *mat_idx = (const int *)(((size_t)late_w[1] << 32) | (size_t)late_w[0]);
			const float *mat_list = (const float *)(((size_t)late_w[3] << 32) | (size_t)late_w[2]);
			const int hm = ugrt_floor2i(hz * 1.0f) == 0 ? mat_idx[res_id] : -1;
			if (hm >= 0 && hm < (int)late_w[4]) {
				float t9[9];
				d_stage_triangle(verts, tris, (u32)res_id, 0.0f, 0.0f, 0.0f, t9);
				if constexpr (SHADOW) {
					// k_occlusion_rays' ray: d_reflect_ray's origin, the direction light - o'' not normalised
					float out[6];
					d_reflect_ray(o, d, res_t, t9, late[29], out);
#pragma unroll
					for (int k = 0; k < 3; k++) {
						o2[k] = out[k];
						d2[k] = late[26 + k] - out[k];
					}
				}
				// the normal as d_finish_pixel stores it, the shading as k_shade<false> reads it
				float *e1 = &t9[3], *e2 = &t9[6], nrm[3], material[6], color[3] = { 0.0f, 0.0f, 0.0f };
				D_NORMALIZE(e1);
				D_NORMALIZE(e2);
				D_CROSS(nrm, e1, e2);
				D_NORMALIZE(nrm);
#pragma unroll
				for (int k = 0; k < 3; k++)
					nrm[k] = nrm[k] < 0 ? nrm[k] * -1 : nrm[k];
				CamBlock view; // (d_lambert reads the rotation and the light, nothing else)
#pragma unroll
				for (int i = 0; i < 12; i++)
					view.cc[16 + i] = late[11 + i];
#pragma unroll
				for (int k = 0; k < 3; k++)
					view.light[k] = late[23 + k];
				d_material_kd(mat_list, hm, material);
				d_lambert<false>(view, P, nrm, color, material, 1.0f);
				d_clamp1(color);
				rg = (u32)d_to_u8(color[0]) | ((u32)d_to_u8(color[1]) << 16);
				bb = (u32)d_to_u8(color[2]);
				lit_hit = true;
			}
		}
		// ---- phase B: is the shadow light hidden from the hit (k_trace_dda_any's loop, the light at t = 1) ----
		if constexpr (SHADOW) {
			const bool occ = d_any_walk<REC>(g, value_list, span, offset, bitmap, verts, tris, rec, o2, d2, 1.0f, lit_hit, COOP,
							 lane);
			if (occ) { // k_add_shadows: each byte / 3
				rg = ((rg & 0xFFFFu) / 3u) | (((rg >> 16) / 3u) << 16);
				bb = bb / 3u;
			}
		}
		// ---- the bytes summed over the pixel's S neighbouring lanes (idle and padding lanes hold zeros) ----
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

extern "C" int ugrt_aa_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
			      const float *d_vertlist, const int *d_trilist, const float *eye_camcoords, const int *d_edge,
			      int num_samples, int set_w, int set_h, const float *d_offsets, const int *d_mat_idx,
			      const float *d_mat_list, int num_materials, const float *shadow_light, float eps, unsigned *d_sum)
{
	if (!ctx || !d_value_list || !d_span || !d_offset || !d_vertlist || !d_trilist || !eye_camcoords || !d_edge || !d_offsets ||
	    !d_mat_idx || !d_mat_list || !d_sum)
		return ugrt_fail(UGRT_EINVAL, "aa_gather: null argument");
	if (num_samples < 1 || num_samples > UGRT_MAX_AA_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "aa_gather: num_samples %d is not in 1..%d", num_samples, UGRT_MAX_AA_SAMPLES);
	if (set_w < 1 || set_w > UGRT_MAX_AA_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "aa_gather: set_w %d is not in 1..%d", set_w, UGRT_MAX_AA_SET_TILE);
	if (set_h < 1 || set_h > UGRT_MAX_AA_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "aa_gather: set_h %d is not in 1..%d", set_h, UGRT_MAX_AA_SET_TILE);
	if (eps != eps)
		return ugrt_fail(UGRT_EINVAL, "aa_gather: eps is not a number");
	if (num_materials < 1)
		return ugrt_fail(UGRT_EINVAL, "aa_gather: num_materials %d is less than 1", num_materials);
	if (((size_t)d_sum & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "aa_gather: d_sum is not 16-byte aligned");
	Grid &G = ctx->grid[UGRT_GRID_UNIFORM];
	if (!G.valid)
		return ugrt_fail(UGRT_EINVAL, "trace_dda: build the uniform grid first (it defines the cell geometry)");
	AaArg a = {};
	if (int rc = ugrt_camera_direction_table(eye_camcoords, a.tex))
		return rc;
	UGRT_HIP(hipSetDevice(ctx->device));
	const DGrid g = ugrt_dgrid_of(G);
	const float4 *rec = ugrt_trirec_of(ctx, d_vertlist, d_trilist);
	a.offsets = d_offsets;
	a.count = num_samples;
	a.set_w = (u32)set_w;
	a.set_h = (u32)set_h;
	for (int k = 0; k < 3; k++) {
		a.eye[k] = eye_camcoords[k];
		a.clight[k] = ctx->cam.light[k];
		a.light[k] = shadow_light ? shadow_light[k] : 0.0f;
	}
	for (int k = 0; k < 4; k++) {
		a.mvp[k] = eye_camcoords[48 + 4 * k + 2];
		a.mvp[4 + k] = eye_camcoords[48 + 4 * k + 3];
	}
	for (int k = 0; k < 12; k++)
		a.view[k] = ctx->cam.cc[16 + k];
	a.W = ctx->cfg.width;
	a.H = ctx->cfg.height;
	a.strict_tex = ctx->cam.strict_tex;
	a.mat_idx = d_mat_idx;
	a.mat_list = d_mat_list;
	a.mat_count = num_materials;
	a.eps = eps;
	// launch shape (ugrt_ctx_set_option; no effect on results): ugrt_gi_gather's
	const u32 L = ctx->opt[UGRT_OPT_ANY_RPW] > 0 ? (ctx->opt[UGRT_OPT_ANY_RPW] < 64 ? (u32)ctx->opt[UGRT_OPT_ANY_RPW] : 64u) : 64u;
	const u32 PPW = L / (u32)num_samples > 0u ? L / (u32)num_samples : 1u;
	const u32 COOP = ctx->opt[UGRT_OPT_ANY_COOP] > 0 ? (u32)ctx->opt[UGRT_OPT_ANY_COOP] : 8u;
	const size_t lds = (((size_t)8 * (size_t)(set_w * set_h * num_samples) + 15u) & ~(size_t)15u) + (AA_TEX + AA_LATE) * 4;
	// The prepare launch, the ray list and the clearing of the band's words are ugrt_gi_gather's (see there for the
	// pointer the prepare kernel is handed): d_edge stands where the active flags stand.
	u32 *list, *dcount;
	ugrt_prof_begin(ctx, UGRT_ST_WORKLIST);
	const int rc = ugrt_dda_prepare(ctx, g, d_edge, nullptr, (int *)d_sum + (size_t)3 * (size_t)ctx->p0, d_span, true, nullptr,
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
	const auto kernel = shadow_light ? (rec ? k_aa_gather<true, true> : k_aa_gather<false, true>)
					 : (rec ? k_aa_gather<true, false> : k_aa_gather<false, false>);
	ugrt_prof_begin(ctx, UGRT_ST_TRACE_DDA);
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, ctx->stream, g, d_value_list, d_span, d_offset,
			   (const u32 *)ctx->ubitmap.p, d_vertlist, d_trilist, rec, (const u32 *)list, (const u32 *)dcount, a, d_sum, PPW,
			   COOP, ctx->d_small + UGRT_DSMALL_TICKET);
	ugrt_prof_end(ctx, UGRT_ST_TRACE_DDA);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}

// ---------------------------------------------------------------------------
// Which pixels are supersampled: p against each of its up to eight neighbours q inside the image (rows outside the band
// are read: the primary arrays are whole-image arrays).  A 3x3 read per pixel, through L2.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PX_THREADS) void k_aa_edges(const float *__restrict__ normal, const float *__restrict__ t_value,
							  const float *__restrict__ dir, const int *__restrict__ ids,
							  const float *__restrict__ cam_pos, const int *__restrict__ mat_idx,
							  const int *__restrict__ shadowed, float normal_cos, float plane_tol, int W,
							  int H, int *__restrict__ edge, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const int p = p0 + i;
	const int y = p / W, x = p - y * W;
	const int id_p = ids[p];
	const bool hit_p = t_value[p] > 0 && id_p >= 0;
	float Pp[3] = { 0.0f, 0.0f, 0.0f }, np[3] = { 0.0f, 0.0f, 0.0f };
	int m_p = 0;
	if (hit_p) {
		const float t = t_value[p];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			Pp[k] = cam_pos[k] + t * dir[p * 3 + k];
			np[k] = normal[p * 3 + k];
		}
		m_p = mat_idx[id_p];
	}
	const int sh_p = shadowed ? shadowed[p] : 0;
	int e = 0;
	for (int dy = -1; dy <= 1; dy++) {
		for (int dx = -1; dx <= 1; dx++) {
			const int qx = x + dx, qy = y + dy;
			if ((dx == 0 && dy == 0) || qx < 0 || qx >= W || qy < 0 || qy >= H)
				continue;
			const int q = qy * W + qx;
			const int id_q = ids[q];
			const bool hit_q = t_value[q] > 0 && id_q >= 0;
			if (hit_p != hit_q)
				e = 1;
			if (hit_p && hit_q && id_p != id_q) {
				const float t = t_value[q];
				float Pq[3], nq[3];
#pragma unroll
				for (int k = 0; k < 3; k++) {
					Pq[k] = cam_pos[k] + t * dir[q * 3 + k];
					nq[k] = normal[q * 3 + k];
				}
				const float cosine = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
				const float dist = (np[0] * (Pq[0] - Pp[0]) + np[1] * (Pq[1] - Pp[1])) + np[2] * (Pq[2] - Pp[2]);
				if (mat_idx[id_q] != m_p || cosine < normal_cos || __builtin_fabsf(dist) > plane_tol)
					e = 1;
			}
			if (shadowed && shadowed[q] != sh_p)
				e = 1;
		}
	}
	edge[p] = e;
}

extern "C" int ugrt_aa_edges(ugrt_ctx *ctx, const float *d_normal, const float *d_t_value, const float *d_ray_dir,
			     const int *d_intersect_id, const float *d_cam_position, const int *d_mat_idx,
			     const int *d_is_shadowed, float normal_cos, float plane_tol, int *d_edge)
{
	if (!ctx || !d_normal || !d_t_value || !d_ray_dir || !d_intersect_id || !d_cam_position || !d_mat_idx || !d_edge)
		return ugrt_fail(UGRT_EINVAL, "aa_edges: null argument");
	if (normal_cos != normal_cos)
		return ugrt_fail(UGRT_EINVAL, "aa_edges: normal_cos is not a number");
	if (plane_tol != plane_tol)
		return ugrt_fail(UGRT_EINVAL, "aa_edges: plane_tol is not a number");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_aa_edges, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position,
				  d_mat_idx, d_is_shadowed, normal_cos, plane_tol, ctx->cfg.width, ctx->cfg.height, d_edge);
}
