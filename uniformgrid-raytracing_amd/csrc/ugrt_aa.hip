// ugrt_aa.hip -- adaptive anti-aliasing: sub-pixel eye rays on edge pixels (not in the reference).
//
// Spec: ugrt_aa_edges flags the pixels whose 3x3 neighbourhood holds a silhouette, a material border, a crease, a depth
// step or a shadow edge.  ugrt_aa_gather sends S eye rays through each flagged pixel -- d_ray_dir's arithmetic at
// (col + sx, row + sy), the offsets of set k(p) of a table in LDS --, finds each ray's closest hit as ugrt_trace_dda finds
// it, gates it as the primary epilogue gates a hit (d_finish_pixel), shades it as k_shade<false> shades a primary hit,
// darkens the bytes to a third where the shadow light is hidden (k_add_shadows' integer division), and sums the bytes of
// the pixel's S rays.  ugrt_aa_resolve (ugrt_shade.hip) writes the rounded mean over the pixel.
// The kernel is k_pixel_gather of ugrt_gather.h (d_closest_walk without a radius) with the Kind below.  Its own parts:
//   * no ray array is read or written: the lane forms its ray from (p, s) and the eye's 5x5x4 node table, which lies in
//     LDS between the offset table and the staged words;
//   * the depth gate and the primary hit's shading, on bytes from the hit on.
#include "ugrt_gather.h"

#define AA_TEX 100

struct AaKind {
	struct Late : GatherLate {
		float eye[3];
		float mvp[8]; // the eye's MVP: what rows 2 and 3 of D_MULMV_ROW(m, 48, ...) read
		int W, H, strict_tex;
	};
	struct Arg : GatherArg { // table: [set_w * set_h][S][2] sub-pixel offsets
		Late late;
		float tex[AA_TEX]; // the eye's node table (ugrt_camera_direction_table)
	};
	struct Colour {
		u32 rg, bb; // r | g << 16, b
	};
	static constexpr u32 entry = 2u, extra = AA_TEX;
	static constexpr bool radius = false;
	static __device__ __forceinline__ void stage(float *tex, const Arg &a, int lane)
	{
#pragma unroll
		for (int i = 0; i < AA_TEX; i += 64)
			if (i + lane < AA_TEX)
				tex[i + lane] = a.tex[i + lane];
	}
	// the eye, d_ray_dir at (col + sx, row + sy) with the lane's offset
	static __device__ __forceinline__ void ray(const Late &late, const float *off, const float *tex, const float *, int,
						   u32 x, u32 y, float *o, float *d)
	{
		CamBlock eye; // (d_ray_dir_at reads the eye, W, H and the strict flag, nothing else)
		eye.W = late.W;
		eye.H = late.H;
		eye.strict_tex = __builtin_amdgcn_readfirstlane(late.strict_tex);
#pragma unroll
		for (int k = 0; k < 3; k++)
			eye.cc[k] = o[k] = late.eye[k];
		// (the table is the caller's data: an offset outside [-0.5, 0.5] is clamped, a NaN becomes -0.5, so that the
		// node index of d_ray_dir_at stays inside the table whatever it holds)
		const float sx = fminf(fmaxf(off[0], -0.5f), 0.5f), sy = fminf(fmaxf(off[1], -0.5f), 0.5f);
		d_ray_dir_at(eye, tex, (float)x + sx, (float)y + sy, d);
	}
	// the hit gated as the primary epilogue gates it and shaded as k_shade<false> shades a primary hit; false: a miss, a
	// gated hit or a material out of range, which stay 0, occluded or not
	template <bool SHADOW>
	static __device__ __forceinline__ bool shade(const Late &late, const float *__restrict__ verts, const int *__restrict__ tris,
						     const float *o, const float *d, float res_t, int res_id, Colour &c, float *o2,
						     float *d2)
	{
		if (res_id < 0)
			return false;
		// d_finish_pixel's gate with the eye's MVP
		float P[3];
#pragma unroll
		for (int k = 0; k < 3; k++)
			P[k] = o[k] + res_t * d[k];
		float hz = late.mvp[0] * P[0] + late.mvp[1] * P[1] + late.mvp[2] * P[2] + late.mvp[3] * 1.0f;
		const float hw = late.mvp[4] * P[0] + late.mvp[5] * P[1] + late.mvp[6] * P[2] + late.mvp[7] * 1.0f;
		hz /= hw;
		const int hm = ugrt_floor2i(hz * 1.0f) == 0 ? late.mat_idx[res_id] : -1;
		if (!(hm >= 0 && hm < late.mat_count))
			return false;
		float t9[9];
		d_stage_triangle(verts, tris, (u32)res_id, 0.0f, 0.0f, 0.0f, t9);
		if constexpr (SHADOW)
			d_gather_occlusion_ray(late, o, d, res_t, t9, o2, d2);
		// the normal as d_finish_pixel stores it, the shading as k_shade<false> reads it
		float *e1 = &t9[3], *e2 = &t9[6], nrm[3], material[6], color[3] = { 0.0f, 0.0f, 0.0f };
		D_NORMALIZE(e1);
		D_NORMALIZE(e2);
		D_CROSS(nrm, e1, e2);
		D_NORMALIZE(nrm);
#pragma unroll
		for (int k = 0; k < 3; k++)
			nrm[k] = nrm[k] < 0 ? nrm[k] * -1 : nrm[k];
		CamBlock view;
		d_gather_view(late, view);
		d_material_kd(late.mat_list, hm, material);
		d_lambert<false>(view, P, nrm, color, material, 1.0f);
		d_clamp1(color);
		c.rg = (u32)d_to_u8(color[0]) | ((u32)d_to_u8(color[1]) << 16);
		c.bb = (u32)d_to_u8(color[2]);
		return true;
	}
	// k_add_shadows: each byte / 3
	static __device__ __forceinline__ void darken(Colour &c, bool occ, bool, u32 &rg, u32 &bb)
	{
		rg = occ ? ((c.rg & 0xFFFFu) / 3u) | (((c.rg >> 16) / 3u) << 16) : c.rg;
		bb = occ ? c.bb / 3u : c.bb;
	}
};

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
	AaKind::Arg a = {};
	if (int rc = ugrt_camera_direction_table(eye_camcoords, a.tex))
		return rc;
	a.table = d_offsets;
	a.count = num_samples;
	a.set_w = (u32)set_w;
	a.set_h = (u32)set_h;
	a.width = (u32)ctx->cfg.width;
	static_cast<GatherLate &>(a.late) = gather_late_of(ctx, d_mat_idx, d_mat_list, num_materials, shadow_light, eps, d_sum);
	for (int k = 0; k < 3; k++)
		a.late.eye[k] = eye_camcoords[k];
	for (int k = 0; k < 4; k++) {
		a.late.mvp[k] = eye_camcoords[48 + 4 * k + 2];
		a.late.mvp[4 + k] = eye_camcoords[48 + 4 * k + 3];
	}
	a.late.W = ctx->cfg.width;
	a.late.H = ctx->cfg.height;
	a.late.strict_tex = ctx->cam.strict_tex;
	// (no ray array: d_edge stands where the active flags stand)
	return pixel_gather<AaKind>({ ctx, d_value_list, d_span, d_offset, d_vertlist, d_trilist, nullptr, d_edge, d_sum }, a,
				    shadow_light != nullptr);
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
