// ugrt_eye_kind.h -- the Kind of k_pixel_gather (ugrt_gather.h) whose rays are eye rays: formed in the kernel from the
// eye's node table, gated as the primary epilogue gates a hit and shaded as a primary hit (DESIGN.md sections 6.11, 6.17).
// ugrt_aa.hip instantiates it as it stands; ugrt_dof.hip derives the lens's Kind from it and replaces ray().
#ifndef UGRT_EYE_KIND_H
#define UGRT_EYE_KIND_H

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
	template <class A> static __device__ __forceinline__ void stage(float *tex, const A &a, int lane)
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

// what ugrt_aa_gather and ugrt_dof_gather check alike; `who` starts the message
static inline int eye_gather_check(const char *who, const void *ctx, const void *d_value_list, const void *d_span,
				   const void *d_offset, const void *d_vertlist, const void *d_trilist, const void *eye_camcoords,
				   const void *d_flags, const void *d_table, const void *d_mat_idx, const void *d_mat_list,
				   const void *d_sum, int num_samples, int set_w, int set_h, float eps, int num_materials)
{
	if (!ctx || !d_value_list || !d_span || !d_offset || !d_vertlist || !d_trilist || !eye_camcoords || !d_flags || !d_table ||
	    !d_mat_idx || !d_mat_list || !d_sum)
		return ugrt_fail(UGRT_EINVAL, "%s: null argument", who);
	if (num_samples < 1 || num_samples > UGRT_MAX_AA_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "%s: num_samples %d is not in 1..%d", who, num_samples, UGRT_MAX_AA_SAMPLES);
	if (set_w < 1 || set_w > UGRT_MAX_AA_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "%s: set_w %d is not in 1..%d", who, set_w, UGRT_MAX_AA_SET_TILE);
	if (set_h < 1 || set_h > UGRT_MAX_AA_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "%s: set_h %d is not in 1..%d", who, set_h, UGRT_MAX_AA_SET_TILE);
	if (eps != eps)
		return ugrt_fail(UGRT_EINVAL, "%s: eps is not a number", who);
	if (num_materials < 1)
		return ugrt_fail(UGRT_EINVAL, "%s: num_materials %d is less than 1", who, num_materials);
	if (((size_t)d_sum & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "%s: d_sum is not 16-byte aligned", who);
	return UGRT_OK;
}

// the eye's part of an Arg: the table, the tile, the Late's words and the node table
template <class Arg>
static inline int eye_gather_arg(Arg &a, const ugrt_ctx *ctx, const float *eye_camcoords, int num_samples, int set_w, int set_h,
				 const float *d_table, const int *d_mat_idx, const float *d_mat_list, int num_materials,
				 const float *shadow_light, float eps, unsigned *d_sum)
{
	if (int rc = ugrt_camera_direction_table(eye_camcoords, a.tex))
		return rc;
	a.table = d_table;
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
	return UGRT_OK;
}

#endif
