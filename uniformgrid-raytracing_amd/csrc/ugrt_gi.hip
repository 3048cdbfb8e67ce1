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
//
// The kernel is k_pixel_gather of ugrt_gather.h -- the index space, the two walks (d_closest_walk<., true>: best_t starts
// at min(3.0e38f, radius) and the walk also ends behind a cell whose exit parameter is not below radius), the staged
// words, the sum across the pixel's S lanes -- with the Kind below: what is this file's own is the lane's ray.
#include "ugrt_gather.h"

struct GiKind : GatherLevelShade {
	typedef GatherLate Late;
	struct Arg : GatherArg { // table: [set_w * set_h][S][3] local directions
		Late late;
	};
	static constexpr u32 entry = 3u;
	// {o', n} of ugrt_ao_rays and the lane's local direction over n
	static __device__ __forceinline__ void ray(const Late &, const float *dir, const float *, const float *__restrict__ rays,
						   int p, u32, u32, float *o, float *d)
	{
		float nrm[3];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			o[k] = rays[p * 6 + k];
			nrm[k] = rays[p * 6 + 3 + k];
		}
		d_hemi_dir(nrm, dir[0], dir[1], dir[2], d);
	}
};

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
	GiKind::Arg a = {};
	a.table = d_dirs;
	a.count = num_dirs;
	a.set_w = (u32)set_w;
	a.set_h = (u32)set_h;
	a.width = (u32)ctx->cfg.width;
	a.radius = radius;
	a.late = gather_late_of(ctx, d_mat_idx, d_mat_list, num_materials, shadow_light, eps, d_sum);
	return pixel_gather<GiKind>({ ctx, d_value_list, d_span, d_offset, d_vertlist, d_trilist, d_orays, d_oactive, d_sum }, a,
				    shadow_light != nullptr);
}
