// ugrt_glossy.hip -- glossy reflections: a lobe of closest-hit rays around the mirror direction (not in the reference;
// DESIGN.md section 6.13).
//
// Spec: an active pixel p of ugrt_reflect_rays' {o, R} sends S rays from o.  Sample s takes the point (u, v) of set k(p)
// of a table of points in the unit disk, the spread a of the primary hit's material, and the direction
// D = d_hemi_dir(normalize(R), a*u, a*v, 1): the mirror direction tilted by at most atan(a).  A D that would enter the
// surface (D.n < 0, n of ugrt_ao_rays) is mirrored back over it.  From {o, D} on everything is ugrt_gi_gather's: the
// kernel is k_pixel_gather of ugrt_gather.h with ugrt_gi.hip's shading (GatherLevelShade) and the Kind below, whose own
// part is the lane's ray.  The lobe is narrow, so a pixel's neighbouring lanes walk the same cells and test the same lists.
// ugrt_glossy_apply blends the mean byte of the lobe into the image with the material's reflect as the weight.
#include "ugrt_gather.h"

// a point's coordinate: clamped to [-1, 1], a NaN counts as 0
__device__ __forceinline__ float d_gl_coord(float x)
{
	x = x == x ? x : 0.0f;
	return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
}

struct GlossyKind : GatherLevelShade {
	struct Late : GatherLate {
		const float *orays;  // {o', n} of ugrt_ao_rays: n is read
		const int *ids;      // the primary hits' triangles
		const float *spread; // per material
	};
	struct Arg : GatherArg { // table: [set_w * set_h][S][2] points of the unit disk
		Late late;
	};
	static constexpr u32 entry = 2u;
	// o of ugrt_reflect_rays' {o, R}, and R tilted by the lane's point times the spread
	static __device__ __forceinline__ void ray(const Late &late, const float *point, const float *,
						   const float *__restrict__ rays, int p, u32, u32, float *o, float *d)
	{
		float R[3], nrm[3];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			o[k] = rays[p * 6 + k];
			R[k] = rays[p * 6 + 3 + k];
			nrm[k] = late.orays[p * 6 + 3 + k];
		}
		// the spread of the primary hit's material: NaN, zeros and negative values count as 0, values above the maximum as it
		float spr = 0.0f;
		const int id = late.ids[p];
		if (id >= 0) {
			const int m = late.mat_idx[id];
			if (m >= 0 && m < late.mat_count) {
				const float sp = late.spread[m];
				if (sp > 0.0f)
					spr = sp > UGRT_MAX_GLOSSY_SPREAD ? UGRT_MAX_GLOSSY_SPREAD : sp;
			}
		}
		const float u = d_gl_coord(point[0]), v = d_gl_coord(point[1]);
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
};

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
	GlossyKind::Arg a = {};
	a.table = d_points;
	a.count = num_samples;
	a.set_w = (u32)set_w;
	a.set_h = (u32)set_h;
	a.width = (u32)ctx->cfg.width;
	a.radius = radius;
	static_cast<GatherLate &>(a.late) =gather_late_of(ctx, d_mat_idx, d_mat_list, num_materials, shadow_light, eps, d_sum);
	a.late.orays = d_orays;
	a.late.ids = d_intersect_id;
	a.late.spread = d_spread;
	return pixel_gather<GlossyKind>({ ctx, d_value_list, d_span, d_offset, d_vertlist, d_trilist, d_rays, d_active, d_sum }, a,
					shadow_light != nullptr);
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
