// ugrt_bounce.hip -- reflections of any depth through the uniform grid (not in the reference; DESIGN.md A13 and
// section 6).  Level 1 is ugrt_reflect_rays + ugrt_trace_dda as they are; a level j >= 2 is ugrt_reflect_rays_next from
// level j-1's hits + ugrt_trace_dda; ugrt_shade_reflect_depth blends the levels front to back.  The levels of a frame
// lie one behind the other: level j's arrays at (j-1) * W*H pixels (rays: (j-1) * W*H * 6 floats), indexed by
// absolute pixel like every per-pixel array of the frame.
#include "ugrt_dev.h"

#define PX_THREADS 256

// ---------------------------------------------------------------------------
// The secondary-ray generators.  A pixel reads a hit, stages its triangle, forms the six floats of the ray that leaves
// the hit and writes them with the ray's active word; a pixel without such a ray writes the empty ray and 0.  The four
// kernels that send a level's ray on are one body, d_secondary_ray:
//   FROM -- where the hit comes from.  HIT_PRIMARY: the primary arrays (the ids are triangle ids: no shading call has run
//   yet), the ray that made it is {cam_pos, dir_list[p*3..]}.  HIT_LEVEL: a level's hit_t / hit_id where active[p], the
//   ray is rays[p*6..]; most pixels of a deep level are inactive: their lane reads the one active word.
//   RULE -- what leaves the hit.  RAY_MIRROR: a material with reflect > 0 sends d_reflect_ray's ray (DESIGN.md A13,
//   section 6).  RAY_GLASS: a material with transmit > 0 or reflect > 0 sends the ray d_continue_ray chooses (DESIGN.md
//   section 6.6); with transmit all zero these are RAY_MIRROR's bytes.
// src is cam_pos or rays; arguments a combination does not read are null.
// k_occlusion_rays and k_ao_rays, which ask no material, have the same skeleton written out: as calls of this body the
// compiler gave them two more vector registers (profiles/secondary_refactor.txt).
// ---------------------------------------------------------------------------
enum HitFrom { HIT_PRIMARY, HIT_LEVEL };
enum RayRule { RAY_MIRROR, RAY_GLASS };

template <HitFrom FROM, RayRule RULE>
__device__ __forceinline__ void d_secondary_ray(const float *__restrict__ src, const float *__restrict__ dir_list,
						const int *__restrict__ active, const float *__restrict__ t_list,
						const int *__restrict__ id_list, const int *__restrict__ mat_idx,
						const float *__restrict__ reflect, const float *__restrict__ transmit,
						const float *__restrict__ ior, int mat_count, const float *__restrict__ verts,
						const int *__restrict__ tris, float eps, float *__restrict__ rays_out,
						int *__restrict__ active_out, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int p = p0 + i;
	float out[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	int act = 0;
	bool live = true;
	if constexpr (FROM == HIT_LEVEL)
		live = active[p] != 0;
	if (live) {
		int id = id_list[p];
		float t = t_list[p];
		if (t > 0 && id >= 0) {
			int m = mat_idx[id];
			bool leaves = m >= 0 && m < mat_count;
			if constexpr (RULE == RAY_GLASS)
				leaves = leaves && (transmit[m] > 0 || reflect[m] > 0);
			else
				leaves = leaves && reflect[m] > 0;
			if (leaves) {
				float tri[9], own[3], d[3];
				const float *o = src; // HIT_PRIMARY: the camera
				d_stage_triangle(verts, tris, (u32)id, 0.0f, 0.0f, 0.0f, tri);
				if constexpr (FROM == HIT_LEVEL) {
#pragma unroll
					for (int k = 0; k < 3; k++) {
						own[k] = src[p * 6 + k];
						d[k] = src[p * 6 + 3 + k];
					}
					o = own;
				} else {
#pragma unroll
					for (int k = 0; k < 3; k++)
						d[k] = dir_list[p * 3 + k];
				}
				if constexpr (RULE == RAY_GLASS) {
					act = d_continue_ray(o, d, t, tri, eps, transmit[m], reflect[m], ior[m], out) ? 1 : 0;
				} else {
					d_reflect_ray(o, d, t, tri, eps, out);
					act = 1;
				}
			}
		}
	}
#pragma unroll
	for (int k = 0; k < 6; k++)
		rays_out[p * 6 + k] = out[k];
	active_out[p] = act;
}

// level 1 from the primary hits
__global__ __launch_bounds__(PX_THREADS) void k_reflect_rays(const float *__restrict__ cam_pos,
							      const float *__restrict__ t_list,
							      const float *__restrict__ dir_list,
							      const int *__restrict__ id_list, const int *__restrict__ mat_idx,
							      const float *__restrict__ reflect, int mat_count,
							      const float *__restrict__ verts, const int *__restrict__ tris,
							      float eps, float *__restrict__ rays, int *__restrict__ active,
							      int p0, int n)
{
	d_secondary_ray<HIT_PRIMARY, RAY_MIRROR>(cam_pos, dir_list, nullptr, t_list, id_list, mat_idx, reflect, nullptr, nullptr,
						 mat_count, verts, tris, eps, rays, active, p0, n);
}

// level j -> j+1, from the ray's own origin
__global__ __launch_bounds__(PX_THREADS) void k_reflect_rays_next(const float *__restrict__ rays,
								   const int *__restrict__ active,
								   const float *__restrict__ hit_t,
								   const int *__restrict__ hit_id,
								   const int *__restrict__ mat_idx,
								   const float *__restrict__ reflect, int mat_count,
								   const float *__restrict__ verts, const int *__restrict__ tris,
								   float eps, float *__restrict__ rays_next,
								   int *__restrict__ active_next, int p0, int n)
{
	d_secondary_ray<HIT_LEVEL, RAY_MIRROR>(rays, nullptr, active, hit_t, hit_id, mat_idx, reflect, nullptr, nullptr, mat_count,
					       verts, tris, eps, rays_next, active_next, p0, n);
}

__global__ __launch_bounds__(PX_THREADS) void k_refract_rays(const float *__restrict__ cam_pos,
							      const float *__restrict__ t_list,
							      const float *__restrict__ dir_list,
							      const int *__restrict__ id_list, const int *__restrict__ mat_idx,
							      const float *__restrict__ reflect,
							      const float *__restrict__ transmit, const float *__restrict__ ior,
							      int mat_count, const float *__restrict__ verts,
							      const int *__restrict__ tris, float eps, float *__restrict__ rays,
							      int *__restrict__ active, int p0, int n)
{
	d_secondary_ray<HIT_PRIMARY, RAY_GLASS>(cam_pos, dir_list, nullptr, t_list, id_list, mat_idx, reflect, transmit, ior,
						mat_count, verts, tris, eps, rays, active, p0, n);
}

__global__ __launch_bounds__(PX_THREADS) void k_refract_rays_next(const float *__restrict__ rays,
								   const int *__restrict__ active,
								   const float *__restrict__ hit_t,
								   const int *__restrict__ hit_id,
								   const int *__restrict__ mat_idx,
								   const float *__restrict__ reflect,
								   const float *__restrict__ transmit,
								   const float *__restrict__ ior, int mat_count,
								   const float *__restrict__ verts, const int *__restrict__ tris,
								   float eps, float *__restrict__ rays_next,
								   int *__restrict__ active_next, int p0, int n)
{
	d_secondary_ray<HIT_LEVEL, RAY_GLASS>(rays, nullptr, active, hit_t, hit_id, mat_idx, reflect, transmit, ior, mat_count,
					      verts, tris, eps, rays_next, active_next, p0, n);
}

// Occlusion rays from one level's hits towards the light: the origin is the one the next
// reflected ray would start from (d_reflect_ray), the direction L - o' is not normalised, so the light lies at t = 1.
// The hit's material plays no part: a diffuse hit seen in a mirror is shadowed too.
__global__ __launch_bounds__(PX_THREADS) void k_occlusion_rays(const float *__restrict__ rays,
								const int *__restrict__ active,
								const float *__restrict__ hit_t,
								const int *__restrict__ hit_id,
								const float *__restrict__ verts, const int *__restrict__ tris,
								float lx, float ly, float lz, float eps,
								float *__restrict__ orays, int *__restrict__ oactive, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int p = p0 + i;
	float out[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	int act = 0;
	if (active[p]) {
		int id = hit_id[p];
		float t = hit_t[p];
		if (t > 0 && id >= 0) {
			const float L[3] = { lx, ly, lz };
			float tri[9], o[3], d[3];
			d_stage_triangle(verts, tris, (u32)id, 0.0f, 0.0f, 0.0f, tri);
#pragma unroll
			for (int k = 0; k < 3; k++) {
				o[k] = rays[p * 6 + k];
				d[k] = rays[p * 6 + 3 + k];
			}
			d_reflect_ray(o, d, t, tri, eps, out);
#pragma unroll
			for (int k = 0; k < 3; k++)
				out[3 + k] = L[k] - out[k];
			act = 1;
		}
	}
#pragma unroll
	for (int k = 0; k < 6; k++)
		orays[p * 6 + k] = out[k];
	oactive[p] = act;
}

// Ambient occlusion: per primary hit, whatever its material, the origin d_reflect_ray gives the
// reflected ray and the flipped unit normal -- {o', n} of D_HIT_FRAME from the camera.  The hemisphere directions are
// formed from these six floats in the walk (k_trace_dda_any<., AnyHemi>) and never written.  The primary arrays are read
// as k_reflect_rays reads them: the ids are triangle ids (no shading call has run yet).
__global__ __launch_bounds__(PX_THREADS) void k_ao_rays(const float *__restrict__ cam_pos,
							 const float *__restrict__ t_list,
							 const float *__restrict__ dir_list,
							 const int *__restrict__ id_list, const float *__restrict__ verts,
							 const int *__restrict__ tris, float eps, float *__restrict__ orays,
							 int *__restrict__ oactive, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int p = p0 + i;
	int id = id_list[p];
	float t = t_list[p];
	float out[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	int act = 0;
	if (t > 0 && id >= 0) {
		float tri[9], d[3], P[3], nn[3], dn;
		d_stage_triangle(verts, tris, (u32)id, 0.0f, 0.0f, 0.0f, tri);
#pragma unroll
		for (int k = 0; k < 3; k++)
			d[k] = dir_list[p * 3 + k];
		D_HIT_FRAME(cam_pos, d, t, tri, P, nn, dn);
#pragma unroll
		for (int k = 0; k < 3; k++) {
			out[k] = P[k] + eps * nn[k];
			out[3 + k] = nn[k];
		}
		act = 1;
	}
#pragma unroll
	for (int k = 0; k < 6; k++)
		orays[p * 6 + k] = out[k];
	oactive[p] = act;
}

// the exports' launch: `args` and the band, inside the reflect_gen bracket
template <class... P, class... A> static int launch_generator(ugrt_ctx *ctx, void (*kernel)(P...), A... args)
{
	UGRT_HIP(hipSetDevice(ctx->device));
	ugrt_prof_begin(ctx, UGRT_ST_REFLECT_GEN);
	hipLaunchKernelGGL(kernel, dim3((ctx->npix + PX_THREADS - 1) / PX_THREADS), dim3(PX_THREADS), 0, ctx->stream, args...,
			   ctx->p0, ctx->npix);
	ugrt_prof_end(ctx, UGRT_ST_REFLECT_GEN);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}

extern "C" int ugrt_reflect_rays(ugrt_ctx *ctx, const float *d_cam_position, const float *d_t_value,
				 const float *d_ray_dir, const int *d_intersect_id, const int *d_mat_idx,
				 const float *d_reflect, int num_materials, const float *d_vertlist, const int *d_trilist,
				 float eps, float *d_rays, int *d_active)
{
	if (!ctx || !d_cam_position || !d_t_value || !d_ray_dir || !d_intersect_id || !d_mat_idx || !d_reflect ||
	    !d_vertlist || !d_trilist || !d_rays || !d_active)
		return ugrt_fail(UGRT_EINVAL, "reflect_rays: null argument");
	if (int rc = launch_generator(ctx, k_reflect_rays, d_cam_position, d_t_value, d_ray_dir, d_intersect_id, d_mat_idx,
				      d_reflect, num_materials, d_vertlist, d_trilist, eps, d_rays, d_active))
		return rc;
	ctx->dda_deeper_level = false; // level 1: its ugrt_trace_dda uses the split-walk history (ugrt_dda.hip)
	return UGRT_OK;
}

extern "C" int ugrt_reflect_rays_next(ugrt_ctx *ctx, const float *d_rays, const int *d_active, const float *d_hit_t,
				      const int *d_hit_id, const int *d_mat_idx, const float *d_reflect, int num_materials,
				      const float *d_vertlist, const int *d_trilist, float eps, float *d_rays_next,
				      int *d_active_next)
{
	if (!ctx || !d_rays || !d_active || !d_hit_t || !d_hit_id || !d_mat_idx || !d_reflect || !d_vertlist ||
	    !d_trilist || !d_rays_next || !d_active_next)
		return ugrt_fail(UGRT_EINVAL, "reflect_rays_next: null argument");
	if (int rc = launch_generator(ctx, k_reflect_rays_next, d_rays, d_active, d_hit_t, d_hit_id, d_mat_idx, d_reflect,
				      num_materials, d_vertlist, d_trilist, eps, d_rays_next, d_active_next))
		return rc;
	ctx->dda_deeper_level = true; // the next ugrt_trace_dda walks without the split-walk history (ugrt_dda.hip)
	return UGRT_OK;
}

extern "C" int ugrt_refract_rays(ugrt_ctx *ctx, const float *d_cam_position, const float *d_t_value, const float *d_ray_dir,
				 const int *d_intersect_id, const int *d_mat_idx, const float *d_reflect,
				 const float *d_transmit, const float *d_ior, int num_materials, const float *d_vertlist,
				 const int *d_trilist, float eps, float *d_rays, int *d_active)
{
	if (!ctx || !d_cam_position || !d_t_value || !d_ray_dir || !d_intersect_id || !d_mat_idx || !d_reflect || !d_transmit ||
	    !d_ior || !d_vertlist || !d_trilist || !d_rays || !d_active)
		return ugrt_fail(UGRT_EINVAL, "refract_rays: null argument");
	if (int rc = launch_generator(ctx, k_refract_rays, d_cam_position, d_t_value, d_ray_dir, d_intersect_id, d_mat_idx,
				      d_reflect, d_transmit, d_ior, num_materials, d_vertlist, d_trilist, eps, d_rays, d_active))
		return rc;
	ctx->dda_deeper_level = false; // level 1, as ugrt_reflect_rays says it
	return UGRT_OK;
}

extern "C" int ugrt_refract_rays_next(ugrt_ctx *ctx, const float *d_rays, const int *d_active, const float *d_hit_t,
				      const int *d_hit_id, const int *d_mat_idx, const float *d_reflect,
				      const float *d_transmit, const float *d_ior, int num_materials, const float *d_vertlist,
				      const int *d_trilist, float eps, float *d_rays_next, int *d_active_next)
{
	if (!ctx || !d_rays || !d_active || !d_hit_t || !d_hit_id || !d_mat_idx || !d_reflect || !d_transmit || !d_ior ||
	    !d_vertlist || !d_trilist || !d_rays_next || !d_active_next)
		return ugrt_fail(UGRT_EINVAL, "refract_rays_next: null argument");
	if (int rc = launch_generator(ctx, k_refract_rays_next, d_rays, d_active, d_hit_t, d_hit_id, d_mat_idx, d_reflect,
				      d_transmit, d_ior, num_materials, d_vertlist, d_trilist, eps, d_rays_next, d_active_next))
		return rc;
	ctx->dda_deeper_level = true; // a level >= 2, as ugrt_reflect_rays_next says it
	return UGRT_OK;
}

extern "C" int ugrt_occlusion_rays(ugrt_ctx *ctx, const float *d_rays, const int *d_active, const float *d_hit_t,
				   const int *d_hit_id, const float *d_vertlist, const int *d_trilist,
				   const float light_pos[3], float eps, float *d_orays, int *d_oactive)
{
	if (!ctx || !d_rays || !d_active || !d_hit_t || !d_hit_id || !d_vertlist || !d_trilist || !light_pos || !d_orays ||
	    !d_oactive)
		return ugrt_fail(UGRT_EINVAL, "occlusion_rays: null argument");
	return launch_generator(ctx, k_occlusion_rays, d_rays, d_active, d_hit_t, d_hit_id, d_vertlist, d_trilist, light_pos[0],
				light_pos[1], light_pos[2], eps, d_orays, d_oactive);
}

extern "C" int ugrt_ao_rays(ugrt_ctx *ctx, const float *d_cam_position, const float *d_t_value, const float *d_ray_dir,
			    const int *d_intersect_id, const float *d_vertlist, const int *d_trilist, float eps,
			    float *d_orays, int *d_oactive)
{
	if (!ctx || !d_cam_position || !d_t_value || !d_ray_dir || !d_intersect_id || !d_vertlist || !d_trilist || !d_orays ||
	    !d_oactive)
		return ugrt_fail(UGRT_EINVAL, "ao_rays: null argument");
	return launch_generator(ctx, k_ao_rays, d_cam_position, d_t_value, d_ray_dir, d_intersect_id, d_vertlist, d_trilist, eps,
				d_orays, d_oactive);
}

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

// the clamped Lambert colour of level j's hit (as k_shade_reflect shades the first bounce's hit); 0 on a miss or a
// material out of range.  *kr: the hit material's reflect (read only where the level goes on, i.e. it is in range).
__device__ __forceinline__ void d_level_color(const CamBlock &cam, const DepthIn &in, const int *__restrict__ mat_idx,
					      const float *__restrict__ mat_list, int mat_count, size_t q, float *rc,
					      float *kr)
{
	rc[0] = rc[1] = rc[2] = 0.0f;
	int hid = in.hit_id[q];
	if (hid < 0)
		return;
	int hm = mat_idx[hid];
	if (hm < 0 || hm >= mat_count)
		return;
	float t9[9], nn[3], hp[3], hmat[6];
	float ht = in.hit_t[q];
	*kr = in.reflect[hm];
	d_stage_triangle(in.verts, in.tris, (u32)hid, 0.0f, 0.0f, 0.0f, t9);
	float *e1 = &t9[3], *e2 = &t9[6];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		hp[k] = in.rays[q * 6 + k] + ht * in.rays[q * 6 + 3 + k];
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

// acc = 0, w = 1; level j that goes on (active_{j+1}): acc += (w*(1-k_j))*L_j, w *= k_j; the first level that does not
// (level `depth` at the latest): acc += w*L_j.  At depth 1 this is k_shade_reflect operation for operation.  A pixel
// reads the levels it reaches and no others.  OCC: a level j >= 1 whose hit is occluded (in.occluded) is darkened to
// L_j / 3, the float counterpart of add_shadows' /= 3, before it is weighted.
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
	int tri = dd_intersect_id[pixelID];
	int idx = tri >= 0 ? mat_idx[tri] : tri;
	dd_intersect_id[pixelID] = idx;
	if (idx >= 0 && idx < mat_count) {
		float color[3] = { 0.0f, 0.0f, 0.0f };
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
	if (!ctx || !d_img || !d_normal || !d_t_value || !d_ray_dir || !d_intersect_id || !d_cam_position || !d_mat_idx ||
	    !d_mat_list || !d_reflect || !d_vertlist || !d_trilist || !d_rays || !d_active || !d_hit_t || !d_hit_id)
		return ugrt_fail(UGRT_EINVAL, "%s: null argument", who);
	if (depth < 1 || depth > UGRT_MAX_REFLECT_DEPTH)
		return ugrt_fail(UGRT_EINVAL, "%s: depth %d outside 1..%d", who, depth, UGRT_MAX_REFLECT_DEPTH);
	UGRT_HIP(hipSetDevice(ctx->device));
	DepthIn in = { d_reflect, d_vertlist, d_trilist, d_rays, d_active, d_hit_t, d_hit_id,
		       (size_t)ctx->cfg.width * (size_t)ctx->cfg.height, depth, d_occluded };
	ugrt_prof_begin(ctx, UGRT_ST_SHADE);
	if (d_occluded)
		hipLaunchKernelGGL(k_shade_reflect_depth<true>, dim3((ctx->npix + PX_THREADS - 1) / PX_THREADS), dim3(PX_THREADS), 0,
				   ctx->stream, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position,
				   d_mat_idx, d_mat_list, num_materials, in, ctx->p0, ctx->npix);
	else
		hipLaunchKernelGGL(k_shade_reflect_depth<false>, dim3((ctx->npix + PX_THREADS - 1) / PX_THREADS), dim3(PX_THREADS), 0,
				   ctx->stream, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position,
				   d_mat_idx, d_mat_list, num_materials, in, ctx->p0, ctx->npix);
	ugrt_prof_end(ctx, UGRT_ST_SHADE);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
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

// ---------------------------------------------------------------------------
// reflections under several lights: the depth composition of k_shade_reflect_depth<OCC> and
// k_add_shadows once per light and the mean of the bytes, in one pass.  The level chain (active_{j+1}, k_j, w) does not
// know the light: it is walked once, every level's hit is fetched once and brought to view space once (d_lambert_view),
// and shaded per light from registers (d_lambert_from) into the light's own accumulator.
// ---------------------------------------------------------------------------
struct ReflectLightsIn {
	float pos[3 * UGRT_MAX_LIGHTS]; // by value: uniform over the launch, read from the kernarg segment
	int count;
	const int *is_shadowed; // [count][level], or null
	const int *occluded;    // [depth][count][level], or null
};

__global__ __launch_bounds__(PX_THREADS) void k_shade_reflect_lights(CamBlock cam, unsigned char *__restrict__ d_img,
								      const float *__restrict__ dd_normal,
								      const float *__restrict__ dd_t_value,
								      const float *__restrict__ dd_dir,
								      int *__restrict__ dd_intersect_id,
								      const float *__restrict__ d_cam_pos,
								      const int *__restrict__ mat_idx,
								      const float *__restrict__ mat_list, int mat_count,
								      DepthIn in, ReflectLightsIn lights, int p0, int n)
{
	int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	int pixelID = p0 + i;
	u32 sum[3] = { 0u, 0u, 0u };
	int tri = dd_intersect_id[pixelID];
	int idx = tri >= 0 ? mat_idx[tri] : tri;
	dd_intersect_id[pixelID] = idx;
	if (idx >= 0 && idx < mat_count) {
		// the hit of the level at hand: lit = it has a colour at all; view-space point and normal; Kd
		float pv[3] = { 0.0f, 0.0f, 0.0f }, nv[3] = { 0.0f, 0.0f, 0.0f }, kd[3];
		float t_value = dd_t_value[pixelID];
		bool lit = t_value > 0;
#pragma unroll
		for (int k = 0; k < 3; k++)
			kd[k] = mat_list[idx * 6 + 3 + k];
		if (lit) {
			float point[3], nrm[3];
#pragma unroll
			for (int k = 0; k < 3; k++) {
				point[k] = d_cam_pos[k] + t_value * dd_dir[pixelID * 3 + k];
				nrm[k] = dd_normal[pixelID * 3 + k];
			}
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
						const bool dark = j >= 1 && lights.occluded &&
								  lights.occluded[((size_t)(j - 1) * (size_t)lights.count + (size_t)l) * in.level + (size_t)pixelID] == 1;
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
			// level j + 1's hit (d_level_color's inputs): a miss or a material out of range has no colour and leaves kr
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
				const bool dark = lights.is_shadowed && lights.is_shadowed[(size_t)l * in.level + (size_t)pixelID] == 1;
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
	if (!ctx || !d_img || !d_normal || !d_t_value || !d_ray_dir || !d_intersect_id || !d_cam_position || !d_mat_idx ||
	    !d_mat_list || !d_reflect || !d_vertlist || !d_trilist || !d_rays || !d_active || !d_hit_t || !d_hit_id || !light_pos)
		return ugrt_fail(UGRT_EINVAL, "shade_reflect_lights: null argument");
	if (depth < 1 || depth > UGRT_MAX_REFLECT_DEPTH)
		return ugrt_fail(UGRT_EINVAL, "shade_reflect_lights: depth %d outside 1..%d", depth, UGRT_MAX_REFLECT_DEPTH);
	if (num_lights < 1 || num_lights > UGRT_MAX_LIGHTS)
		return ugrt_fail(UGRT_EINVAL, "shade_reflect_lights: num_lights %d is not in 1..%d", num_lights, UGRT_MAX_LIGHTS);
	UGRT_HIP(hipSetDevice(ctx->device));
	DepthIn in = { d_reflect, d_vertlist, d_trilist, d_rays, d_active, d_hit_t, d_hit_id,
		       (size_t)ctx->cfg.width * (size_t)ctx->cfg.height, depth, nullptr };
	ReflectLightsIn lights = {};
	for (int k = 0; k < 3 * num_lights; k++)
		lights.pos[k] = light_pos[k];
	lights.count = num_lights;
	lights.is_shadowed = d_is_shadowed;
	lights.occluded = d_occluded;
	ugrt_prof_begin(ctx, UGRT_ST_SHADE);
	hipLaunchKernelGGL(k_shade_reflect_lights, dim3((ctx->npix + PX_THREADS - 1) / PX_THREADS), dim3(PX_THREADS), 0,
			   ctx->stream, ctx->cam, d_img, d_normal, d_t_value, d_ray_dir, d_intersect_id, d_cam_position,
			   d_mat_idx, d_mat_list, num_materials, in, lights, ctx->p0, ctx->npix);
	ugrt_prof_end(ctx, UGRT_ST_SHADE);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}
