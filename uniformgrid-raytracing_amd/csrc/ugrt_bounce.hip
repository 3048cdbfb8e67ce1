// ugrt_bounce.hip -- the secondary-ray generators of the reflections of any depth through the uniform grid (not in the
// reference).  Level 1 is ugrt_reflect_rays + ugrt_trace_dda as they are; a level j >= 2 is
// ugrt_reflect_rays_next from level j-1's hits + ugrt_trace_dda; ugrt_shade_reflect_depth (with every other shader in
// ugrt_shade.hip) blends the levels front to back.  The levels of a frame lie one behind the other: level j's arrays at
// (j-1) * W*H pixels (rays: (j-1) * W*H * 6 floats), indexed by absolute pixel like every per-pixel array of the frame.
#include "ugrt_dev.h"

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

extern "C" int ugrt_reflect_rays(ugrt_ctx *ctx, const float *d_cam_position, const float *d_t_value,
				 const float *d_ray_dir, const int *d_intersect_id, const int *d_mat_idx,
				 const float *d_reflect, int num_materials, const float *d_vertlist, const int *d_trilist,
				 float eps, float *d_rays, int *d_active)
{
	if (!ctx || !d_cam_position || !d_t_value || !d_ray_dir || !d_intersect_id || !d_mat_idx || !d_reflect ||
	    !d_vertlist || !d_trilist || !d_rays || !d_active)
		return ugrt_fail(UGRT_EINVAL, "reflect_rays: null argument");
	if (int rc = ugrt_launch_pixels(ctx, UGRT_ST_REFLECT_GEN, k_reflect_rays, d_cam_position, d_t_value, d_ray_dir,
				d_intersect_id, d_mat_idx, d_reflect, num_materials, d_vertlist, d_trilist, eps,
				d_rays, d_active))
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
	if (int rc = ugrt_launch_pixels(ctx, UGRT_ST_REFLECT_GEN, k_reflect_rays_next, d_rays, d_active, d_hit_t,
				d_hit_id, d_mat_idx, d_reflect, num_materials, d_vertlist, d_trilist, eps, d_rays_next,
				d_active_next))
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
	if (int rc = ugrt_launch_pixels(ctx, UGRT_ST_REFLECT_GEN, k_refract_rays, d_cam_position, d_t_value, d_ray_dir,
				d_intersect_id, d_mat_idx, d_reflect, d_transmit, d_ior, num_materials, d_vertlist,
				d_trilist, eps, d_rays, d_active))
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
	if (int rc = ugrt_launch_pixels(ctx, UGRT_ST_REFLECT_GEN, k_refract_rays_next, d_rays, d_active, d_hit_t,
				d_hit_id, d_mat_idx, d_reflect, d_transmit, d_ior, num_materials, d_vertlist,
				d_trilist, eps, d_rays_next, d_active_next))
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
	return ugrt_launch_pixels(ctx, UGRT_ST_REFLECT_GEN, k_occlusion_rays, d_rays, d_active, d_hit_t, d_hit_id,
				d_vertlist, d_trilist, light_pos[0], light_pos[1], light_pos[2], eps, d_orays,
				d_oactive);
}

extern "C" int ugrt_ao_rays(ugrt_ctx *ctx, const float *d_cam_position, const float *d_t_value, const float *d_ray_dir,
			    const int *d_intersect_id, const float *d_vertlist, const int *d_trilist, float eps,
			    float *d_orays, int *d_oactive)
{
	if (!ctx || !d_cam_position || !d_t_value || !d_ray_dir || !d_intersect_id || !d_vertlist || !d_trilist || !d_orays ||
	    !d_oactive)
		return ugrt_fail(UGRT_EINVAL, "ao_rays: null argument");
	return ugrt_launch_pixels(ctx, UGRT_ST_REFLECT_GEN, k_ao_rays, d_cam_position, d_t_value, d_ray_dir,
				d_intersect_id, d_vertlist, d_trilist, eps, d_orays, d_oactive);
}
