// ugrt_aa.hip -- adaptive anti-aliasing: sub-pixel eye rays on edge pixels (not in the reference).
//
// Spec: ugrt_aa_edges flags the pixels whose 3x3 neighbourhood holds a silhouette, a material border, a crease, a depth
// step or a shadow edge.  ugrt_aa_gather sends S eye rays through each flagged pixel -- d_ray_dir's arithmetic at
// (col + sx, row + sy), the offsets of set k(p) of a table in LDS --, finds each ray's closest hit as ugrt_trace_dda finds
// it, gates it as the primary epilogue gates a hit (d_finish_pixel), shades it as k_shade<false> shades a primary hit,
// darkens the bytes to a third where the shadow light is hidden (k_add_shadows' integer division), and sums the bytes of
// the pixel's S rays.  ugrt_aa_resolve (ugrt_shade.hip) writes the rounded mean over the pixel.
// The kernel is k_pixel_gather of ugrt_gather.h (d_closest_walk without a radius) with AaKind of ugrt_eye_kind.h, which
// ugrt_dof.hip derives its lens rays from.  Its own parts:
//   * no ray array is read or written: the lane forms its ray from (p, s) and the eye's 5x5x4 node table, which lies in
//     LDS between the offset table and the staged words;
//   * the depth gate and the primary hit's shading, on bytes from the hit on.
#include "ugrt_eye_kind.h"

extern "C" int ugrt_aa_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
			      const float *d_vertlist, const int *d_trilist, const float *eye_camcoords, const int *d_edge,
			      int num_samples, int set_w, int set_h, const float *d_offsets, const int *d_mat_idx,
			      const float *d_mat_list, int num_materials, const float *shadow_light, float eps, unsigned *d_sum)
{
	if (int rc = eye_gather_check("aa_gather", ctx, d_value_list, d_span, d_offset, d_vertlist, d_trilist, eye_camcoords, d_edge,
				      d_offsets, d_mat_idx, d_mat_list, d_sum, num_samples, set_w, set_h, eps, num_materials))
		return rc;
	AaKind::Arg a = {};
	if (int rc = eye_gather_arg(a, ctx, eye_camcoords, num_samples, set_w, set_h, d_offsets, d_mat_idx, d_mat_list, num_materials,
				    shadow_light, eps, d_sum))
		return rc;
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
