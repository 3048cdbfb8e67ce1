// ugrt_dof.hip -- depth of field: thin-lens eye rays on the pixels whose blur matters (not in the reference; DESIGN.md
// section 6.17).
//
// Spec: ugrt_dof_pixels flags the pixels whose own circle of confusion, or a neighbour's, reaches them.  ugrt_dof_gather
// sends S lens rays through each flagged pixel: the eye ray of ugrt_aa_gather through (col + sx, row + sy), its origin
// moved by L = lu * U + lv * V on the lens and its direction tilted by -L / s_f, s_f = F / (d0 . A), so that all lens
// rays of one image point meet on the plane A . (P - eye) = F.  The rest is ugrt_aa_gather's on {o, d}: the closest hit,
// the depth gate, the primary hit's shading, the occlusion ray, the byte sums.  ugrt_aa_resolve writes the mean.
// The kernel is k_pixel_gather of ugrt_gather.h with the Kind below: AaKind (ugrt_eye_kind.h) with four floats per table
// entry and its own ray().  U, V, A and F lie in the Late block in LDS and are read where the ray is formed: the lens
// costs no register over the walks.
#include "ugrt_eye_kind.h"

struct DofKind : AaKind {
	struct Late : AaKind::Late {
		float lens[10]; // U[3], V[3], A[3], F
	};
	struct Arg : GatherArg { // table: [set_w * set_h][S][4], (sx, sy, lu, lv)
		Late late;
		float tex[AA_TEX];
	};
	static constexpr u32 entry = 4u;
	static __device__ __forceinline__ void ray(const Late &late, const float *ent, const float *tex, const float *rays, int p,
						   u32 x, u32 y, float *o, float *d)
	{
		const float4 e = *(const float4 *)ent; // (sx, sy, lu, lv): one 16-byte LDS read
		const float off[2] = { e.x, e.y };
		AaKind::ray(late, off, tex, rays, p, x, y, o, d);
		// a point of the lens outside the unit square is clamped to it, a NaN is the lens's centre
		const float lu = e.z != e.z ? 0.0f : fminf(fmaxf(e.z, -1.0f), 1.0f);
		const float lv = e.w != e.w ? 0.0f : fminf(fmaxf(e.w, -1.0f), 1.0f);
		const float c = (d[0] * late.lens[6] + d[1] * late.lens[7]) + d[2] * late.lens[8];
		if (!(c > 0)) // the view axis points away from the ray: the pinhole ray
			return;
		const float s_f = late.lens[9] / c;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const float L = lu * late.lens[k] + lv * late.lens[3 + k];
			o[k] = o[k] + L;
			d[k] = d[k] - L / s_f;
		}
	}
};

extern "C" int ugrt_dof_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
			       const float *d_vertlist, const int *d_trilist, const float *eye_camcoords, const float *lens,
			       const int *d_flags, int num_samples, int set_w, int set_h, const float *d_table, const int *d_mat_idx,
			       const float *d_mat_list, int num_materials, const float *shadow_light, float eps, unsigned *d_sum)
{
	if (!lens)
		return ugrt_fail(UGRT_EINVAL, "dof_gather: null argument");
	if (int rc = eye_gather_check("dof_gather", ctx, d_value_list, d_span, d_offset, d_vertlist, d_trilist, eye_camcoords, d_flags,
				      d_table, d_mat_idx, d_mat_list, d_sum, num_samples, set_w, set_h, eps, num_materials))
		return rc;
	static const char *const part[3] = { "U", "V", "A" };
	for (int k = 0; k < 9; k++)
		if (!__builtin_isfinite(lens[k]))
			return ugrt_fail(UGRT_EINVAL, "dof_gather: lens %s[%d] is not finite", part[k / 3], k % 3);
	if (!__builtin_isfinite(lens[9]) || !(lens[9] > 0.0f))
		return ugrt_fail(UGRT_EINVAL, "dof_gather: lens F %g is not a finite distance above 0", (double)lens[9]);
	DofKind::Arg a = {};
	if (int rc = eye_gather_arg(a, ctx, eye_camcoords, num_samples, set_w, set_h, d_table, d_mat_idx, d_mat_list, num_materials,
				    shadow_light, eps, d_sum))
		return rc;
	for (int k = 0; k < 10; k++)
		a.late.lens[k] = lens[k];
	return pixel_gather<DofKind>({ ctx, d_value_list, d_span, d_offset, d_vertlist, d_trilist, nullptr, d_flags, d_sum }, a,
				     shadow_light != nullptr);
}

// ---------------------------------------------------------------------------
// Which pixels get lens rays.  One launch, no intermediate array: a workgroup owns DP_TW x DP_TH pixels, forms the reach
// of every pixel of the tile and of a border of R pixels around it in LDS -- floor(coc) capped at R where coc >= coc_min,
// -1 otherwise; coc >= m for an integer m >= 0 is floor(coc) >= m --, and dilates in two passes over LDS: per row the
// largest reach among the sources that reach the column, then per column that reach against |dy|.  2 (2R + 1) LDS reads
// per pixel in the place of (2R + 1)^2 reads through L2; the border is formed again by the neighbouring workgroups, 1.7
// times the tile's pixels at R = 4 and 2.5 times at R = 8.
// ---------------------------------------------------------------------------
#define DP_TW 64
#define DP_TH 16
#define DP_MAXR UGRT_MAX_DOF_WINDOW

__global__ __launch_bounds__(PX_THREADS) void k_dof_pixels(const float *__restrict__ t_value, const float *__restrict__ dir,
							    const int *__restrict__ ids, float A0, float A1, float A2, float F,
							    float coc_scale, float coc_min, int R, int W, int H, int *__restrict__ flag,
							    int p0, int n)
{
	__shared__ signed char s_reach[(DP_TH + 2 * DP_MAXR) * (DP_TW + 2 * DP_MAXR)];
	__shared__ signed char s_row[(DP_TH + 2 * DP_MAXR) * DP_TW];
	const int tid = threadIdx.x;
	const int bx = blockIdx.x * DP_TW, by = p0 / W + blockIdx.y * DP_TH;
	const int LW = DP_TW + 2 * R, LH = DP_TH + 2 * R;
	for (int i = tid; i < LW * LH; i += PX_THREADS) {
		const int ly = i / LW, lx = i - ly * LW;
		const int qx = bx - R + lx, qy = by - R + ly;
		int reach = -1;
		if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
			const int q = qy * W + qx;
			const float t = t_value[q];
			float coc = 0.0f;
			if (t > 0 && ids[q] >= 0) {
				const float z = t * ((dir[3 * q] * A0 + dir[3 * q + 1] * A1) + dir[3 * q + 2] * A2);
				if (z > 0)
					coc = coc_scale * __builtin_fabsf(z - F) / z;
			}
			if (coc >= coc_min && coc >= 0.0f)
				reach = (int)fminf(coc, (float)R);
		}
		s_reach[i] = (signed char)reach;
	}
	__syncthreads();
	for (int i = tid; i < LH * DP_TW; i += PX_THREADS) {
		const int ly = i / DP_TW, x = i - ly * DP_TW;
		int best = -1;
		for (int dx = -R; dx <= R; dx++) {
			const int r = s_reach[ly * LW + x + R + dx];
			if (r >= (dx < 0 ? -dx : dx) && r > best)
				best = r;
		}
		s_row[i] = (signed char)best;
	}
	__syncthreads();
	for (int i = tid; i < DP_TH * DP_TW; i += PX_THREADS) {
		const int y = i / DP_TW, x = i - y * DP_TW;
		int f = 0;
		for (int dy = -R; dy <= R; dy++)
			if (s_row[(y + R + dy) * DP_TW + x] >= (dy < 0 ? -dy : dy))
				f = 1;
		const int px = bx + x, py = by + y;
		if (px < W && py < H) {
			const int p = py * W + px;
			if (p >= p0 && p < p0 + n)
				flag[p] = f;
		}
	}
}

extern "C" int ugrt_dof_pixels(ugrt_ctx *ctx, const float *d_t_value, const float *d_ray_dir, const int *d_intersect_id,
			       const float *axis, float focus, float coc_scale, float coc_min, int radius, int *d_flags)
{
	if (!ctx || !d_t_value || !d_ray_dir || !d_intersect_id || !axis || !d_flags)
		return ugrt_fail(UGRT_EINVAL, "dof_pixels: null argument");
	for (int k = 0; k < 3; k++)
		if (axis[k] != axis[k])
			return ugrt_fail(UGRT_EINVAL, "dof_pixels: axis[%d] is not a number", k);
	if (focus != focus)
		return ugrt_fail(UGRT_EINVAL, "dof_pixels: focus is not a number");
	if (coc_scale != coc_scale)
		return ugrt_fail(UGRT_EINVAL, "dof_pixels: coc_scale is not a number");
	if (coc_min != coc_min)
		return ugrt_fail(UGRT_EINVAL, "dof_pixels: coc_min is not a number");
	if (radius < 0 || radius > UGRT_MAX_DOF_WINDOW)
		return ugrt_fail(UGRT_EINVAL, "dof_pixels: radius %d is not in 0..%d", radius, UGRT_MAX_DOF_WINDOW);
	if (ctx->npix <= 0)
		return UGRT_OK;
	UGRT_HIP(hipSetDevice(ctx->device));
	const int W = ctx->cfg.width;
	const int rows = (ctx->p0 + ctx->npix - 1) / W - ctx->p0 / W + 1;
	ugrt_prof_begin(ctx, UGRT_ST_SHADE);
	hipLaunchKernelGGL(k_dof_pixels, dim3((W + DP_TW - 1) / DP_TW, (rows + DP_TH - 1) / DP_TH), dim3(PX_THREADS), 0, ctx->stream,
			   d_t_value, d_ray_dir, d_intersect_id, axis[0], axis[1], axis[2], focus, coc_scale, coc_min, radius, W,
			   ctx->cfg.height, d_flags, ctx->p0, ctx->npix);
	ugrt_prof_end(ctx, UGRT_ST_SHADE);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}
