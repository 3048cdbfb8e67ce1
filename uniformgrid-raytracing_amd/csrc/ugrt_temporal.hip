// ugrt_temporal.hip -- temporal accumulation of the stochastic effects' shares (not in the reference; DESIGN.md section
// 6.12).  A frame's gather (ugrt_filter_visibility, ugrt_gi_filter) leaves a pixel's share of open rays, or its mean
// indirect colour, as integer sums; these kernels blend that share into a running mean carried from frame to frame.  The
// mean of the frame before is fetched where the pixel's surface point lay under the previous camera: the point is
// projected with the screen-grid binning's own arithmetic, four taps around the position are weighted in sixteenths of a
// pixel, and a tap counts only where the previous G-buffer holds the same surface (the gather's normal and plane tests).
#include "ugrt_dev.h"

#define TP_TW 32 // tile: a 256-lane workgroup covers 32 x 8 pixels, a wave = two rows of 32: its taps fall into a
#define TP_TH 8  // compact patch of the previous frame
static_assert(TP_TW * TP_TH == PX_THREADS, "one pixel per lane");

// rows 16..47 of the previous eye's dd_camcoords: the modelview and the projection matrix (128 B, by value: SGPRs)
struct PrevCam {
	float m[32];
};

// d_transformed_vertex (grid_kernel.cu:13-36: MV, divide, P, divide) under the previous camera, operand for operand,
// with the projective w of the second divide handed out beside the two image coordinates
__device__ __forceinline__ void d_reproject(const PrevCam &pc, float px, float py, float pz, float *ndc0, float *ndc1, float *w)
{
	const float *m = pc.m;
	float t0 = D_MULMV_ROW(m, 0, 0, px, py, pz);
	float t1 = D_MULMV_ROW(m, 0, 1, px, py, pz);
	float t2 = D_MULMV_ROW(m, 0, 2, px, py, pz);
	float t3 = D_MULMV_ROW(m, 0, 3, px, py, pz);
	const float qx = t0 / t3, qy = t1 / t3, qz = t2 / t3;
	t0 = D_MULMV_ROW(m, 16, 0, qx, qy, qz);
	t1 = D_MULMV_ROW(m, 16, 1, qx, qy, qz);
	t3 = D_MULMV_ROW(m, 16, 3, qx, qy, qz);
	*ndc0 = t0 / t3;
	*ndc1 = t1 / t3;
	*w = t3;
}

// One pixel per lane.  GI = false: `cur` is ugrt_filter_visibility's pair per pixel, the history is (share, frames) and
// `out` the pair over UGRT_TEMPORAL_DEN; GI = true: ugrt_gi_filter's four words, (r, g, b, frames) and four words, moved
// with 16-byte loads and stores (the pairs of the other form need no alignment beyond a word's).  C = the channels.
// Every load of a tap stands behind the tests that can drop it: the active word and the frame count first, the tap's
// position, normal and shares behind them.
template <bool GI>
__device__ __forceinline__ void d_temporal_pixel(const u32 *__restrict__ cur, u32 S, const float *__restrict__ orays,
						 const int *__restrict__ oactive, const PrevCam &pc,
						 const float *__restrict__ prev_orays, const int *__restrict__ prev_oactive,
						 const float *__restrict__ hist_in, float max_frames, float normal_cos, float plane_tol,
						 int W, int H, int row0, int row1, float *__restrict__ hist_out, u32 *__restrict__ out)
{
	constexpr int C = GI ? 3 : 1;
	const int tid = threadIdx.x;
	const int x = (int)blockIdx.x * TP_TW + (tid & (TP_TW - 1)), y = row0 + (int)blockIdx.y * TP_TH + tid / TP_TW;
	if (x >= W || y >= row1)
		return;
	const size_t p = (size_t)y * (size_t)W + (size_t)x;
	u32 num[3] = { 0u, 0u, 0u }, den = 0u;
	if (oactive[p] != 0) {
		if constexpr (GI) {
			const uint4 a = *(const uint4 *)(cur + 4 * p);
			num[0] = a.x, num[1] = a.y, num[2] = a.z, den = a.w;
		} else {
			num[0] = cur[2 * p], den = cur[2 * p + 1];
		}
	}
	if (den == 0u) { // inactive, or active without a pair: zeros, frame count 0
		if constexpr (GI) {
			*(float4 *)(hist_out + 4 * p) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
			*(uint4 *)(out + 4 * p) = make_uint4(0u, 0u, 0u, 0u);
		} else {
			hist_out[2 * p] = hist_out[2 * p + 1] = 0.0f;
			out[2 * p] = out[2 * p + 1] = 0u;
		}
		return;
	}
	const float over = (float)((GI ? 255u : 1u) * S * den);
	float c[C];
#pragma unroll
	for (int k = 0; k < C; k++)
		c[k] = (float)num[k] / over;
	float op[3], np[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		op[k] = orays[6 * p + k];
		np[k] = orays[6 * p + 3 + k];
	}
	float ndc0, ndc1, w;
	d_reproject(pc, op[0], op[1], op[2], &ndc0, &ndc1, &w);
	const float fx = ((ndc0 + 1.0f) / 2.0f) * (float)W, fy = ((ndc1 + 1.0f) / 2.0f) * (float)H;
	float sum[C], nmin = __builtin_inff();
#pragma unroll
	for (int k = 0; k < C; k++)
		sum[k] = 0.0f;
	u32 wsum = 0u;
	// (every comparison with a NaN is false: a NaN in fx, fy or w leaves the pixel without a history)
	if (w > 0.0f && fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) {
		const int X = ugrt_floor2i(fx * 16.0f + 0.5f), Y = ugrt_floor2i(fy * 16.0f + 0.5f);
		const int ix = X >> 4, iy = Y >> 4, ax = X & 15, ay = Y & 15;
#pragma unroll
		for (int tap = 0; tap < 4; tap++) {
			const int i = tap & 1, j = tap >> 1;
			const u32 wt = (u32)((i ? ax : 16 - ax) * (j ? ay : 16 - ay));
			const int qx = ix + i, qy = iy + j;
			if (wt == 0u || qx < 0 || qx >= W || qy < 0 || qy >= H || qy < row0 || qy >= row1)
				continue;
			const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
			if (prev_oactive[q] == 0)
				continue;
			const float frames = hist_in[(GI ? 4 : 2) * q + (GI ? 3 : 1)];
			if (!(frames >= 1.0f))
				continue;
			float hq[C];
			if constexpr (GI) {
				const float4 h = *(const float4 *)(hist_in + 4 * q);
				hq[0] = h.x, hq[1] = h.y, hq[2] = h.z;
			} else {
				hq[0] = hist_in[2 * q];
			}
			bool in_range = true;
#pragma unroll
			for (int k = 0; k < C; k++)
				in_range = in_range && hq[k] >= 0.0f && hq[k] <= 1.0f;
			const float d0 = prev_orays[6 * q] - op[0], d1 = prev_orays[6 * q + 1] - op[1], d2 = prev_orays[6 * q + 2] - op[2];
			const float cosine = (np[0] * prev_orays[6 * q + 3] + np[1] * prev_orays[6 * q + 4]) + np[2] * prev_orays[6 * q + 5];
			const float dist = (d0 * np[0] + d1 * np[1]) + d2 * np[2];
			if (!(in_range && cosine >= normal_cos && __builtin_fabsf(dist) <= plane_tol))
				continue;
#pragma unroll
			for (int k = 0; k < C; k++)
				sum[k] = sum[k] + (float)wt * hq[k];
			wsum += wt;
			const float next = frames + 1.0f;
			nmin = next < nmin ? next : nmin;
		}
	}
	float h[C], n = 1.0f;
	if (wsum != 0u)
		n = nmin < max_frames ? nmin : max_frames;
	if (n == 1.0f) { // no tap counted, or max_frames = 1: the input itself (hp + (c - hp) would miss it by an ulp)
#pragma unroll
		for (int k = 0; k < C; k++)
			h[k] = c[k];
	} else {
#pragma unroll
		for (int k = 0; k < C; k++) {
			const float hp = sum[k] / (float)wsum;
			h[k] = hp + (c[k] - hp) / n;
		}
	}
	const u32 full = (GI ? 255u : 1u) * S * UGRT_TEMPORAL_DEN;
	u32 o[C];
#pragma unroll
	for (int k = 0; k < C; k++) {
		const int v = ugrt_floor2i(h[k] * (float)full + 0.5f);
		o[k] = v < (int)full ? (u32)v : full;
	}
	if constexpr (GI) {
		*(float4 *)(hist_out + 4 * p) = make_float4(h[0], h[1], h[2], n);
		*(uint4 *)(out + 4 * p) = make_uint4(o[0], o[1], o[2], UGRT_TEMPORAL_DEN);
	} else {
		hist_out[2 * p] = h[0];
		hist_out[2 * p + 1] = n;
		out[2 * p] = o[0];
		out[2 * p + 1] = UGRT_TEMPORAL_DEN;
	}
}

__global__ __launch_bounds__(PX_THREADS) void k_temporal_visibility(const u32 *__restrict__ vis, u32 S, const float *__restrict__ orays,
								     const int *__restrict__ oactive, PrevCam pc,
								     const float *__restrict__ prev_orays, const int *__restrict__ prev_oactive,
								     const float *__restrict__ hist_in, float max_frames, float normal_cos,
								     float plane_tol, int W, int H, int row0, int row1,
								     float *__restrict__ hist_out, u32 *__restrict__ vis_out)
{
	d_temporal_pixel<false>(vis, S, orays, oactive, pc, prev_orays, prev_oactive, hist_in, max_frames, normal_cos, plane_tol, W, H,
				row0, row1, hist_out, vis_out);
}

__global__ __launch_bounds__(PX_THREADS) void k_temporal_gi(const u32 *__restrict__ acc, u32 S, const float *__restrict__ orays,
							     const int *__restrict__ oactive, PrevCam pc,
							     const float *__restrict__ prev_orays, const int *__restrict__ prev_oactive,
							     const float *__restrict__ hist_in, float max_frames, float normal_cos, float plane_tol,
							     int W, int H, int row0, int row1, float *__restrict__ hist_out,
							     u32 *__restrict__ acc_out)
{
	d_temporal_pixel<true>(acc, S, orays, oactive, pc, prev_orays, prev_oactive, hist_in, max_frames, normal_cos, plane_tol, W, H,
			       row0, row1, hist_out, acc_out);
}

// what both exports check, and the launch over the band's rows (gi: the four-word form, moved 16 bytes at a time)
static int temporal_launch(ugrt_ctx *ctx, const char *who, const char *count_name, bool gi, const unsigned *d_cur, int count,
			   const float *d_orays, const int *d_oactive, const float *prev_camcoords, const float *d_prev_orays,
			   const int *d_prev_oactive, const float *d_hist_in, int max_frames, float normal_cos, float plane_tol,
			   float *d_hist_out, unsigned *d_out)
{
	if (!ctx || !d_cur || !d_orays || !d_oactive || !prev_camcoords || !d_prev_orays || !d_prev_oactive || !d_hist_in ||
	    !d_hist_out || !d_out)
		return ugrt_fail(UGRT_EINVAL, "%s: null argument", who);
	if (count < 1 || count > 32)
		return ugrt_fail(UGRT_EINVAL, "%s: %s %d is not in 1..32", who, count_name, count);
	if (max_frames < 1 || max_frames > UGRT_MAX_TEMPORAL_FRAMES)
		return ugrt_fail(UGRT_EINVAL, "%s: max_frames %d is not in 1..%d", who, max_frames, UGRT_MAX_TEMPORAL_FRAMES);
	if (!(plane_tol >= 0.0f))
		return ugrt_fail(UGRT_EINVAL, "%s: plane_tol must be 0 or greater", who);
	if (normal_cos != normal_cos)
		return ugrt_fail(UGRT_EINVAL, "%s: normal_cos is a NaN", who);
	if (d_hist_in == d_hist_out)
		return ugrt_fail(UGRT_EINVAL, "%s: d_hist_in and d_hist_out are the same buffer (neighbours are read)", who);
	if (d_cur == d_out)
		return ugrt_fail(UGRT_EINVAL, "%s: %s is the same buffer as the input (neighbours are read)", who,
				 gi ? "d_acc_out" : "d_vis_out");
	if (gi && (((size_t)d_cur | (size_t)d_out | (size_t)d_hist_in | (size_t)d_hist_out) & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "%s: d_acc, d_hist_in, d_hist_out and d_acc_out must be 16-byte aligned", who);
	UGRT_HIP(hipSetDevice(ctx->device));
	const int W = ctx->cfg.width, H = ctx->cfg.height, row0 = ctx->p0 / W, rows = ctx->npix / W;
	if (rows < 1)
		return UGRT_OK;
	PrevCam pc;
	for (int k = 0; k < 32; k++)
		pc.m[k] = prev_camcoords[16 + k];
	const dim3 grid((W + TP_TW - 1) / TP_TW, (rows + TP_TH - 1) / TP_TH);
	ugrt_prof_begin(ctx, UGRT_ST_SHADE);
	if (gi)
		hipLaunchKernelGGL(k_temporal_gi, grid, dim3(PX_THREADS), 0, ctx->stream, d_cur, (u32)count, d_orays, d_oactive, pc,
				   d_prev_orays, d_prev_oactive, d_hist_in, (float)max_frames, normal_cos, plane_tol, W, H, row0,
				   row0 + rows, d_hist_out, d_out);
	else
		hipLaunchKernelGGL(k_temporal_visibility, grid, dim3(PX_THREADS), 0, ctx->stream, d_cur, (u32)count, d_orays, d_oactive,
				   pc, d_prev_orays, d_prev_oactive, d_hist_in, (float)max_frames, normal_cos, plane_tol, W, H, row0,
				   row0 + rows, d_hist_out, d_out);
	ugrt_prof_end(ctx, UGRT_ST_SHADE);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}

extern "C" int ugrt_temporal_visibility(ugrt_ctx *ctx, const unsigned *d_vis, int num_bits, const float *d_orays,
					const int *d_oactive, const float *prev_camcoords, const float *d_prev_orays,
					const int *d_prev_oactive, const float *d_hist_in, int max_frames, float normal_cos,
					float plane_tol, float *d_hist_out, unsigned *d_vis_out)
{
	return temporal_launch(ctx, "temporal_visibility", "num_bits", false, d_vis, num_bits, d_orays, d_oactive, prev_camcoords,
			       d_prev_orays, d_prev_oactive, d_hist_in, max_frames, normal_cos, plane_tol, d_hist_out, d_vis_out);
}

extern "C" int ugrt_temporal_gi(ugrt_ctx *ctx, const unsigned *d_acc, int num_dirs, const float *d_orays, const int *d_oactive,
				const float *prev_camcoords, const float *d_prev_orays, const int *d_prev_oactive,
				const float *d_hist_in, int max_frames, float normal_cos, float plane_tol, float *d_hist_out,
				unsigned *d_acc_out)
{
	return temporal_launch(ctx, "temporal_gi", "num_dirs", true, d_acc, num_dirs, d_orays, d_oactive, prev_camcoords, d_prev_orays,
			       d_prev_oactive, d_hist_in, max_frames, normal_cos, plane_tol, d_hist_out, d_acc_out);
}
