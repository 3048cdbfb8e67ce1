// ugrt_filter.hip -- the edge-aware gather over mask words (not in the reference).  Interleaved
// sample sets (ugrt_trace_dda_any_area_sets) give neighbouring pixels different S points of the light; the gather sums
// the open bits of the pixels around p that lie on p's surface, with a tent weight, and ugrt_shade_area_vis
// (ugrt_shade.hip) turns the two sums into ugrt_shade_area's byte.
#include "ugrt_dev.h"

#define FV_TW 32 // tile: FV_TH / 8 pixels per lane of a 256-lane workgroup, a wave = two rows of 32
#ifndef FV_TH
#define FV_TH 8 // (a multiple of 8; make EXTRA=-DFV_TH=16 builds the taller tile that DESIGN.md section 6.8 measures)
#endif
static_assert(FV_TH % 8 == 0 && FV_TH >= 8 && FV_TH <= 32, "tile height" /* 63 KB of LDS at radius 8 */);
#define FV_ACTIVE 0x80000000u

// (dynamic LDS, its base 16-byte aligned: seven planes of LW * LH words, each a multiple of 16 bytes)
extern __shared__ __attribute__((aligned(16))) u32 s_fv[];

// The tile and its halo of R are staged once as structure-of-arrays: o[3], n[3] and one word = open | FV_ACTIVE (0 for a
// pixel outside the image, outside the band's rows or inactive: it is never accepted, and its floats are zeros).  A
// staged row is LW = FV_TW + 2R words; the 32 lanes of a half-wave read 32 consecutive words of one row for every
// (dx, dy), which is conflict-free for ds_read_b32 at any row stride.  The loops over (dx, dy) are uniform in R, every
// index lies inside the staged rectangle for every lane (pixels of the tile past the image's edge included), so no lane
// is masked off before the stores.
//
// GI: the same window, weights and acceptance tests over the indirect light's byte sums (ugrt_gi_filter; DESIGN.md section
// 6.10): `mask` is d_sum, four words per pixel, the three sums of at most 32 * 255 < 2^13 each are staged as
// r | g << 13 beside FV_ACTIVE and b in an eighth plane, and `vis` is d_acc: the three weighted sums and the weight sum.
template <bool GI>
__device__ __forceinline__ void d_filter_tile(const u32 *__restrict__ mask, const float *__restrict__ orays,
					      const int *__restrict__ oactive, u32 S, u32 low_bits, int R, float normal_cos,
					      float plane_tol, int W, int row0, int row1, u32 *__restrict__ vis)
{
	const int LW = FV_TW + 2 * R, LH = FV_TH + 2 * R;
	const int plane = (LW * LH + 3) & ~3;
	u32 *s_blue = s_fv + 7 * plane; // (GI only)
	u32 *s_word = s_fv;
	float *s_o0 = (float *)(s_fv + plane), *s_o1 = (float *)(s_fv + 2 * plane), *s_o2 = (float *)(s_fv + 3 * plane);
	float *s_n0 = (float *)(s_fv + 4 * plane), *s_n1 = (float *)(s_fv + 5 * plane), *s_n2 = (float *)(s_fv + 6 * plane);
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int x0 = (int)blockIdx.x * FV_TW, y0 = row0 + (int)blockIdx.y * FV_TH;
	// staging: a wave per row (LW <= 48 lanes of it)
	for (int ly = wave; ly < LH; ly += PX_THREADS / 64) {
		const int lx = lane, gx = x0 - R + lx, gy = y0 - R + ly;
		if (lx < LW) {
			u32 word = 0u, blue = 0u;
			float v[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
			if (gx >= 0 && gx < W && gy >= row0 && gy < row1) {
				const size_t q = (size_t)gy * (size_t)W + (size_t)gx;
				if (oactive[q] != 0) {
					if constexpr (GI) {
						const uint4 sums = *(const uint4 *)(mask + 4 * q);
						word = sums.x | (sums.y << 13) | FV_ACTIVE;
						blue = sums.z;
					} else {
						word = (S - (u32)__popc(mask[q] & low_bits)) | FV_ACTIVE;
					}
#pragma unroll
					for (int k = 0; k < 6; k++)
						v[k] = orays[q * 6 + k];
				}
			}
			const int at = ly * LW + lx;
			s_word[at] = word;
			if constexpr (GI)
				s_blue[at] = blue;
			s_o0[at] = v[0];
			s_o1[at] = v[1];
			s_o2[at] = v[2];
			s_n0[at] = v[3];
			s_n1[at] = v[4];
			s_n2[at] = v[5];
		}
	}
	__syncthreads();
	const int tx = tid & (FV_TW - 1);
	for (int ty = tid / FV_TW; ty < FV_TH; ty += PX_THREADS / FV_TW) {
		const int c = (ty + R) * LW + tx + R;
		const u32 wp = s_word[c];
		const float op0 = s_o0[c], op1 = s_o1[c], op2 = s_o2[c], np0 = s_n0[c], np1 = s_n1[c], np2 = s_n2[c];
		u32 num = 0u, den = 0u, num_g = 0u, num_b = 0u; // (GI: num is red's)
		for (int dy = -R; dy <= R; dy++) {
			const u32 wy = (u32)(R + 1 - (dy < 0 ? -dy : dy));
			for (int dx = -R; dx <= R; dx++) {
				const int at = c + dy * LW + dx;
				const u32 wq = s_word[at];
				const float d0 = s_o0[at] - op0, d1 = s_o1[at] - op1, d2 = s_o2[at] - op2;
				const float cosine = (np0 * s_n0[at] + np1 * s_n1[at]) + np2 * s_n2[at];
				const float dist = (d0 * np0 + d1 * np1) + d2 * np2;
				const bool same = (dx == 0 && dy == 0) || (cosine >= normal_cos && __builtin_fabsf(dist) <= plane_tol);
				if ((wq & FV_ACTIVE) != 0u && same) {
					const u32 w = wy * (u32)(R + 1 - (dx < 0 ? -dx : dx));
					if constexpr (GI) {
						num += w * (wq & 0x1FFFu);
						num_g += w * ((wq >> 13) & 0x1FFFu);
						num_b += w * s_blue[at];
					} else {
						num += w * (wq & ~FV_ACTIVE);
					}
					den += w;
				}
			}
		}
		const int px = x0 + tx, py = y0 + ty;
		if (px < W && py < row1) {
			const size_t p = (size_t)py * (size_t)W + (size_t)px;
			const bool act = (wp & FV_ACTIVE) != 0u;
			if constexpr (GI) {
				*(uint4 *)(vis + 4 * p) = act ? make_uint4(num, num_g, num_b, den) : make_uint4(0u, 0u, 0u, 0u);
			} else {
				vis[2 * p] = act ? num : 0u;
				vis[2 * p + 1] = act ? den : 0u;
			}
		}
	}
}

__global__ __launch_bounds__(PX_THREADS) void k_filter_visibility(const u32 *__restrict__ mask, const float *__restrict__ orays,
								   const int *__restrict__ oactive, u32 S, u32 low_bits, int R,
								   float normal_cos, float plane_tol, int W, int row0, int row1,
								   u32 *__restrict__ vis)
{
	d_filter_tile<false>(mask, orays, oactive, S, low_bits, R, normal_cos, plane_tol, W, row0, row1, vis);
}

__global__ __launch_bounds__(PX_THREADS) void k_gi_filter(const u32 *__restrict__ sum, const float *__restrict__ orays,
							   const int *__restrict__ oactive, int R, float normal_cos, float plane_tol,
							   int W, int row0, int row1, u32 *__restrict__ acc)
{
	d_filter_tile<true>(sum, orays, oactive, 0u, 0u, R, normal_cos, plane_tol, W, row0, row1, acc);
}

// what both exports check of the window, and the launch's geometry: the tiles over the band's rows and the LDS of `planes`
// staged words per pixel (seven, and the blue sums' eighth); rows < 1: nothing to launch
struct FilterLaunch {
	int W, row0, rows;
	dim3 grid;
	size_t lds;
};
static int filter_geometry(ugrt_ctx *ctx, const char *who, int radius, float plane_tol, int planes, FilterLaunch *f)
{
	if (radius < 0 || radius > UGRT_MAX_FILTER_RADIUS)
		return ugrt_fail(UGRT_EINVAL, "%s: radius %d is not in 0..%d", who, radius, UGRT_MAX_FILTER_RADIUS);
	if (!(plane_tol >= 0.0f))
		return ugrt_fail(UGRT_EINVAL, "%s: plane_tol must be 0 or greater", who);
	UGRT_HIP(hipSetDevice(ctx->device));
	f->W = ctx->cfg.width;
	f->row0 = ctx->p0 / f->W;
	f->rows = ctx->npix / f->W;
	const int LW = FV_TW + 2 * radius, LH = FV_TH + 2 * radius;
	f->grid = dim3((f->W + FV_TW - 1) / FV_TW, (f->rows + FV_TH - 1) / FV_TH);
	f->lds = (size_t)planes * (size_t)((LW * LH + 3) & ~3) * sizeof(u32); // 31.5 KB (GI: 36 KB) at radius 8 with FV_TH 8
	return UGRT_OK;
}

extern "C" int ugrt_filter_visibility(ugrt_ctx *ctx, const unsigned *d_mask, int num_bits, const float *d_orays,
				      const int *d_oactive, int radius, float normal_cos, float plane_tol, unsigned *d_vis)
{
	if (!ctx || !d_mask || !d_orays || !d_oactive || !d_vis)
		return ugrt_fail(UGRT_EINVAL, "filter_visibility: null argument");
	if (num_bits < 1 || num_bits > 32)
		return ugrt_fail(UGRT_EINVAL, "filter_visibility: num_bits %d is not in 1..32", num_bits);
	FilterLaunch f;
	if (int rc = filter_geometry(ctx, "filter_visibility", radius, plane_tol, 7, &f))
		return rc;
	if (f.rows < 1)
		return UGRT_OK;
	const u32 low_bits = num_bits == 32 ? 0xFFFFFFFFu : (1u << num_bits) - 1u;
	ugrt_prof_begin(ctx, UGRT_ST_SHADE);
	hipLaunchKernelGGL(k_filter_visibility, f.grid, dim3(PX_THREADS), f.lds, ctx->stream, d_mask, d_orays, d_oactive,
			   (u32)num_bits, low_bits, radius, normal_cos, plane_tol, f.W, f.row0, f.row0 + f.rows, d_vis);
	ugrt_prof_end(ctx, UGRT_ST_SHADE);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}

extern "C" int ugrt_gi_filter(ugrt_ctx *ctx, const unsigned *d_sum, const float *d_orays, const int *d_oactive, int radius,
			      float normal_cos, float plane_tol, unsigned *d_acc)
{
	if (!ctx || !d_sum || !d_orays || !d_oactive || !d_acc)
		return ugrt_fail(UGRT_EINVAL, "gi_filter: null argument");
	if ((((size_t)d_sum | (size_t)d_acc) & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "gi_filter: d_sum and d_acc must be 16-byte aligned");
	FilterLaunch f;
	if (int rc = filter_geometry(ctx, "gi_filter", radius, plane_tol, 8, &f))
		return rc;
	if (f.rows < 1)
		return UGRT_OK;
	ugrt_prof_begin(ctx, UGRT_ST_SHADE);
	hipLaunchKernelGGL(k_gi_filter, f.grid, dim3(PX_THREADS), f.lds, ctx->stream, d_sum, d_orays, d_oactive, radius,
			   normal_cos, plane_tol, f.W, f.row0, f.row0 + f.rows, d_acc);
	ugrt_prof_end(ctx, UGRT_ST_SHADE);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}
