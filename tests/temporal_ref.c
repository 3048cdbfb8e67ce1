/*
 * temporal_ref.c -- CPU restatement of the temporal accumulation of DESIGN.md section 6.12, the checker of
 * ugrt_temporal_visibility and ugrt_temporal_gi (tests/test_temporal.py builds and loads it).
 *
 * Test infrastructure only.  One loop per pixel, the rule of include/ugrt.h in its stated order.  Build: gcc -O2 -fPIC
 * -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.  Arrays are indexed by absolute pixel
 * p = y * W + x of a W*H frame; a band is the rows row0 .. row1 - 1.  C = 1: the pair form (cur, out: 2 words, hist: 2
 * floats per pixel); C = 3: the GI form (4 and 4).
 */
#include <stddef.h>

#include "ugrt_fmath.h"

#define MULMV_ROW(m, base, r, x, y, z) \
	(m[(base) + (r)] * (x) + m[(base) + 4 + (r)] * (y) + m[(base) + 8 + (r)] * (z) + m[(base) + 12 + (r)] * 1.0f)

/* the reference's vertex transform (MV, divide, P, divide) under camcoords cc; out = {fx, fy, w} */
void temporal_project(const float *cc, const float *o, int W, int H, float *out)
{
	float t0 = MULMV_ROW(cc, 16, 0, o[0], o[1], o[2]);
	float t1 = MULMV_ROW(cc, 16, 1, o[0], o[1], o[2]);
	float t2 = MULMV_ROW(cc, 16, 2, o[0], o[1], o[2]);
	float t3 = MULMV_ROW(cc, 16, 3, o[0], o[1], o[2]);
	float qx = t0 / t3, qy = t1 / t3, qz = t2 / t3;
	float ndc0, ndc1;
	t0 = MULMV_ROW(cc, 32, 0, qx, qy, qz);
	t1 = MULMV_ROW(cc, 32, 1, qx, qy, qz);
	t3 = MULMV_ROW(cc, 32, 3, qx, qy, qz);
	ndc0 = t0 / t3;
	ndc1 = t1 / t3;
	out[0] = ((ndc0 + 1.0f) / 2.0f) * (float)W;
	out[1] = ((ndc1 + 1.0f) / 2.0f) * (float)H;
	out[2] = t3;
}

/* taps[5p ..] (may be NULL): ix, iy, ax, ay of an active pixel with a position inside the window (else -9 four times),
 * and the bit mask of the taps that counted */
void temporal_blend(int C, const unsigned *cur, int S, const float *orays, const int *oactive, const float *prev_cc,
		    const float *prev_orays, const int *prev_oactive, const float *hist_in, int max_frames, float normal_cos,
		    float plane_tol, int W, int H, int row0, int row1, float *hist_out, unsigned *out, int *taps)
{
	int y;
	const int CW = C == 3 ? 4 : 2; /* words per pixel */
#pragma omp parallel for schedule(static)
	for (y = row0; y < row1; y++) {
		int x, k, tap;
		for (x = 0; x < W; x++) {
			size_t p = (size_t)y * W + x;
			const float *op = orays + 6 * p, *np = op + 3;
			unsigned den = oactive[p] ? cur[CW * p + CW - 1] : 0u, wsum = 0u, full;
			float c[3], sum[3] = { 0.0f, 0.0f, 0.0f }, h[3], n = 1.0f, nmin = __builtin_inff(), over, f[3];
			if (taps)
				for (k = 0; k < 5; k++)
					taps[5 * p + k] = k < 4 ? -9 : 0;
			if (den == 0u) {
				for (k = 0; k < CW; k++) {
					hist_out[CW * p + k] = 0.0f;
					out[CW * p + k] = 0u;
				}
				continue;
			}
			over = (float)((C == 3 ? 255u : 1u) * (unsigned)S * den);
			for (k = 0; k < C; k++)
				c[k] = (float)cur[CW * p + k] / over;
			temporal_project(prev_cc, op, W, H, f);
			if (f[2] > 0.0f && f[0] > -1.0f && f[0] < (float)W && f[1] > -1.0f && f[1] < (float)H) {
				int X = ugrt_floor2i(f[0] * 16.0f + 0.5f), Y = ugrt_floor2i(f[1] * 16.0f + 0.5f);
				int ix = X >> 4, iy = Y >> 4, ax = X & 15, ay = Y & 15;
				if (taps)
					taps[5 * p] = ix, taps[5 * p + 1] = iy, taps[5 * p + 2] = ax, taps[5 * p + 3] = ay;
				for (tap = 0; tap < 4; tap++) {
					int i = tap & 1, j = tap >> 1, qx = ix + i, qy = iy + j, ok = 1;
					unsigned w = (unsigned)((i ? ax : 16 - ax) * (j ? ay : 16 - ay));
					const float *oq, *nq, *hq;
					float d[3], cosine, dist, frames;
					size_t q;
					if (w == 0u || qx < 0 || qx >= W || qy < 0 || qy >= H || qy < row0 || qy >= row1)
						continue;
					q = (size_t)qy * W + qx;
					if (!prev_oactive[q])
						continue;
					hq = hist_in + CW * q;
					frames = hq[CW - 1];
					if (!(frames >= 1.0f))
						continue;
					for (k = 0; k < C; k++)
						ok = ok && hq[k] >= 0.0f && hq[k] <= 1.0f;
					oq = prev_orays + 6 * q, nq = oq + 3;
					for (k = 0; k < 3; k++)
						d[k] = oq[k] - op[k];
					cosine = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
					dist = (d[0] * np[0] + d[1] * np[1]) + d[2] * np[2];
					if (!(ok && cosine >= normal_cos && __builtin_fabsf(dist) <= plane_tol))
						continue;
					for (k = 0; k < C; k++)
						sum[k] = sum[k] + (float)w * hq[k];
					wsum += w;
					if (frames + 1.0f < nmin)
						nmin = frames + 1.0f;
					if (taps)
						taps[5 * p + 4] |= 1 << tap;
				}
			}
			if (wsum != 0u)
				n = nmin < (float)max_frames ? nmin : (float)max_frames;
			if (n == 1.0f) { /* no tap counted, or max_frames = 1 */
				for (k = 0; k < C; k++)
					h[k] = c[k];
			} else {
				for (k = 0; k < C; k++) {
					float hp = sum[k] / (float)wsum;
					h[k] = hp + (c[k] - hp) / n;
				}
			}
			full = (C == 3 ? 255u : 1u) * (unsigned)S * 256u;
			for (k = 0; k < C; k++) {
				int v = ugrt_floor2i(h[k] * (float)full + 0.5f);
				hist_out[CW * p + k] = h[k];
				out[CW * p + k] = v < (int)full ? (unsigned)v : full;
			}
			hist_out[CW * p + C] = n;
			out[CW * p + C] = 256u;
		}
	}
}
