/*
 * area_sets_ref.c -- CPU restatement of the gather and the shading of DESIGN.md section 6.8, the checker of
 * ugrt_filter_visibility and ugrt_shade_area_vis (tests/test_filter_visibility.py builds and loads it; so does
 * tests/test_area_sets.py for the frames).
 *
 * Test infrastructure only.  The walk over sample sets has no restatement here: its expected masks are cpu_mask of
 * tests/test_area_light.py once per set, selected per pixel by sets_select below.  Build: gcc -O2 -fPIC
 * -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.  Arrays are indexed by absolute pixel
 * p = y * W + x of a W*H frame; a band is the rows row0 .. row1 - 1.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

/* out[p] = masks[k(p) * N + p] for the pixels of the band, k(p) = (y % set_h) * set_w + (x % set_w) */
void sets_select(const unsigned *masks, int set_w, int set_h, int W, int H, int row0, int row1, unsigned *out)
{
	int x, y;
	size_t N = (size_t)W * (size_t)H;
	for (y = row0; y < row1; y++)
		for (x = 0; x < W; x++) {
			size_t p = (size_t)y * W + x;
			out[p] = masks[(size_t)((y % set_h) * set_w + (x % set_w)) * N + p];
		}
}

static unsigned open_bits(unsigned m, int S)
{
	unsigned dark = 0;
	int s;
	for (s = 0; s < S; s++)
		dark += (m >> s) & 1u;
	return (unsigned)S - dark;
}

/* vis[2p] = sum of w * open_q, vis[2p + 1] = sum of w over the accepted q; inactive pixels of the band: (0, 0) */
void sets_filter(const unsigned *mask, int S, const float *orays, const int *oactive, int R, float normal_cos,
		 float plane_tol, int W, int H, int row0, int row1, unsigned *vis)
{
	int y;
	(void)H;
#pragma omp parallel for schedule(static)
	for (y = row0; y < row1; y++) {
		int x, dx, dy, k;
		for (x = 0; x < W; x++) {
			size_t p = (size_t)y * W + x;
			unsigned num = 0, den = 0;
			const float *op = orays + p * 6, *np = op + 3;
			if (oactive[p]) {
				for (dy = -R; dy <= R; dy++)
					for (dx = -R; dx <= R; dx++) {
						int qx = x + dx, qy = y + dy, same = dx == 0 && dy == 0;
						size_t q;
						if (qx < 0 || qx >= W || qy < row0 || qy >= row1)
							continue;
						q = (size_t)qy * W + qx;
						if (!oactive[q])
							continue;
						if (!same) {
							const float *oq = orays + q * 6, *nq = oq + 3;
							float d[3], cosine, dist;
							for (k = 0; k < 3; k++)
								d[k] = oq[k] - op[k];
							cosine = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
							dist = (d[0] * np[0] + d[1] * np[1]) + d[2] * np[2];
							same = cosine >= normal_cos && __builtin_fabsf(dist) <= plane_tol;
						}
						if (same) {
							unsigned w = (unsigned)((R + 1 - (dx < 0 ? -dx : dx)) * (R + 1 - (dy < 0 ? -dy : dy)));
							num += w * open_bits(mask[q], S);
							den += w;
						}
					}
			}
			vis[2 * p] = num;
			vis[2 * p + 1] = den;
		}
	}
}

/* den = vis[2p + 1] != 0: each byte b becomes (b * (S * den + 2 * num)) / (3 * S * den) */
void sets_shade(unsigned char *img, const unsigned *vis, int num_samples, int p0, int n)
{
	int i, k;
	for (i = 0; i < n; i++) {
		size_t p = (size_t)p0 + i;
		unsigned num = vis[2 * p], den = vis[2 * p + 1], S = (unsigned)num_samples;
		if (den == 0)
			continue;
		for (k = 0; k < 3; k++)
			img[p * 3 + k] = (unsigned char)(((unsigned)img[p * 3 + k] * (S * den + 2u * num)) / (3u * S * den));
	}
}
