/*
 * ambient_sets_ref.c -- CPU restatement of ugrt_ao_shade_vis, the shading behind the gather over
 * the hemisphere masks (tests/test_ambient_sets.py builds and loads it).
 *
 * Test infrastructure only.  The walk over direction sets has no restatement here: its expected masks are cpu_mask of
 * tests/test_ambient.py once per set, selected per pixel by sets_select of tests/area_sets_ref.c; the gather is that
 * file's sets_filter.  Build: gcc -O2 -fPIC -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.
 * Arrays are indexed by absolute pixel p of a W*H frame; a band is the pixels p0 .. p0 + n - 1.
 */
#include <stddef.h>

/* den = vis[2p + 1] != 0: each byte b becomes (b * num) / (S * den), num = vis[2p]; den = 0 leaves the pixel alone */
void ao_sets_shade(unsigned char *img, const unsigned *vis, int num_dirs, int p0, int n)
{
	int i, k;
	for (i = 0; i < n; i++) {
		size_t p = (size_t)p0 + i;
		unsigned num = vis[2 * p], den = vis[2 * p + 1], S = (unsigned)num_dirs;
		if (den == 0)
			continue;
		for (k = 0; k < 3; k++)
			img[p * 3 + k] = (unsigned char)(((unsigned)img[p * 3 + k] * num) / (S * den));
	}
}
