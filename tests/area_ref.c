/*
 * area_ref.c -- CPU restatement of the area light, the checker of ugrt_trace_dda_any_area,
 * ugrt_trace_dda_any_area_thru and ugrt_shade_area (tests/test_area_light.py builds and loads it).
 *
 * Test infrastructure only.  area_expand writes out, for ONE sample s, the explicit rays {o, pos_s - o} that the kernel
 * forms in registers; the expected mask is oc_trace_any of tests/occlusion_ref.c on those rays at t_max = 1, once per s,
 * OR-ed into bit s: the walk has no second restatement here (the see-through form: the same on a grid without the glass
 * triangles).  Build: gcc -O2 -fPIC -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.  Arrays are
 * indexed by absolute pixel p = p0 + i of a W*H frame.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

/* the explicit rays towards ONE point pos: for an active pixel rays = {o, pos - o}, o = floats 0..2 of its slot, the
 * subtraction per component in fp32; every other pixel of the band: six zeros */
void area_expand(const float *orays, const int *oactive, const float *pos, int p0, int n, float *rays)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k;
		for (k = 0; k < 6; k++)
			rays[p * 6 + k] = 0.0f;
		if (!oactive[p])
			continue;
		for (k = 0; k < 3; k++) {
			float o = orays[p * 6 + k];
			rays[p * 6 + k] = o;
			rays[p * 6 + 3 + k] = pos[k] - o;
		}
	}
}

/* lit = num_samples - popcount(mask & low num_samples bits); each byte b of the pixel becomes
 * (b * (num_samples + 2 * lit)) / (3 * num_samples) */
void area_shade(unsigned char *img, const unsigned *mask, int num_samples, int p0, int n)
{
	int i;
	for (i = 0; i < n; i++) {
		int p = p0 + i, s, k;
		unsigned dark = 0, lit, S = (unsigned)num_samples;
		for (s = 0; s < num_samples; s++)
			dark += (mask[p] >> s) & 1u;
		lit = S - dark;
		for (k = 0; k < 3; k++)
			img[p * 3 + k] = (unsigned char)(((unsigned)img[p * 3 + k] * (S + 2u * lit)) / (3u * S));
	}
}
