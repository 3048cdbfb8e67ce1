/*
 * lights_ref.c -- CPU restatement of the shading for several lights, the checker of
 * ugrt_shade_lights (tests/test_lights.py builds and loads it).
 *
 * Test infrastructure only.  Written from the specification, light by light and without the kernel's hoisting: every
 * light runs the whole Lambert term from the world-space point and normal.  Build: gcc -O2 -fPIC -ffp-contract=off
 * -fno-fast-math -fopenmp -I include, as the oracle.  Arrays are indexed by absolute pixel p = p0 + i of a W*H
 * frame; light l's flags lie at l * level.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

#define LT_MAX_LIGHTS 8

static void lt_normalize(float *a)
{
	float l = 1.0f / __builtin_sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
	a[0] *= l;
	a[1] *= l;
	a[2] *= l;
}

/* Rv = the 3x3 of cc[16..]: Rv^T v as the shading kernels apply it */
static void lt_to_view(const float *cc, const float *v, float *out)
{
	int k;
	for (k = 0; k < 3; k++)
		out[k] = cc[16 + k] * v[0] + cc[16 + 4 + k] * v[1] + cc[16 + 8 + k] * v[2];
}

/* the clamped Lambert colour of one light, accumulated from zero: ambient Kd/2, then Kd |L.N| */
static void lt_light_color(const float *cc, const float *light, const float *point, const float *normal, const float *kd,
			   float *c)
{
	float lv[3], pv[3], nv[3], ld[3], dot;
	int k;
	lt_to_view(cc, light, lv);
	lt_to_view(cc, point, pv);
	lt_to_view(cc, normal, nv);
	lt_normalize(nv);
	for (k = 0; k < 3; k++)
		ld[k] = pv[k] - lv[k];
	lt_normalize(ld);
	for (k = 0; k < 3; k++) {
		c[k] = 0.0f;
		c[k] += kd[k] * 0.5f;
	}
	dot = ld[0] * nv[0] + ld[1] * nv[1] + ld[2] * nv[2];
	if (dot > 0)
		dot *= 1;
	else
		dot *= -1;
	if (dot > 0)
		for (k = 0; k < 3; k++)
			c[k] += kd[k] * 1.0f * dot;
	for (k = 0; k < 3; k++)
		if (c[k] > 1.0f)
			c[k] = 1.0f;
}

/* returns 0, or 1 for num_lights outside 1..8 (nothing is written) */
int lt_shade_lights(const float *cc, unsigned char *img, const float *normal, const float *t_value, const float *dir,
		    int *ids, const float *cam_pos, const int *mat_idx, const float *mat_list, int mat_count,
		    int num_lights, const float *light_pos, const int *is_shadowed, long long level, int p0, int n)
{
	int i;
	if (num_lights < 1 || num_lights > LT_MAX_LIGHTS)
		return 1;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k, l;
		unsigned int sum[3] = { 0u, 0u, 0u };
		int id = ids[p];
		int idx = (id >= 0) ? mat_idx[id] : id;
		float t = t_value[p];
		ids[p] = idx;
		if (idx >= 0 && idx < mat_count && t > 0) {
			float point[3];
			const float *kd = &mat_list[idx * 6 + 3];
			for (k = 0; k < 3; k++)
				point[k] = cam_pos[k] + t * dir[p * 3 + k];
			for (l = 0; l < num_lights; l++) {
				float c[3];
				lt_light_color(cc, &light_pos[3 * l], point, &normal[p * 3], kd, c);
				for (k = 0; k < 3; k++) {
					unsigned char b = (unsigned char)(ugrt_f2u(c[k] * 255) & 0xFFu);
					if (is_shadowed && is_shadowed[(size_t)l * (size_t)level + (size_t)p] == 1)
						b = (unsigned char)(b / 3);
					sum[k] += b;
				}
			}
		}
		for (k = 0; k < 3; k++)
			img[p * 3 + k] = (unsigned char)(sum[k] / (unsigned int)num_lights);
	}
	return 0;
}
