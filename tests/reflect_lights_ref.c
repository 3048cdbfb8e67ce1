/*
 * reflect_lights_ref.c -- CPU restatement of the reflection shading under several lights, the
 * checker of ugrt_shade_reflect_lights (tests/test_reflect_lights.py builds and loads it).
 *
 * Test infrastructure only.  Written from the specification, light by light and with nothing hoisted: every light
 * walks the pixel's whole level chain again and runs the whole Lambert term from the world-space point and normal of
 * every level.  The any-hit side has no restatement of its own: the expected flags are oc_occlusion_rays +
 * oc_trace_any of tests/occlusion_ref.c, once per light.  Build: gcc -O2 -fPIC -ffp-contract=off -fno-fast-math
 * -fopenmp -I include, as the oracle.  Arrays are indexed by absolute pixel p = p0 + i of a W*H frame; level j (1..D)
 * of a stacked array lies at (j-1) * level pixels, light l's shadow flags at l * level, the occlusion flag of level j
 * and light l at ((j-1) * L + l) * level.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

#define RL_MAX_LIGHTS 8
#define RL_MAX_DEPTH 8

static void rl_normalize(float *a)
{
	float l = 1.0f / __builtin_sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
	a[0] *= l;
	a[1] *= l;
	a[2] *= l;
}

/* Rv = the 3x3 of cc[16..]: Rv^T v as the shading kernels apply it */
static void rl_to_view(const float *cc, const float *v, float *out)
{
	int k;
	for (k = 0; k < 3; k++)
		out[k] = cc[16 + k] * v[0] + cc[16 + 4 + k] * v[1] + cc[16 + 8 + k] * v[2];
}

/* the clamped Lambert colour under one light, accumulated from zero: ambient Kd/2, then Kd |L.N| */
static void rl_light_color(const float *cc, const float *light, const float *point, const float *normal, const float *kd,
			   float *c)
{
	float lv[3], pv[3], nv[3], ld[3], dot;
	int k;
	rl_to_view(cc, light, lv);
	rl_to_view(cc, point, pv);
	rl_to_view(cc, normal, nv);
	rl_normalize(nv);
	for (k = 0; k < 3; k++)
		ld[k] = pv[k] - lv[k];
	rl_normalize(ld);
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

/* colour of level j >= 1's hit under one light (0 on a miss or a material out of range), a third of it where the hit
 * is occluded from that light; *kr = the hit material's reflect where it is in range */
static void rl_level_color(const float *cc, const float *light, const int *mat_idx, const float *mat_list,
			   const float *reflect, int mat_count, const float *vertlist, const int *trilist, const float *ray,
			   float ht, int hid, int occ, float *rc, float *kr)
{
	float hp[3], e1[3], e2[3], nn[3];
	int k, hm;
	rc[0] = rc[1] = rc[2] = 0.0f;
	if (hid < 0)
		return;
	hm = mat_idx[hid];
	if (hm < 0 || hm >= mat_count)
		return;
	*kr = reflect[hm];
	for (k = 0; k < 3; k++) {
		float v0 = vertlist[3 * trilist[hid * 3 + 0] + k];
		e1[k] = vertlist[3 * trilist[hid * 3 + 1] + k] - v0;
		e2[k] = vertlist[3 * trilist[hid * 3 + 2] + k] - v0;
		hp[k] = ray[k] + ht * ray[3 + k];
	}
	rl_normalize(e1);
	rl_normalize(e2);
	nn[0] = e1[1] * e2[2] - e1[2] * e2[1];
	nn[1] = e1[2] * e2[0] - e1[0] * e2[2];
	nn[2] = e1[0] * e2[1] - e1[1] * e2[0];
	rl_normalize(nn);
	rl_light_color(cc, light, hp, nn, &mat_list[hm * 6 + 3], rc);
	if (occ == 1)
		for (k = 0; k < 3; k++)
			rc[k] = rc[k] / 3.0f;
}

/* returns 0, or 1 for num_lights / depth outside 1..8 (nothing is written).  is_shadowed and occluded may be null. */
int rl_shade(const float *cc, unsigned char *img, const float *normal, const float *t_value, const float *dir, int *ids,
	     const float *cam_pos, const int *mat_idx, const float *mat_list, const float *reflect, int mat_count,
	     const float *vertlist, const int *trilist, int depth, long long level, const float *rays, const int *active,
	     const float *hit_t, const int *hit_id, int num_lights, const float *light_pos, const int *is_shadowed,
	     const int *occluded, int p0, int n)
{
	int i;
	if (num_lights < 1 || num_lights > RL_MAX_LIGHTS || depth < 1 || depth > RL_MAX_DEPTH)
		return 1;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k, j, l;
		unsigned int sum[3] = { 0u, 0u, 0u };
		int tri = ids[p];
		int idx = (tri >= 0) ? mat_idx[tri] : tri;
		ids[p] = idx;
		if (idx >= 0 && idx < mat_count) {
			for (l = 0; l < num_lights; l++) {
				const float *light = &light_pos[3 * l];
				float acc[3] = { 0.0f, 0.0f, 0.0f }, color[3] = { 0.0f, 0.0f, 0.0f }, w = 1.0f, kr = reflect[idx];
				if (t_value[p] > 0) {
					float point[3];
					for (k = 0; k < 3; k++)
						point[k] = cam_pos[k] + t_value[p] * dir[p * 3 + k];
					rl_light_color(cc, light, point, &normal[p * 3], &mat_list[idx * 6 + 3], color);
				}
				for (j = 0;; j++) {
					size_t q = (size_t)j * (size_t)level + (size_t)p;
					int occ = 0;
					if (j >= depth || !active[q]) {
						for (k = 0; k < 3; k++)
							acc[k] = acc[k] + w * color[k];
						break;
					}
					for (k = 0; k < 3; k++)
						acc[k] = acc[k] + (w * (1.0f - kr)) * color[k];
					w = w * kr;
					if (occluded)
						occ = occluded[((size_t)j * (size_t)num_lights + (size_t)l) * (size_t)level + (size_t)p];
					rl_level_color(cc, light, mat_idx, mat_list, reflect, mat_count, vertlist, trilist, &rays[q * 6],
						       hit_t[q], hit_id[q], occ, color, &kr);
				}
				for (k = 0; k < 3; k++) {
					unsigned char b = (unsigned char)(ugrt_f2u(acc[k] * 255) & 0xFFu);
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
