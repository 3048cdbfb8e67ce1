/*
 * occlusion_ref.c -- CPU restatement of the shadows on reflected hits, the checker of
 * ugrt_occlusion_rays, ugrt_trace_dda_any and ugrt_shade_reflect_depth_occluded (tests/test_reflect_shadows.py builds
 * and loads it).
 *
 * Test infrastructure only.  oc_trace_any restates the walk of the oracle's orc_trace_dda (oracle/ugrt_oracle.c) and
 * visits ALL cells of the specified set with no early exit: a different program from the kernel, which stops at the
 * first occluder.  oc_brute_any tests every triangle.  Build: gcc -O2 -fPIC -ffp-contract=off -fno-fast-math -fopenmp
 * -I include, as the oracle.  Arrays are indexed by absolute pixel p = p0 + i of a W*H frame; level j (1..D) of a
 * stacked array lies at (j-1) * level pixels.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

typedef unsigned int u32;

#define OC_EPSILON 1e-21f
#define CROSS(dest, v1, v2)                          \
	do {                                         \
		dest[0] = v1[1] * v2[2] - v1[2] * v2[1]; \
		dest[1] = v1[2] * v2[0] - v1[0] * v2[2]; \
		dest[2] = v1[0] * v2[1] - v1[1] * v2[0]; \
	} while (0)
#define DOT(v1, v2) (v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2])
#define NORMALIZE(A)                                                                   \
	do {                                                                           \
		float l_ = 1.0f / __builtin_sqrtf(A[0] * A[0] + A[1] * A[1] + A[2] * A[2]); \
		A[0] *= l_;                                                            \
		A[1] *= l_;                                                            \
		A[2] *= l_;                                                            \
	} while (0)

/* for a pixel with active, hit_t > 0 and hit_id >= 0: o' = P + eps*n (P = o + t*d, n = normalize(e1 x e2) turned
 * against d), ray {o', L - o'}, oactive 1; every other pixel of the band: six zeros and 0 */
void oc_occlusion_rays(const float *rays, const int *active, const float *hit_t, const int *hit_id,
		       const float *vertlist, const int *trilist, const float *light, float eps, int p0, int n,
		       float *orays, int *oactive)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k, id = hit_id[p];
		float t = hit_t[p], e1[3], e2[3], nn[3], P[3], dn;
		const float *o = &rays[p * 6], *d = &rays[p * 6 + 3];
		oactive[p] = 0;
		for (k = 0; k < 6; k++)
			orays[p * 6 + k] = 0.0f;
		if (!active[p] || !(t > 0) || id < 0)
			continue;
		for (k = 0; k < 3; k++) {
			float v0 = vertlist[3 * trilist[id * 3 + 0] + k];
			e1[k] = vertlist[3 * trilist[id * 3 + 1] + k] - v0;
			e2[k] = vertlist[3 * trilist[id * 3 + 2] + k] - v0;
			P[k] = o[k] + t * d[k];
		}
		CROSS(nn, e1, e2);
		NORMALIZE(nn);
		dn = DOT(d, nn);
		if (dn > 0) {
			nn[0] = -nn[0];
			nn[1] = -nn[1];
			nn[2] = -nn[2];
		}
		for (k = 0; k < 3; k++) {
			orays[p * 6 + k] = P[k] + eps * nn[k];
			orays[p * 6 + 3 + k] = light[k] - orays[p * 6 + k];
		}
		oactive[p] = 1;
	}
}

/* Moller-Trumbore in the operation order of orc_mt_signed: 1 when the ray hits with 0 < t < t_max */
static int oc_hits(const float *o, const float *d, const float *vertlist, const int *trilist, u32 f, float t_max)
{
	const float *v0 = &vertlist[3 * trilist[f * 3 + 0]], *v1p = &vertlist[3 * trilist[f * 3 + 1]],
		    *v2p = &vertlist[3 * trilist[f * 3 + 2]];
	float tvec[3], e1[3], e2[3], pvec[3], qvec[3], det, inv_det, u, v, t;
	int k;
	for (k = 0; k < 3; k++) {
		e1[k] = v1p[k] - v0[k];
		e2[k] = v2p[k] - v0[k];
		tvec[k] = o[k] - v0[k];
	}
	CROSS(pvec, d, e2);
	det = DOT(e1, pvec);
	if (det > -OC_EPSILON && det < OC_EPSILON)
		return 0;
	inv_det = 1.0f / det;
	u = DOT(tvec, pvec) * inv_det;
	if (u < 0.0f || u > 1.0f)
		return 0;
	CROSS(qvec, tvec, e1);
	v = DOT(d, qvec) * inv_det;
	if (v < 0.0f || u + v > 1.0f)
		return 0;
	t = DOT(e2, qvec) * inv_det;
	return t > 0.0f && t < t_max;
}

static int oc_ucell(const float *g, const int *dims, int k, float p)
{
	int c = ugrt_floor2i((p - g[k]) * g[6 + k]);
	return c < 0 ? 0 : (c > dims[k] - 1 ? dims[k] - 1 : c);
}

/* The any-hit walk: orc_trace_dda's clip, entry cell, stepping and guard; a cell is visited while its entry parameter
 * (tenter, then the exit parameter of the cell before) is below t_max; occluded = OR over every triangle of every
 * visited cell.  g: lo[3], cell size[3], 1 / cell size[3].  Inactive pixels of the band get 0.
 * counters (may be null): [0] tests, [1] cells visited, [2] active rays. */
void oc_trace_any(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
		  const float *vertlist, const int *trilist, const float *rays, const int *active, float t_max, int p0,
		  int n, int *occluded, unsigned long long *counters)
{
	int i;
	unsigned long long tests = 0, cells = 0, nact = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : tests, cells, nact)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k, c[3], step[3], occ = 0;
		float o[3], d[3], tmax[3], tdelta[3], tenter = 0.0f, texit = 3.0e38f, tin;
		occluded[p] = 0;
		if (!active[p])
			continue;
		nact++;
		for (k = 0; k < 3; k++) {
			o[k] = rays[p * 6 + k];
			d[k] = rays[p * 6 + 3 + k];
		}
		for (k = 0; k < 3; k++) {
			float lo = g[k], hi = g[k] + g[3 + k] * (float)dims[k];
			if (d[k] != 0.0f) {
				float inv = 1.0f / d[k];
				float t0 = (lo - o[k]) * inv, t1 = (hi - o[k]) * inv;
				if (t0 > t1) {
					float s = t0;
					t0 = t1;
					t1 = s;
				}
				if (t0 > tenter)
					tenter = t0;
				if (t1 < texit)
					texit = t1;
			} else if (o[k] < lo || o[k] > hi) {
				texit = -1.0f;
			}
		}
		if (!(tenter <= texit))
			continue;
		for (k = 0; k < 3; k++) {
			float pe = o[k] + tenter * d[k];
			c[k] = oc_ucell(g, dims, k, pe);
			if (d[k] > 0.0f) {
				step[k] = 1;
				tmax[k] = ((g[k] + (float)(c[k] + 1) * g[3 + k]) - o[k]) / d[k];
				tdelta[k] = g[3 + k] / d[k];
			} else if (d[k] < 0.0f) {
				step[k] = -1;
				tmax[k] = ((g[k] + (float)c[k] * g[3 + k]) - o[k]) / d[k];
				tdelta[k] = -g[3 + k] / d[k];
			} else {
				step[k] = 0;
				tmax[k] = 3.0e38f;
				tdelta[k] = 3.0e38f;
			}
		}
		tin = tenter;
		for (k = dims[0] + dims[1] + dims[2] + 3; k > 0 && tin < t_max; k--) {
			u32 cell = (u32)((c[0] * dims[1] + c[1]) * dims[2] + c[2]);
			u32 sp = span[cell], off = offset[cell], r;
			int ax = (tmax[0] < tmax[1]) ? ((tmax[0] < tmax[2]) ? 0 : 2) : ((tmax[1] < tmax[2]) ? 1 : 2);
			cells++;
			for (r = 0; r < sp; r++) {
				tests++;
				occ |= oc_hits(o, d, vertlist, trilist, value_list[off + r], t_max);
			}
			tin = tmax[ax];
			c[ax] += step[ax];
			if (step[ax] == 0 || c[ax] < 0 || c[ax] >= dims[ax])
				break;
			tmax[ax] += tdelta[ax];
		}
		occluded[p] = occ;
	}
	if (counters) {
		counters[0] = tests;
		counters[1] = cells;
		counters[2] = nact;
	}
}

/* every triangle, 0 < t < t_max */
void oc_brute_any(const float *vertlist, const int *trilist, int F, const float *rays, const int *active, float t_max,
		  int p0, int n, int *occluded)
{
	int i;
#pragma omp parallel for schedule(dynamic, 64)
	for (i = 0; i < n; i++) {
		int p = p0 + i, f, occ = 0;
		occluded[p] = 0;
		if (!active[p])
			continue;
		for (f = 0; f < F && !occ; f++)
			occ = oc_hits(&rays[p * 6], &rays[p * 6 + 3], vertlist, trilist, (u32)f, t_max);
		occluded[p] = occ;
	}
}

/* orc_lambert without the drop-off */
static void oc_lambert(const float *cc, const float *light_position, const float *point, const float *normal,
		       float *color, const float *material)
{
	float light_dir[3], lpv[3], pv[3], nv[3], dot_diffuse;
	int k;
	for (k = 0; k < 3; k++) {
		lpv[k] = cc[16 + k] * light_position[0] + cc[16 + 4 + k] * light_position[1] + cc[16 + 8 + k] * light_position[2];
		pv[k] = cc[16 + k] * point[0] + cc[16 + 4 + k] * point[1] + cc[16 + 8 + k] * point[2];
		nv[k] = cc[16 + k] * normal[0] + cc[16 + 4 + k] * normal[1] + cc[16 + 8 + k] * normal[2];
	}
	NORMALIZE(nv);
	light_dir[0] = pv[0] - lpv[0];
	light_dir[1] = pv[1] - lpv[1];
	light_dir[2] = pv[2] - lpv[2];
	NORMALIZE(light_dir);
	for (k = 0; k < 3; k++)
		color[k] += material[k] * 0.5f;
	dot_diffuse = DOT(light_dir, nv);
	if (dot_diffuse > 0)
		dot_diffuse *= 1;
	else
		dot_diffuse *= -1;
	if (dot_diffuse > 0)
		for (k = 0; k < 3; k++)
			color[k] += material[3 + k] * 1.0f * dot_diffuse;
}

static unsigned char oc_to_u8(float c)
{
	return (unsigned char)(ugrt_f2u(c * 255) & 0xFFu);
}

/* clamped Lambert colour of a level's hit (0 on a miss or a material out of range), a third of it where the hit is
 * occluded; *kr = the hit material's reflect */
static void oc_level_color(const float *cc, const float *light, const int *mat_idx, const float *mat_list,
			   const float *reflect, int mat_count, const float *vertlist, const int *trilist,
			   const float *ray, float ht, int hid, int occ, float *rc, float *kr)
{
	float hp[3], e1[3], e2[3], nn[3], hmat[6];
	int k, hm;
	rc[0] = rc[1] = rc[2] = 0.0f;
	if (hid >= 0 && (hm = mat_idx[hid]) >= 0 && hm < mat_count) {
		*kr = reflect[hm];
		for (k = 0; k < 3; k++) {
			float v0 = vertlist[3 * trilist[hid * 3 + 0] + k];
			e1[k] = vertlist[3 * trilist[hid * 3 + 1] + k] - v0;
			e2[k] = vertlist[3 * trilist[hid * 3 + 2] + k] - v0;
			hp[k] = ray[k] + ht * ray[3 + k];
			hmat[k] = mat_list[hm * 6 + 3 + k];
			hmat[3 + k] = mat_list[hm * 6 + 3 + k];
		}
		NORMALIZE(e1);
		NORMALIZE(e2);
		CROSS(nn, e1, e2);
		NORMALIZE(nn);
		oc_lambert(cc, light, hp, nn, rc, hmat);
		for (k = 0; k < 3; k++)
			if (rc[k] > 1.0f)
				rc[k] = 1.0f;
	}
	if (occ == 1)
		for (k = 0; k < 3; k++)
			rc[k] = rc[k] / 3.0f;
}

/* the depth-D composition of DESIGN.md section 6.1 with the occluded levels darkened: acc = 0, w = 1; a level that
 * goes on adds (w*(1-k))*L and sets w = w*k; the first that does not (level D at the latest) adds w*L */
void oc_shade_depth_occluded(const float *cc, const float *light, unsigned char *img, const float *normal,
			     const float *t_value, const float *dir, int *ids, const float *cam_pos, const int *mat_idx,
			     const float *mat_list, const float *reflect, int mat_count, const float *vertlist,
			     const int *trilist, int depth, long long level, const float *rays, const int *active,
			     const float *hit_t, const int *hit_id, const int *occluded, int p0, int n)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k, j;
		float acc[3] = { 0.0f, 0.0f, 0.0f };
		int tri = ids[p];
		int idx = (tri >= 0) ? mat_idx[tri] : tri;
		ids[p] = idx;
		if (idx >= 0 && idx < mat_count) {
			float color[3] = { 0.0f, 0.0f, 0.0f }, material[6], w = 1.0f, kr = reflect[idx];
			for (k = 0; k < 3; k++) {
				material[k] = mat_list[idx * 6 + 3 + k];
				material[3 + k] = mat_list[idx * 6 + 3 + k];
			}
			if (t_value[p] > 0) {
				float point[3];
				for (k = 0; k < 3; k++)
					point[k] = cam_pos[k] + t_value[p] * dir[p * 3 + k];
				oc_lambert(cc, light, point, &normal[p * 3], color, material);
				for (k = 0; k < 3; k++)
					if (color[k] > 1.0f)
						color[k] = 1.0f;
			}
			for (j = 0;; j++) {
				size_t q = (size_t)j * (size_t)level + (size_t)p;
				if (j >= depth || !active[q]) {
					for (k = 0; k < 3; k++)
						acc[k] = acc[k] + w * color[k];
					break;
				}
				for (k = 0; k < 3; k++)
					acc[k] = acc[k] + (w * (1.0f - kr)) * color[k];
				w = w * kr;
				oc_level_color(cc, light, mat_idx, mat_list, reflect, mat_count, vertlist, trilist, &rays[q * 6],
					       hit_t[q], hit_id[q], occluded[q], color, &kr);
			}
		}
		img[p * 3 + 0] = oc_to_u8(acc[0]);
		img[p * 3 + 1] = oc_to_u8(acc[1]);
		img[p * 3 + 2] = oc_to_u8(acc[2]);
	}
}
