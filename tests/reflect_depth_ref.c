/*
 * reflect_depth_ref.c -- CPU restatement of reflections of depth D, the checker of
 * ugrt_reflect_rays_next and ugrt_shade_reflect_depth (tests/test_reflect_depth.py builds and loads it).
 *
 * Test infrastructure only.  It restates the oracle's orc_reflect_rays (with a per-ray origin), orc_lambert and
 * orc_to_u8 (oracle/ugrt_oracle.c) and the depth-D composition; the levels in between are traced with the oracle's
 * own orc_trace_dda.  Build: gcc -O2 -fPIC -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.
 * Arrays are indexed by absolute pixel p = p0 + i of a W*H frame; level j (1..D) of a stacked array lies at
 * (j-1) * level pixels.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

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

/* the reflected ray off triangle `id` hit at o + t*d: {P + eps*n, d - 2(d.n)n}, n = normalize(e1 x e2) against d */
static void rd_reflect(const float *o, const float *d, float t, int id, const float *vertlist, const int *trilist,
		       float eps, float *out)
{
	float e1[3], e2[3], nn[3], P[3], dn;
	int k;
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
		dn = -dn;
	}
	for (k = 0; k < 3; k++) {
		out[k] = P[k] + eps * nn[k];
		out[3 + k] = d[k] - (2.0f * dn) * nn[k];
	}
}

static int rd_goes_on(float t, int id, const int *mat_idx, const float *reflect, int mat_count)
{
	int m;
	if (!(t > 0) || id < 0)
		return 0;
	m = mat_idx[id];
	return m >= 0 && m < mat_count && reflect[m] > 0;
}

/* level 1: from the camera and the primary hits (orc_reflect_rays) */
void rd_reflect_rays(const float *cam, const float *t_list, const float *dir_list, const int *id_list,
		     const int *mat_idx, const float *reflect, int mat_count, const float *vertlist, const int *trilist,
		     float eps, int p0, int n, float *rays, int *active)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k;
		active[p] = 0;
		for (k = 0; k < 6; k++)
			rays[p * 6 + k] = 0.0f;
		if (!rd_goes_on(t_list[p], id_list[p], mat_idx, reflect, mat_count))
			continue;
		rd_reflect(cam, &dir_list[p * 3], t_list[p], id_list[p], vertlist, trilist, eps, &rays[p * 6]);
		active[p] = 1;
	}
}

/* level j -> j+1: from each ray's own origin */
void rd_reflect_rays_next(const float *rays, const int *active, const float *hit_t, const int *hit_id,
			  const int *mat_idx, const float *reflect, int mat_count, const float *vertlist,
			  const int *trilist, float eps, int p0, int n, float *rays_next, int *active_next)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k;
		active_next[p] = 0;
		for (k = 0; k < 6; k++)
			rays_next[p * 6 + k] = 0.0f;
		if (!active[p] || !rd_goes_on(hit_t[p], hit_id[p], mat_idx, reflect, mat_count))
			continue;
		rd_reflect(&rays[p * 6], &rays[p * 6 + 3], hit_t[p], hit_id[p], vertlist, trilist, eps, &rays_next[p * 6]);
		active_next[p] = 1;
	}
}

/* orc_lambert without the drop-off */
static void rd_lambert(const float *cc, const float *light_position, const float *point, const float *normal,
		       float *color, const float *material)
{
	float light_dir[3], lpv[3], pv[3], nv[3], dot_diffuse;
	const float light_ambient[3] = { 0.5f, 0.5f, 0.5f };
	const float light_diffuse[3] = { 1.0f, 1.0f, 1.0f };
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
		color[k] += material[k] * light_ambient[k];
	dot_diffuse = DOT(light_dir, nv);
	if (dot_diffuse > 0)
		dot_diffuse *= 1;
	else
		dot_diffuse *= -1;
	if (dot_diffuse > 0)
		for (k = 0; k < 3; k++)
			color[k] += material[3 + k] * light_diffuse[k] * dot_diffuse;
}

static unsigned char rd_to_u8(float c)
{
	return (unsigned char)(ugrt_f2u(c * 255) & 0xFFu);
}

/* clamped Lambert colour of a level's hit (0 on a miss or a material out of range); *kr = its reflect */
static void rd_level_color(const float *cc, const float *light, const int *mat_idx, const float *mat_list,
			   const float *reflect, int mat_count, const float *vertlist, const int *trilist,
			   const float *ray, float ht, int hid, float *rc, float *kr)
{
	float hp[3], e1[3], e2[3], nn[3], hmat[6];
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
		hmat[k] = mat_list[hm * 6 + 3 + k];
		hmat[3 + k] = mat_list[hm * 6 + 3 + k];
	}
	NORMALIZE(e1);
	NORMALIZE(e2);
	CROSS(nn, e1, e2);
	NORMALIZE(nn);
	rd_lambert(cc, light, hp, nn, rc, hmat);
	for (k = 0; k < 3; k++)
		if (rc[k] > 1.0f)
			rc[k] = 1.0f;
}

/* depth-D shading: acc = 0, w = 1; a level that goes on adds (w*(1-k))*L and sets w = w*k; the first that does not
 * (level D at the latest) adds w*L.  ids are rewritten to material indices as orc_shade_reflect does. */
void rd_shade_depth(const float *cc, const float *light, unsigned char *img, const float *normal, const float *t_value,
		    const float *dir, int *ids, const float *cam_pos, const int *mat_idx, const float *mat_list,
		    const float *reflect, int mat_count, const float *vertlist, const int *trilist, int depth,
		    long long level, const float *rays, const int *active, const float *hit_t, const int *hit_id, int p0,
		    int n)
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
				rd_lambert(cc, light, point, &normal[p * 3], color, material);
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
				rd_level_color(cc, light, mat_idx, mat_list, reflect, mat_count, vertlist, trilist,
					       &rays[q * 6], hit_t[q], hit_id[q], color, &kr);
			}
		}
		img[p * 3 + 0] = rd_to_u8(acc[0]);
		img[p * 3 + 1] = rd_to_u8(acc[1]);
		img[p * 3 + 2] = rd_to_u8(acc[2]);
	}
}
