/*
 * glossy_ref.c -- CPU restatement of the glossy reflections, the checker of ugrt_glossy_gather and
 * ugrt_glossy_apply (tests/test_glossy.py builds and loads it; the gather over the sums is ugrt_gi_filter, whose checker
 * is gi_filter of tests/indirect_ref.c).
 *
 * Test infrastructure only.  One loop per sample: the direction D_s is formed from the pixel's mirror direction, its
 * material's spread and the point of its set, turned back over the surface where it would enter it, walked to its closest
 * hit below `radius`, the hit is shaded and, with a shadow light, tested for an occluder towards it with a walk over ALL
 * cells of the specified set (no early exit) -- a different program from the kernel, which keeps S rays of a pixel in
 * neighbouring lanes, plans windows of cells and adds the bytes across lanes.  The walks and the shading are those of
 * tests/indirect_ref.c.  Per-sample outputs (hit_t, hit_id, occ, mirrored) let the tests compare each phase with the
 * checkers that exist: orc_trace_dda of oracle/ugrt_oracle.c and oc_trace_any of tests/occlusion_ref.c on the explicit
 * rays (glossy_expand).  Build: gcc -O2 -fPIC -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.  Arrays
 * are indexed by absolute pixel p of a W*H frame; a band is the pixels p0 .. p0 + n - 1; per-sample arrays lie at
 * s * N + p.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

typedef unsigned int u32;

#define GL_EPSILON 1e-21f
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

/* the tangent frame over the normal n and the world direction of the local one (x, y, z): a = the index of the smallest
 * |n[k]| (strict <: 1 against 0, then 2 against the winner), T = normalize(n x e_a), B = n x T, D = (x*T + y*B) + z*n */
static void gl_dir(const float *n, const float *loc, float *D)
{
	float a0 = __builtin_fabsf(n[0]), a1 = __builtin_fabsf(n[1]), a2 = __builtin_fabsf(n[2]);
	float best = a0, T[3], B[3];
	int a = 0, k;
	if (a1 < best) {
		a = 1;
		best = a1;
	}
	if (a2 < best)
		a = 2;
	if (a == 0) { /* n x (1,0,0) */
		T[0] = 0.0f;
		T[1] = n[2];
		T[2] = -n[1];
	} else if (a == 1) { /* n x (0,1,0) */
		T[0] = -n[2];
		T[1] = 0.0f;
		T[2] = n[0];
	} else { /* n x (0,0,1) */
		T[0] = n[1];
		T[1] = -n[0];
		T[2] = 0.0f;
	}
	NORMALIZE(T);
	CROSS(B, n, T);
	for (k = 0; k < 3; k++)
		D[k] = (loc[0] * T[k] + loc[1] * B[k]) + loc[2] * n[k];
}

/* Moller-Trumbore in the operation order of orc_mt_signed: 1 and *t when the ray hits with t_lo < t < t_hi */
static int gl_mt(const float *o, const float *d, const float *vertlist, const int *trilist, u32 f, float t_lo, float t_hi,
		 float *t_out)
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
	if (det > -GL_EPSILON && det < GL_EPSILON)
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
	if (!(t > t_lo && t < t_hi))
		return 0;
	*t_out = t;
	return 1;
}

static int gl_ucell(const float *g, const int *dims, int k, float p)
{
	int c = ugrt_floor2i((p - g[k]) * g[6 + k]);
	return c < 0 ? 0 : (c > dims[k] - 1 ? dims[k] - 1 : c);
}

/* the walk's start: the slab clip and the entry cell; 0: the ray misses the box */
static int gl_start(const float *g, const int *dims, const float *o, const float *d, float *tenter_out, int *c, int *step,
		    float *tmax, float *tdelta)
{
	float tenter = 0.0f, texit = 3.0e38f;
	int k;
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
		return 0;
	for (k = 0; k < 3; k++) {
		float pe = o[k] + tenter * d[k];
		c[k] = gl_ucell(g, dims, k, pe);
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
	*tenter_out = tenter;
	return 1;
}

/* The closest hit below radius: orc_trace_dda's walk with best_t started at min(3.0e38f, radius), entered only with
 * tenter < radius and ended behind a cell whose exit parameter is not below radius.  Returns the triangle or -2; *later:
 * 1 when the hit is not the first triangle the walk accepted (an any-hit walk would have answered with another). */
static int gl_closest(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
		      const float *vertlist, const int *trilist, const float *o, const float *d, float radius, float *t_out,
		      int *later)
{
	int c[3], step[3], k, best_id = -2, first_id = -2;
	float tmax[3], tdelta[3], tenter, best_t = radius < 3.0e38f ? radius : 3.0e38f;
	*later = 0;
	if (!gl_start(g, dims, o, d, &tenter, c, step, tmax, tdelta) || !(tenter < radius))
		return -2;
	for (k = dims[0] + dims[1] + dims[2] + 3; k > 0; k--) {
		u32 cell = (u32)((c[0] * dims[1] + c[1]) * dims[2] + c[2]);
		u32 sp = span[cell], off = offset[cell], r;
		int ax = (tmax[0] < tmax[1]) ? ((tmax[0] < tmax[2]) ? 0 : 2) : ((tmax[1] < tmax[2]) ? 1 : 2);
		float tnext = tmax[ax], t;
		for (r = 0; r < sp; r++) {
			u32 f = value_list[off + r];
			if (gl_mt(o, d, vertlist, trilist, f, 0.0f, best_t, &t)) {
				best_t = t;
				best_id = (int)f;
				if (first_id < 0)
					first_id = (int)f;
			}
		}
		if (best_id >= 0 && best_t <= tnext) {
			*t_out = best_t;
			*later = best_id != first_id;
			return best_id;
		}
		if (!(tnext < radius))
			break;
		c[ax] += step[ax];
		if (step[ax] == 0 || c[ax] < 0 || c[ax] >= dims[ax])
			break;
		tmax[ax] += tdelta[ax];
	}
	return -2;
}

/* the any-hit walk of oc_trace_any (tests/occlusion_ref.c) for one ray: every cell whose entry parameter is below t_max,
 * every triangle of it, no early exit */
static int gl_any(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
		  const float *vertlist, const int *trilist, const float *o, const float *d, float t_max)
{
	int c[3], step[3], k, occ = 0;
	float tmax[3], tdelta[3], tin, t;
	if (!gl_start(g, dims, o, d, &tin, c, step, tmax, tdelta))
		return 0;
	for (k = dims[0] + dims[1] + dims[2] + 3; k > 0 && tin < t_max; k--) {
		u32 cell = (u32)((c[0] * dims[1] + c[1]) * dims[2] + c[2]);
		u32 sp = span[cell], off = offset[cell], r;
		int ax = (tmax[0] < tmax[1]) ? ((tmax[0] < tmax[2]) ? 0 : 2) : ((tmax[1] < tmax[2]) ? 1 : 2);
		for (r = 0; r < sp; r++)
			occ |= gl_mt(o, d, vertlist, trilist, value_list[off + r], 0.0f, t_max, &t);
		tin = tmax[ax];
		c[ax] += step[ax];
		if (step[ax] == 0 || c[ax] < 0 || c[ax] >= dims[ax])
			break;
		tmax[ax] += tdelta[ax];
	}
	return occ;
}

/* orc_lambert without the drop-off */
static void gl_lambert(const float *cc, const float *light_position, const float *point, const float *normal, float *color,
		       const float *material)
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

static unsigned char gl_to_u8(float c)
{
	return (unsigned char)(ugrt_f2u(c * 255) & 0xFFu);
}

/* the spread of pixel p's lobe: d_spread[m] of the primary hit's material where that is > 0 (NaN, zeros and negative values
 * count as 0), at most 1; an id below 0 or a material out of range: 0 */
static float gl_spread(const int *ids, const int *mat_idx, const float *spread, int mat_count, int p)
{
	int id = ids[p], m;
	float a;
	if (id < 0)
		return 0.0f;
	m = mat_idx[id];
	if (m < 0 || m >= mat_count)
		return 0.0f;
	a = spread[m];
	if (!(a > 0.0f))
		return 0.0f;
	return a > 1.0f ? 1.0f : a;
}

static float gl_coord(float x)
{
	if (!(x == x))
		return 0.0f;
	return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
}

/* the direction of sample s of pixel p; returns 1 when the horizon rule mirrored it */
static int gl_lobe(const float *rays, const float *orays, float a, int S, int set_w, int set_h, const float *points, int width,
		   int p, int s, float *D)
{
	int y = p / width, x = p - y * width, k;
	const float *uv = &points[2 * (((y % set_h) * set_w + x % set_w) * S + s)];
	const float *R = &rays[p * 6 + 3], *n = &orays[p * 6 + 3];
	float len2 = (R[0] * R[0] + R[1] * R[1]) + R[2] * R[2];
	float inv = 1.0f / __builtin_sqrtf(len2);
	float r[3], loc[3], c;
	for (k = 0; k < 3; k++)
		r[k] = R[k] * inv;
	loc[0] = a * gl_coord(uv[0]);
	loc[1] = a * gl_coord(uv[1]);
	loc[2] = 1.0f;
	gl_dir(r, loc, D);
	c = (D[0] * n[0] + D[1] * n[1]) + D[2] * n[2];
	if (c < 0.0f) {
		for (k = 0; k < 3; k++)
			D[k] = D[k] - (2.0f * c) * n[k];
		return 1;
	}
	return 0;
}

/* the explicit rays of sample s: for an active pixel out = {o, D_s}; every other pixel of the band: six zeros */
void glossy_expand(const float *rays, const int *active, const float *orays, const int *ids, const int *mat_idx,
		   const float *spread, int mat_count, int S, int set_w, int set_h, const float *points, int width, int s, int p0,
		   int n, float *out)
{
	int i;
	for (i = 0; i < n; i++) {
		int p = p0 + i, k;
		for (k = 0; k < 6; k++)
			out[p * 6 + k] = 0.0f;
		if (!active[p])
			continue;
		for (k = 0; k < 3; k++)
			out[p * 6 + k] = rays[p * 6 + k];
		gl_lobe(rays, orays, gl_spread(ids, mat_idx, spread, mat_count, p), S, set_w, set_h, points, width, p, s,
			&out[p * 6 + 3]);
	}
}

/* ugrt_glossy_gather.  cc, light: the camera block and the shading light of the context; shadow_light: null = no shadow
 * phase.  Per-sample outputs (each may be null), at s * N + p: hit_t (-1 on a miss), hit_id (-2 on a miss), occ (the
 * shadow phase's bit for a hit, whatever its material; 0 on a miss or without a shadow light), mirrored (the horizon rule
 * turned the sample). */
void glossy_gather(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
		   const float *vertlist, const int *trilist, const float *rays, const int *active, const float *orays,
		   const int *ids, const int *mat_idx, const float *spread, int S, int set_w, int set_h, const float *points,
		   int width, float radius, const float *mat_list, int mat_count, const float *cc, const float *light,
		   const float *shadow_light, float eps, int p0, int n, long long N, u32 *sum, float *hit_t, int *hit_id,
		   int *occ_out, int *mirrored_out)
{
	int i;
#pragma omp parallel for schedule(dynamic, 64)
	for (i = 0; i < n; i++) {
		int p = p0 + i, s, k;
		u32 acc[3] = { 0u, 0u, 0u };
		float a;
		for (s = 0; s < S; s++) {
			size_t q = (size_t)s * (size_t)N + (size_t)p;
			if (hit_t)
				hit_t[q] = -1.0f;
			if (hit_id)
				hit_id[q] = -2;
			if (occ_out)
				occ_out[q] = 0;
			if (mirrored_out)
				mirrored_out[q] = 0;
		}
		for (k = 0; k < 4; k++)
			sum[4 * (size_t)p + k] = 0u;
		if (!active[p])
			continue;
		a = gl_spread(ids, mat_idx, spread, mat_count, p);
		for (s = 0; s < S; s++) {
			size_t q = (size_t)s * (size_t)N + (size_t)p;
			const float *o = &rays[p * 6];
			float D[3], t = -1.0f, L[3] = { 0.0f, 0.0f, 0.0f };
			int later = 0, id, hm, occ = 0;
			int mirrored = gl_lobe(rays, orays, a, S, set_w, set_h, points, width, p, s, D);
			if (mirrored_out)
				mirrored_out[q] = mirrored;
			id = gl_closest(g, dims, value_list, span, offset, vertlist, trilist, o, D, radius, &t, &later);
			if (id < 0)
				continue;
			if (shadow_light) { /* the occlusion ray of the hit, whatever its material (oc_occlusion_rays) */
				float e1[3], e2[3], nn[3], P[3], o2[3], d2[3], dn;
				for (k = 0; k < 3; k++) {
					float v0 = vertlist[3 * trilist[id * 3 + 0] + k];
					e1[k] = vertlist[3 * trilist[id * 3 + 1] + k] - v0;
					e2[k] = vertlist[3 * trilist[id * 3 + 2] + k] - v0;
					P[k] = o[k] + t * D[k];
				}
				CROSS(nn, e1, e2);
				NORMALIZE(nn);
				dn = DOT(D, nn);
				if (dn > 0) {
					nn[0] = -nn[0];
					nn[1] = -nn[1];
					nn[2] = -nn[2];
				}
				for (k = 0; k < 3; k++) {
					o2[k] = P[k] + eps * nn[k];
					d2[k] = shadow_light[k] - o2[k];
				}
				occ = gl_any(g, dims, value_list, span, offset, vertlist, trilist, o2, d2, 1.0f);
			}
			if (hit_t)
				hit_t[q] = t;
			if (hit_id)
				hit_id[q] = id;
			if (occ_out)
				occ_out[q] = occ;
			hm = mat_idx[id];
			if (hm < 0 || hm >= mat_count)
				continue;
			{ /* the level's colour (oc_level_color of tests/occlusion_ref.c) */
				float hp[3], e1[3], e2[3], nn[3], hmat[6];
				for (k = 0; k < 3; k++) {
					float v0 = vertlist[3 * trilist[id * 3 + 0] + k];
					e1[k] = vertlist[3 * trilist[id * 3 + 1] + k] - v0;
					e2[k] = vertlist[3 * trilist[id * 3 + 2] + k] - v0;
					hp[k] = o[k] + t * D[k];
					hmat[k] = mat_list[hm * 6 + 3 + k];
					hmat[3 + k] = mat_list[hm * 6 + 3 + k];
				}
				NORMALIZE(e1);
				NORMALIZE(e2);
				CROSS(nn, e1, e2);
				NORMALIZE(nn);
				gl_lambert(cc, light, hp, nn, L, hmat);
				for (k = 0; k < 3; k++)
					if (L[k] > 1.0f)
						L[k] = 1.0f;
			}
			if (occ)
				for (k = 0; k < 3; k++)
					L[k] = L[k] / 3.0f;
			for (k = 0; k < 3; k++)
				acc[k] += (u32)gl_to_u8(L[k]);
		}
		for (k = 0; k < 3; k++)
			sum[4 * (size_t)p + k] = acc[k];
		sum[4 * (size_t)p + 3] = 1u;
	}
}

/* ugrt_glossy_apply: ids are material indices (behind the shading call) */
void glossy_apply(unsigned char *img, const u32 *acc, int S, const int *ids, const float *reflect, int mat_count, int p0, int n)
{
	int i, c;
	for (i = 0; i < n; i++) {
		size_t p = (size_t)p0 + i;
		int m = ids[p];
		u32 den = acc[4 * p + 3];
		float k, over;
		if (den == 0u || m < 0 || m >= mat_count)
			continue;
		k = reflect[m];
		if (!(k > 0.0f))
			continue;
		if (k > 1.0f)
			k = 1.0f;
		over = (float)((u32)S * den);
		for (c = 0; c < 3; c++) {
			float mean = (float)acc[4 * p + c] / over;
			int v = ugrt_floor2i(((1.0f - k) * (float)img[p * 3 + c] + k * mean) + 0.5f);
			img[p * 3 + c] = (unsigned char)(v > 255 ? 255 : v);
		}
	}
}
