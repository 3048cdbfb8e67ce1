/*
 * aa_ref.c -- CPU restatement of the adaptive anti-aliasing, the checker of ugrt_aa_edges,
 * ugrt_aa_gather and ugrt_aa_resolve (tests/test_antialias.py builds and loads it).
 *
 * Test infrastructure only.  One loop per sample: the eye ray through (col + sx, row + sy) is formed from the eye's node
 * table, walked to its closest hit cell by cell (no windows, no bitmap, no cooperative rounds), gated, shaded and, with a
 * shadow light, tested for an occluder with a walk over ALL cells towards the light (no early exit) -- a different
 * program from the kernel, which keeps the S rays of a pixel in neighbouring lanes and adds the bytes across lanes.
 * Per-sample outputs (hit_t, hit_id) let the tests compare the hit with the oracle's primary pass.  Build: gcc -O2 -fPIC
 * -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.  Arrays are indexed by absolute pixel p of a W*H
 * frame; a band is the pixels p0 .. p0 + n - 1; per-sample arrays lie at s * N + p.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

typedef unsigned int u32;

#define AA_EPSILON 1e-21f
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

/* ---- ugrt_aa_edges ---- */
static int aa_hit(const float *t, const int *ids, int x)
{
	return t[x] > 0 && ids[x] >= 0;
}

void aa_edges(const float *normal, const float *t, const float *dir, const int *ids, const float *cam, const int *mat_idx,
	      const int *shadowed, float normal_cos, float plane_tol, int W, int H, int p0, int n, int *edge)
{
	int i;
	for (i = 0; i < n; i++) {
		int p = p0 + i, y = p / W, x = p - y * W, dx, dy, k, e = 0;
		int hp = aa_hit(t, ids, p);
		for (dy = -1; dy <= 1; dy++) {
			for (dx = -1; dx <= 1; dx++) {
				int qx = x + dx, qy = y + dy, q, hq;
				if ((dx == 0 && dy == 0) || qx < 0 || qx >= W || qy < 0 || qy >= H)
					continue;
				q = qy * W + qx;
				hq = aa_hit(t, ids, q);
				if (hp != hq)
					e = 1;
				if (hp && hq && ids[p] != ids[q]) {
					float Pp[3], Pq[3], cosine, dist;
					const float *np = &normal[3 * p], *nq = &normal[3 * q];
					for (k = 0; k < 3; k++) {
						Pp[k] = cam[k] + t[p] * dir[3 * p + k];
						Pq[k] = cam[k] + t[q] * dir[3 * q + k];
					}
					cosine = (np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2];
					dist = (np[0] * (Pq[0] - Pp[0]) + np[1] * (Pq[1] - Pp[1])) + np[2] * (Pq[2] - Pp[2]);
					if (mat_idx[ids[p]] != mat_idx[ids[q]] || cosine < normal_cos || __builtin_fabsf(dist) > plane_tol)
						e = 1;
				}
				if (shadowed && shadowed[p] != shadowed[q])
					e = 1;
			}
		}
		edge[p] = e;
	}
}

/* ---- ugrt_aa_gather ---- */

/* the primary pass's direction (trace_kernel.cu:96-114 as the oracle states it) at the image position (fcol, frow) */
static void aa_dir(const float *eye, const float *tex, int W, int H, int strict, float fcol, float frow, float *d)
{
	float ftx = fcol / (float)W, fty = frow / (float)H, xs, ys, a, b, w00, w10, w01, w11;
	const float *n00, *n01;
	int i, j, k;
	ftx = 1 - ftx;
	xs = ftx * 4.0f;
	ys = fty * 4.0f;
	i = ugrt_f2i(xs);
	j = ugrt_f2i(ys);
	i = i > 3 ? 3 : i;
	j = j > 3 ? 3 : j;
	a = xs - (float)i;
	b = ys - (float)j;
	if (strict) {
		ugrt_tex_linear8(ftx * 0.8f + 0.1f, 5, &i, &a);
		ugrt_tex_linear8(fty * 0.8f + 0.1f, 5, &j, &b);
	}
	w00 = (1.0f - a) * (1.0f - b);
	w10 = a * (1.0f - b);
	w01 = (1.0f - a) * b;
	w11 = a * b;
	n00 = tex + (j * 5 + i) * 4;
	n01 = tex + ((j + 1) * 5 + i) * 4;
	for (k = 0; k < 3; k++) {
		float T = ((w00 * n00[k] + w10 * n00[4 + k]) + w01 * n01[k]) + w11 * n01[4 + k];
		d[k] = T - eye[k];
	}
	NORMALIZE(d);
}

/* aa_dir for n image positions, exported so that a test can aim triangles at the rays of chosen (pixel, offset) pairs
 * (tests/test_antialias_synthetic.py); d: [n][3].  The offset is the caller's: no clamp here. */
void aa_directions(const float *eye, const float *tex, int W, int H, int strict, int n, const float *fcol, const float *frow,
		   float *d)
{
	int i;
	for (i = 0; i < n; i++)
		aa_dir(eye, tex, W, H, strict, fcol[i], frow[i], d + 3 * (size_t)i);
}

/* Moller-Trumbore in the operation order of orc_mt_signed: 1 and *t when the ray hits with t_lo < t < t_hi */
static int aa_mt(const float *o, const float *d, const float *vertlist, const int *trilist, u32 f, float t_lo, float t_hi,
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
	if (det > -AA_EPSILON && det < AA_EPSILON)
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

static int aa_ucell(const float *g, const int *dims, int k, float p)
{
	int c = ugrt_floor2i((p - g[k]) * g[6 + k]);
	return c < 0 ? 0 : (c > dims[k] - 1 ? dims[k] - 1 : c);
}

/* the walk's start: the slab clip and the entry cell; 0: the ray misses the box */
static int aa_start(const float *g, const int *dims, const float *o, const float *d, float *tenter_out, int *c, int *step,
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
		c[k] = aa_ucell(g, dims, k, pe);
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

/* orc_trace_dda's walk for one ray: the triangle or -2 */
static int aa_closest(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
		      const float *vertlist, const int *trilist, const float *o, const float *d, float *t_out)
{
	int c[3], step[3], k, best_id = -2;
	float tmax[3], tdelta[3], tenter, best_t = 3.0e38f;
	if (!aa_start(g, dims, o, d, &tenter, c, step, tmax, tdelta))
		return -2;
	for (k = dims[0] + dims[1] + dims[2] + 3; k > 0; k--) {
		u32 cell = (u32)((c[0] * dims[1] + c[1]) * dims[2] + c[2]);
		u32 sp = span[cell], off = offset[cell], r;
		int ax = (tmax[0] < tmax[1]) ? ((tmax[0] < tmax[2]) ? 0 : 2) : ((tmax[1] < tmax[2]) ? 1 : 2);
		float tnext = tmax[ax], t;
		for (r = 0; r < sp; r++) {
			u32 f = value_list[off + r];
			if (aa_mt(o, d, vertlist, trilist, f, 0.0f, best_t, &t)) {
				best_t = t;
				best_id = (int)f;
			}
		}
		if (best_id >= 0 && best_t <= tnext) {
			*t_out = best_t;
			return best_id;
		}
		c[ax] += step[ax];
		if (step[ax] == 0 || c[ax] < 0 || c[ax] >= dims[ax])
			break;
		tmax[ax] += tdelta[ax];
	}
	return -2;
}

/* the any-hit walk of oc_trace_any (tests/occlusion_ref.c) for one ray: every cell whose entry parameter is below t_max,
 * every triangle of it, no early exit */
static int aa_any(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
		  const float *vertlist, const int *trilist, const float *o, const float *d, float t_max)
{
	int c[3], step[3], k, occ = 0;
	float tmax[3], tdelta[3], tin, t;
	if (!aa_start(g, dims, o, d, &tin, c, step, tmax, tdelta))
		return 0;
	for (k = dims[0] + dims[1] + dims[2] + 3; k > 0 && tin < t_max; k--) {
		u32 cell = (u32)((c[0] * dims[1] + c[1]) * dims[2] + c[2]);
		u32 sp = span[cell], off = offset[cell], r;
		int ax = (tmax[0] < tmax[1]) ? ((tmax[0] < tmax[2]) ? 0 : 2) : ((tmax[1] < tmax[2]) ? 1 : 2);
		for (r = 0; r < sp; r++)
			occ |= aa_mt(o, d, vertlist, trilist, value_list[off + r], 0.0f, t_max, &t);
		tin = tmax[ax];
		c[ax] += step[ax];
		if (step[ax] == 0 || c[ax] < 0 || c[ax] >= dims[ax])
			break;
		tmax[ax] += tdelta[ax];
	}
	return occ;
}

/* orc_lambert without the drop-off */
static void aa_lambert(const float *cc, const float *light_position, const float *point, const float *normal, float *color,
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

static unsigned char aa_to_u8(float c)
{
	return (unsigned char)(ugrt_f2u(c * 255) & 0xFFu);
}

/* ugrt_aa_gather.  eye_cc, tex: the eye's camera block and its 5x5x4 node table; cc, light: the context's current camera
 * block and shading light; shadow_light: null = no shadow phase.  Per-sample outputs (each may be null), at s * N + p:
 * hit_t (-1 on a miss or a hit the gate rejects), hit_id (-2 likewise). */
void aa_gather(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
	       const float *vertlist, const int *trilist, const float *eye_cc, const float *tex, int strict, int W, int H,
	       const int *edge, int S, int set_w, int set_h, const float *offsets, const int *mat_idx, const float *mat_list,
	       int mat_count, const float *cc, const float *light, const float *shadow_light, float eps, int p0, int n,
	       long long N, u32 *sum, float *hit_t, int *hit_id)
{
	int i;
#pragma omp parallel for schedule(dynamic, 64)
	for (i = 0; i < n; i++) {
		int p = p0 + i, s, k, y = p / W, x = p - y * W;
		u32 acc[3] = { 0u, 0u, 0u };
		for (s = 0; s < S; s++) {
			size_t q = (size_t)s * (size_t)N + (size_t)p;
			if (hit_t)
				hit_t[q] = -1.0f;
			if (hit_id)
				hit_id[q] = -2;
		}
		for (k = 0; k < 4; k++)
			sum[4 * (size_t)p + k] = 0u;
		if (!edge[p])
			continue;
		for (s = 0; s < S; s++) {
			size_t q = (size_t)s * (size_t)N + (size_t)p;
			const float *off = &offsets[2 * (((y % set_h) * set_w + x % set_w) * S + s)];
			const float *o = eye_cc;
			float D[3], t = -1.0f, P[3], hz, hw, e1[3], e2[3], nn[3], hmat[6], L[3] = { 0.0f, 0.0f, 0.0f };
			unsigned char b[3];
			int id, hm;
			float sx = off[0] > -0.5f ? off[0] : -0.5f, sy = off[1] > -0.5f ? off[1] : -0.5f; /* (clamped; a NaN: -0.5) */
			sx = sx < 0.5f ? sx : 0.5f;
			sy = sy < 0.5f ? sy : 0.5f;
			aa_dir(eye_cc, tex, W, H, strict, (float)x + sx, (float)y + sy, D);
			id = aa_closest(g, dims, value_list, span, offset, vertlist, trilist, o, D, &t);
			if (id < 0)
				continue;
			/* the primary epilogue's gate (trace_kernel.cu:56-82 isWithin) under the eye's MVP */
			for (k = 0; k < 3; k++)
				P[k] = o[k] + t * D[k];
			hz = eye_cc[48 + 2] * P[0] + eye_cc[48 + 4 + 2] * P[1] + eye_cc[48 + 8 + 2] * P[2] + eye_cc[48 + 12 + 2] * 1.0f;
			hw = eye_cc[48 + 3] * P[0] + eye_cc[48 + 4 + 3] * P[1] + eye_cc[48 + 8 + 3] * P[2] + eye_cc[48 + 12 + 3] * 1.0f;
			hz /= hw;
			if (ugrt_floor2i(hz * 1.0f) != 0)
				continue;
			if (hit_t)
				hit_t[q] = t;
			if (hit_id)
				hit_id[q] = id;
			hm = mat_idx[id];
			if (hm < 0 || hm >= mat_count)
				continue;
			for (k = 0; k < 3; k++) {
				float v0 = vertlist[3 * trilist[id * 3 + 0] + k];
				e1[k] = vertlist[3 * trilist[id * 3 + 1] + k] - v0;
				e2[k] = vertlist[3 * trilist[id * 3 + 2] + k] - v0;
				hmat[k] = mat_list[hm * 6 + 3 + k];
				hmat[3 + k] = mat_list[hm * 6 + 3 + k];
			}
			{ /* the shadow phase: the occlusion ray of the hit (oc_occlusion_rays), the light at t = 1 */
				int occ = 0;
				if (shadow_light) {
					float fn[3], o2[3], d2[3], dn;
					CROSS(fn, e1, e2);
					NORMALIZE(fn);
					dn = DOT(D, fn);
					if (dn > 0) {
						fn[0] = -fn[0];
						fn[1] = -fn[1];
						fn[2] = -fn[2];
					}
					for (k = 0; k < 3; k++) {
						o2[k] = P[k] + eps * fn[k];
						d2[k] = shadow_light[k] - o2[k];
					}
					occ = aa_any(g, dims, value_list, span, offset, vertlist, trilist, o2, d2, 1.0f);
				}
				/* the primary epilogue's normal and orc_shade's colour */
				NORMALIZE(e1);
				NORMALIZE(e2);
				CROSS(nn, e1, e2);
				NORMALIZE(nn);
				for (k = 0; k < 3; k++)
					nn[k] = nn[k] < 0 ? nn[k] * -1 : nn[k];
				aa_lambert(cc, light, P, nn, L, hmat);
				for (k = 0; k < 3; k++) {
					if (L[k] > 1.0f)
						L[k] = 1.0f;
					b[k] = aa_to_u8(L[k]);
					if (occ)
						b[k] /= 3;
					acc[k] += (u32)b[k];
				}
			}
		}
		for (k = 0; k < 3; k++)
			sum[4 * (size_t)p + k] = acc[k];
		sum[4 * (size_t)p + 3] = 1u;
	}
}

/* ugrt_aa_resolve */
void aa_resolve(unsigned char *img, const u32 *sum, int S, int p0, int n)
{
	int i, k;
	for (i = 0; i < n; i++) {
		size_t p = (size_t)p0 + i;
		if (sum[4 * p + 3] == 0u)
			continue;
		for (k = 0; k < 3; k++)
			img[p * 3 + k] = (unsigned char)((sum[4 * p + k] + (u32)S / 2u) / (u32)S);
	}
}
