/*
 * fresnel_ref.c -- CPU restatement of the Fresnel glass, the checker of ugrt_fresnel_gather and
 * ugrt_fresnel_shade (tests/test_fresnel.py builds and loads it).
 *
 * Test infrastructure only.  A plain recursion over the rule: a node is shaded, its children are formed, each followed
 * child is walked to its closest hit and visited in turn, child 0 first; a node's term goes to the leaf that owns it, and
 * the leaves are added in the rule's fixed order at the end -- a different program from the kernel, which keeps the 2^D
 * leaves of a pixel in neighbouring lanes and walks a level at a time.  The walks (all cells, list order, no windows) and
 * the shading are those of tests/glossy_ref.c; the any-hit walk skips the faces whose material transmits.  Build: gcc -O2
 * -fPIC -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.  Arrays are indexed by absolute pixel p of a
 * W*H frame; a band is the pixels p0 .. p0 + n - 1; the per-level read-outs of path 0 lie at (j - 1) * N + p.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

typedef unsigned int u32;

#define FR_EPSILON 1e-21f
#define FR_MAX_DEPTH 6
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

/* ---- the rule's scalars, exported for the CPU tests ---- */

/* The share of a glass hit with cosine c = -u.n on the side the ray comes from: 0 and *F left alone past the critical
 * angle (k2 < 0), else 1 and *F = scale * (r0 + (1 - r0) * x^5), x = 1 - (front ? c : sqrt(k2)).  *k2_out gets k2. */
int fr_share(float c, float ior_m, int front, float scale, float *F, float *k2_out)
{
	float ior = ior_m > 0 ? ior_m : 1.0f;
	float eta = front ? 1.0f / ior : ior;
	float k2 = 1.0f - (eta * eta) * (1.0f - c * c);
	float q, r0, cs, x;
	if (k2_out)
		*k2_out = k2;
	if (k2 < 0)
		return 0;
	q = (1.0f - ior) / (1.0f + ior);
	r0 = q * q;
	cs = front ? c : __builtin_sqrtf(k2);
	x = 1.0f - cs;
	*F = scale * (r0 + (1.0f - r0) * (((x * x) * (x * x)) * x));
	return 1;
}

/* the children's weights of a split: (w*k)*(1 - F) and (w*k)*F */
void fr_split(float w, float k, float F, float *w0, float *w1)
{
	float wk = w * k;
	*w0 = wk * (1.0f - F);
	*w1 = wk * F;
}

/* ---- the walks and the shading of tests/glossy_ref.c ---- */

static int fr_mt(const float *o, const float *d, const float *vertlist, const int *trilist, u32 f, float t_lo, float t_hi,
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
	if (det > -FR_EPSILON && det < FR_EPSILON)
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

static int fr_ucell(const float *g, const int *dims, int k, float p)
{
	int c = ugrt_floor2i((p - g[k]) * g[6 + k]);
	return c < 0 ? 0 : (c > dims[k] - 1 ? dims[k] - 1 : c);
}

static int fr_start(const float *g, const int *dims, const float *o, const float *d, float *tenter_out, int *c, int *step,
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
		c[k] = fr_ucell(g, dims, k, pe);
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

struct fr_scene {
	const float *g;
	const int *dims;
	const u32 *value_list, *span, *offset;
	const float *vertlist;
	const int *trilist;
	const int *mat_idx;
	const float *mat_list, *reflect, *transmit, *ior;
	int mat_count, depth;
	float scale, min_weight, eps;
	const float *cc, *light, *shadow_light;
};

/* orc_trace_dda's walk: the closest hit, or -2 */
static int fr_closest(const struct fr_scene *S, const float *o, const float *d, float *t_out)
{
	const int *dims = S->dims;
	int c[3], step[3], k, best_id = -2;
	float tmax[3], tdelta[3], tenter, best_t = 3.0e38f;
	if (!fr_start(S->g, dims, o, d, &tenter, c, step, tmax, tdelta))
		return -2;
	for (k = dims[0] + dims[1] + dims[2] + 3; k > 0; k--) {
		u32 cell = (u32)((c[0] * dims[1] + c[1]) * dims[2] + c[2]);
		u32 sp = S->span[cell], off = S->offset[cell], r;
		int ax = (tmax[0] < tmax[1]) ? ((tmax[0] < tmax[2]) ? 0 : 2) : ((tmax[1] < tmax[2]) ? 1 : 2);
		float tnext = tmax[ax], t;
		for (r = 0; r < sp; r++) {
			u32 f = S->value_list[off + r];
			if (fr_mt(o, d, S->vertlist, S->trilist, f, 0.0f, best_t, &t)) {
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

/* oc_trace_any's walk for one ray, the faces whose material transmits taken out: every cell whose entry parameter is
 * below t_max, every triangle of it, no early exit */
static int fr_any_thru(const struct fr_scene *S, const float *o, const float *d, float t_max)
{
	const int *dims = S->dims;
	int c[3], step[3], k, occ = 0;
	float tmax[3], tdelta[3], tin, t;
	if (!fr_start(S->g, dims, o, d, &tin, c, step, tmax, tdelta))
		return 0;
	for (k = dims[0] + dims[1] + dims[2] + 3; k > 0 && tin < t_max; k--) {
		u32 cell = (u32)((c[0] * dims[1] + c[1]) * dims[2] + c[2]);
		u32 sp = S->span[cell], off = S->offset[cell], r;
		int ax = (tmax[0] < tmax[1]) ? ((tmax[0] < tmax[2]) ? 0 : 2) : ((tmax[1] < tmax[2]) ? 1 : 2);
		for (r = 0; r < sp; r++) {
			u32 f = S->value_list[off + r];
			int m = S->mat_idx[f];
			if (m >= 0 && m < S->mat_count && S->transmit[m] > 0)
				continue;
			occ |= fr_mt(o, d, S->vertlist, S->trilist, f, 0.0f, t_max, &t);
		}
		tin = tmax[ax];
		c[ax] += step[ax];
		if (step[ax] == 0 || c[ax] < 0 || c[ax] >= dims[ax])
			break;
		tmax[ax] += tdelta[ax];
	}
	return occ;
}

/* orc_lambert without the drop-off */
static void fr_lambert(const float *cc, const float *light_position, const float *point, const float *normal, float *color,
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

static unsigned char fr_to_u8(float c)
{
	return (unsigned char)(ugrt_f2u(c * 255) & 0xFFu);
}

/* ---- the tree ---- */

/* what one pixel's recursion writes */
struct fr_pixel {
	float leaf[1 << FR_MAX_DEPTH][3];
	long long nodes; /* walked */
	float share;     /* the root's k*F (0 without a split) */
	/* path 0, level j at [j - 1] */
	float ray[FR_MAX_DEPTH][6], t[FR_MAX_DEPTH];
	int id[FR_MAX_DEPTH], active[FR_MAX_DEPTH];
};

/* The node of level j and prefix `pre` (bits 0 .. j-1): ray {o, d}, weight w, hit (t, id); nrm: the root's stored normal,
 * null for a level; first: the root's child 0 as the caller gave it, null for a level. */
static void fr_node(const struct fr_scene *S, struct fr_pixel *px, int j, u32 pre, const float *o, const float *d, float w,
		    float t, int id, const float *nrm, const float *first)
{
	float L[3] = { 0.0f, 0.0f, 0.0f }, kw = 0.0f, w0 = 0.0f, w1 = 0.0f, c0[6], c1[6];
	int m = -1, f0 = 0, f1 = 0, k;
	if (id >= 0) {
		m = S->mat_idx[id];
		if (m < 0 || m >= S->mat_count)
			m = -1;
	}
	if (m >= 0) {
		float e1[3], e2[3], nn[3], P[3], dn, hmat[6];
		int front, two = 0;
		for (k = 0; k < 3; k++) {
			float v0 = S->vertlist[3 * S->trilist[id * 3 + 0] + k];
			e1[k] = S->vertlist[3 * S->trilist[id * 3 + 1] + k] - v0;
			e2[k] = S->vertlist[3 * S->trilist[id * 3 + 2] + k] - v0;
			P[k] = o[k] + t * d[k];
			hmat[k] = S->mat_list[m * 6 + 3 + k];
			hmat[3 + k] = S->mat_list[m * 6 + 3 + k];
		}
		/* the hit frame: the normal turned against the ray */
		CROSS(nn, e1, e2);
		NORMALIZE(nn);
		dn = DOT(d, nn);
		front = !(dn > 0);
		if (!front) {
			nn[0] = -nn[0];
			nn[1] = -nn[1];
			nn[2] = -nn[2];
			dn = -dn;
		}
		{
			float kt = S->transmit[m], kr = S->reflect[m], wk;
			kw = kt > 0 ? kt : kr;
			wk = w * kw;
			if (j < S->depth) {
				/* the mirrored ray: a mirror's child, a glass hit's child 1, and its child 0 past the critical angle */
				float mir[6];
				for (k = 0; k < 3; k++) {
					mir[k] = P[k] + S->eps * nn[k];
					mir[3 + k] = d[k] - (2.0f * dn) * nn[k];
				}
				if (kt > 0) {
					float u[3] = { d[0], d[1], d[2] }, c, F = 0.0f, k2;
					NORMALIZE(u);
					c = -DOT(u, nn);
					two = fr_share(c, S->ior[m], front, S->scale, &F, &k2);
					if (two) {
						float ior = S->ior[m] > 0 ? S->ior[m] : 1.0f;
						float eta = front ? 1.0f / ior : ior;
						float gg = eta * c - __builtin_sqrtf(k2);
						for (k = 0; k < 3; k++) {
							c0[k] = P[k] - S->eps * nn[k];
							c0[3 + k] = eta * u[k] + gg * nn[k];
							c1[k] = mir[k];
							c1[3 + k] = mir[3 + k];
						}
						fr_split(w, kw, F, &w0, &w1);
						if (j == 0)
							px->share = kw * F;
					} else {
						for (k = 0; k < 6; k++)
							c0[k] = mir[k];
						w0 = wk;
					}
				} else if (kr > 0) {
					for (k = 0; k < 6; k++)
						c0[k] = mir[k];
					w0 = wk;
				}
				if (first)
					for (k = 0; k < 6; k++)
						c0[k] = first[k];
				f0 = w0 > S->min_weight;
				f1 = two && w1 > S->min_weight;
			}
		}
		/* the colour */
		if (nrm) {
			if (t > 0) {
				fr_lambert(S->cc, S->light, P, nrm, L, hmat);
				for (k = 0; k < 3; k++)
					if (L[k] > 1.0f)
						L[k] = 1.0f;
			}
		} else {
			float hn[3];
			NORMALIZE(e1);
			NORMALIZE(e2);
			CROSS(hn, e1, e2);
			NORMALIZE(hn);
			fr_lambert(S->cc, S->light, P, hn, L, hmat);
			for (k = 0; k < 3; k++)
				if (L[k] > 1.0f)
					L[k] = 1.0f;
			if (S->shadow_light) {
				float o2[3], d2[3];
				for (k = 0; k < 3; k++) {
					o2[k] = P[k] + S->eps * nn[k];
					d2[k] = S->shadow_light[k] - o2[k];
				}
				if (fr_any_thru(S, o2, d2, 1.0f))
					for (k = 0; k < 3; k++)
						L[k] = L[k] / 3.0f;
			}
		}
	}
	if (f0 || f1) {
		for (k = 0; k < 3; k++)
			px->leaf[pre][k] = px->leaf[pre][k] + (w * (1.0f - kw)) * L[k];
	} else {
		for (k = 0; k < 3; k++)
			px->leaf[pre][k] = px->leaf[pre][k] + w * L[k];
		return;
	}
	if (f0) {
		float ct = -1.0f;
		int cid = fr_closest(S, c0, &c0[3], &ct);
		px->nodes++;
		if (pre == 0u) {
			for (k = 0; k < 6; k++)
				px->ray[j][k] = c0[k];
			px->t[j] = cid >= 0 ? ct : -1.0f;
			px->id[j] = cid;
			px->active[j] = 1;
		}
		fr_node(S, px, j + 1, pre, c0, &c0[3], w0, ct, cid, NULL, NULL);
	}
	if (f1) {
		float ct = -1.0f;
		int cid = fr_closest(S, c1, &c1[3], &ct);
		px->nodes++;
		fr_node(S, px, j + 1, pre | (1u << j), c1, &c1[3], w1, ct, cid, NULL, NULL);
	}
}

/* ugrt_fresnel_gather.  cc, light: the camera block and the shading light of the context; shadow_light: null = no shadow
 * phase.  acc [4N] float.  Read-outs (each may be null): nodes_out [1] the nodes walked; share [N] the root's k*F;
 * p_rays [depth][6N], p_active / p_id [depth][N] ints, p_t [depth][N]: path 0's level rays and hits (zeros / 0 / -1 / -2
 * where path 0 does not reach the level). */
void fresnel_gather(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
		    const float *vertlist, const int *trilist, const float *rays, const int *active, const float *normal,
		    const float *t_value, const float *ray_dir, const int *ids, const float *cam_pos, const int *mat_idx,
		    const float *mat_list, const float *reflect, const float *transmit, const float *ior, int mat_count, int depth,
		    float scale, float min_weight, const float *cc, const float *light, const float *shadow_light, float eps, int p0,
		    int n, long long N, float *acc, long long *nodes_out, float *share, float *p_rays, int *p_active, float *p_t,
		    int *p_id)
{
	struct fr_scene S = { g,        dims,    value_list, span,      offset, vertlist, trilist,    mat_idx, mat_list,
			      reflect,  transmit, ior,       mat_count, depth,  scale,    min_weight, eps,     cc,
			      light,    shadow_light };
	long long total = 0;
	int i;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : total)
	for (i = 0; i < n; i++) {
		int p = p0 + i, j, k;
		u32 b;
		struct fr_pixel px;
		for (k = 0; k < 4; k++)
			acc[4 * (size_t)p + k] = 0.0f;
		if (share)
			share[p] = 0.0f;
		for (j = 0; j < depth; j++) {
			size_t q = (size_t)j * (size_t)N + (size_t)p;
			if (p_rays)
				for (k = 0; k < 6; k++)
					p_rays[q * 6 + k] = 0.0f;
			if (p_active)
				p_active[q] = 0;
			if (p_t)
				p_t[q] = -1.0f;
			if (p_id)
				p_id[q] = -2;
		}
		if (!active[p])
			continue;
		for (b = 0; b < (1u << depth); b++)
			px.leaf[b][0] = px.leaf[b][1] = px.leaf[b][2] = 0.0f;
		px.nodes = 0;
		px.share = 0.0f;
		for (j = 0; j < FR_MAX_DEPTH; j++)
			px.active[j] = 0;
		fr_node(&S, &px, 0, 0u, cam_pos, &ray_dir[p * 3], 1.0f, t_value[p], ids[p], &normal[p * 3], &rays[p * 6]);
		/* the leaves' sum: pairwise from the deepest bit up */
		for (j = depth - 1; j >= 0; j--)
			for (b = 0; b < (1u << j); b++)
				for (k = 0; k < 3; k++)
					px.leaf[b][k] = px.leaf[b][k] + px.leaf[b + (1u << j)][k];
		for (k = 0; k < 3; k++)
			acc[4 * (size_t)p + k] = px.leaf[0][k];
		acc[4 * (size_t)p + 3] = 1.0f;
		total += px.nodes;
		if (share)
			share[p] = px.share;
		for (j = 0; j < depth; j++) {
			size_t q = (size_t)j * (size_t)N + (size_t)p;
			if (!px.active[j])
				continue;
			if (p_rays)
				for (k = 0; k < 6; k++)
					p_rays[q * 6 + k] = px.ray[j][k];
			if (p_active)
				p_active[q] = 1;
			if (p_t)
				p_t[q] = px.t[j];
			if (p_id)
				p_id[q] = px.id[j];
		}
	}
	if (nodes_out)
		*nodes_out = total;
}

/* ugrt_fresnel_shade: ids are triangle ids on entry and material indices on return */
void fresnel_shade(const float *cc, const float *light, unsigned char *img, const float *normal, const float *t_value,
		   const float *ray_dir, int *ids, const float *cam_pos, const int *mat_idx, const float *mat_list, int mat_count,
		   const float *acc, int p0, int n)
{
	int i;
	for (i = 0; i < n; i++) {
		size_t p = (size_t)p0 + i;
		float a[3] = { 0.0f, 0.0f, 0.0f };
		int tri = ids[p], idx = tri >= 0 ? mat_idx[tri] : tri, k;
		ids[p] = idx;
		if (acc[4 * p + 3] != 0.0f) {
			for (k = 0; k < 3; k++)
				a[k] = acc[4 * p + k];
		} else if (idx >= 0 && idx < mat_count) {
			float color[3] = { 0.0f, 0.0f, 0.0f }, material[6], point[3], t = t_value[p];
			for (k = 0; k < 3; k++) {
				material[k] = mat_list[idx * 6 + 3 + k];
				material[3 + k] = mat_list[idx * 6 + 3 + k];
			}
			if (t > 0) {
				for (k = 0; k < 3; k++)
					point[k] = cam_pos[k] + t * ray_dir[p * 3 + k];
				fr_lambert(cc, light, point, &normal[p * 3], color, material);
				for (k = 0; k < 3; k++)
					if (color[k] > 1.0f)
						color[k] = 1.0f;
			}
			for (k = 0; k < 3; k++)
				a[k] = a[k] + 1.0f * color[k];
		}
		for (k = 0; k < 3; k++)
			img[p * 3 + k] = fr_to_u8(a[k]);
	}
}
