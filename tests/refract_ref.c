/*
 * refract_ref.c -- CPU restatement of the refracted ray, the checker of ugrt_refract_rays and
 * ugrt_refract_rays_next (tests/test_refract.py builds and loads it).
 *
 * Test infrastructure only.  It writes the formula of section 6.6 out: the hit frame, Snell's law with the relative
 * index taken from the side the ray comes from, total internal reflection, and the choice between the transmitted and
 * the mirrored ray per material.  The levels' nearest hits are traced with the oracle's own orc_trace_dda and the images
 * come from the existing shading restatements with the `continue` list in the place of `reflect`; the see-through
 * any-hit walk is oc_trace_any on a grid whose lists were filtered in numpy.  Build: gcc -O2 -fPIC -ffp-contract=off
 * -fno-fast-math -fopenmp -I include, as the oracle.  Arrays are indexed by absolute pixel p = p0 + i of a W*H frame.
 */
#include <math.h>
#include <stddef.h>

#include "ugrt_fmath.h"

/* kind of the ray written for a pixel (rf_*'s `kind` output; 0: none) */
#define RF_MIRROR 1 /* the material only reflects */
#define RF_FRONT 2  /* refracted into the solid: the winding's normal faced the ray */
#define RF_BACK 3   /* refracted out of the solid */
#define RF_TOTAL 4  /* glass, past the critical angle: mirrored */

static float rf_dot(const float *a, const float *b)
{
	return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

static void rf_scale_to_unit(float *a)
{
	float l = 1.0f / sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
	a[0] *= l;
	a[1] *= l;
	a[2] *= l;
}

/* the ray that leaves triangle `id`, hit at o + t*d, for a material (transmit_m, reflect_m, ior_m); returns its kind */
static int rf_ray(const float *o, const float *d, float t, int id, const float *vertlist, const int *trilist, float eps,
		  float transmit_m, float reflect_m, float ior_m, float *out)
{
	float a[3], b[3], n[3], P[3], u[3], dn, c, ior, eta, k, g;
	int q, front;
	if (!(transmit_m > 0) && !(reflect_m > 0))
		return 0;
	for (q = 0; q < 3; q++) {
		float v0 = vertlist[3 * trilist[id * 3 + 0] + q];
		a[q] = vertlist[3 * trilist[id * 3 + 1] + q] - v0;
		b[q] = vertlist[3 * trilist[id * 3 + 2] + q] - v0;
		P[q] = o[q] + t * d[q];
	}
	n[0] = a[1] * b[2] - a[2] * b[1];
	n[1] = a[2] * b[0] - a[0] * b[2];
	n[2] = a[0] * b[1] - a[1] * b[0];
	rf_scale_to_unit(n);
	dn = rf_dot(d, n);
	front = !(dn > 0);
	if (!front) {
		n[0] = -n[0];
		n[1] = -n[1];
		n[2] = -n[2];
		dn = -dn;
	}
	if (transmit_m > 0) {
		u[0] = d[0];
		u[1] = d[1];
		u[2] = d[2];
		rf_scale_to_unit(u);
		c = -rf_dot(u, n);
		ior = ior_m > 0 ? ior_m : 1.0f;
		eta = front ? 1.0f / ior : ior;
		k = 1.0f - (eta * eta) * (1.0f - c * c);
		if (!(k < 0)) {
			g = eta * c - sqrtf(k);
			for (q = 0; q < 3; q++) {
				out[q] = P[q] - eps * n[q];
				out[3 + q] = eta * u[q] + g * n[q];
			}
			return front ? RF_FRONT : RF_BACK;
		}
	}
	for (q = 0; q < 3; q++) {
		out[q] = P[q] + eps * n[q];
		out[3 + q] = d[q] - (2.0f * dn) * n[q];
	}
	return transmit_m > 0 ? RF_TOTAL : RF_MIRROR;
}

static int rf_pixel(const float *o, const float *d, float t, int id, const int *mat_idx, const float *reflect,
		    const float *transmit, const float *ior, int mat_count, const float *vertlist, const int *trilist,
		    float eps, float *out)
{
	int m;
	if (!(t > 0) || id < 0)
		return 0;
	m = mat_idx[id];
	if (m < 0 || m >= mat_count)
		return 0;
	return rf_ray(o, d, t, id, vertlist, trilist, eps, transmit[m], reflect[m], ior[m], out);
}

/* level 1: from the camera and the primary hits */
void rf_refract_rays(const float *cam, const float *t_list, const float *dir_list, const int *id_list, const int *mat_idx,
		     const float *reflect, const float *transmit, const float *ior, int mat_count, const float *vertlist,
		     const int *trilist, float eps, int p0, int n, float *rays, int *active, int *kind)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, q;
		for (q = 0; q < 6; q++)
			rays[p * 6 + q] = 0.0f;
		kind[p] = rf_pixel(cam, &dir_list[p * 3], t_list[p], id_list[p], mat_idx, reflect, transmit, ior, mat_count,
				   vertlist, trilist, eps, &rays[p * 6]);
		active[p] = kind[p] != 0;
	}
}

/* level j -> j+1: from each ray's own origin */
void rf_refract_rays_next(const float *rays, const int *active, const float *hit_t, const int *hit_id, const int *mat_idx,
			  const float *reflect, const float *transmit, const float *ior, int mat_count,
			  const float *vertlist, const int *trilist, float eps, int p0, int n, float *rays_next,
			  int *active_next, int *kind)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, q;
		for (q = 0; q < 6; q++)
			rays_next[p * 6 + q] = 0.0f;
		kind[p] = 0;
		if (active[p])
			kind[p] = rf_pixel(&rays[p * 6], &rays[p * 6 + 3], hit_t[p], hit_id[p], mat_idx, reflect, transmit, ior,
					   mat_count, vertlist, trilist, eps, &rays_next[p * 6]);
		active_next[p] = kind[p] != 0;
	}
}
