/*
 * ambient_ref.c -- CPU restatement of ambient occlusion, the checker of ugrt_ao_rays,
 * ugrt_trace_dda_any_hemi and ugrt_shade_ao (tests/test_ambient.py builds and loads it).
 *
 * Test infrastructure only.  ao_expand writes out, for ONE direction s, the explicit rays {o, D_s} that the kernel
 * forms in registers; the expected mask is oc_trace_any of tests/occlusion_ref.c on those rays at t_max = radius, once
 * per s: the walk has no second restatement here.  The basis is written out case by case, with nothing shared with the
 * kernel's text.  Build: gcc -O2 -fPIC -ffp-contract=off -fno-fast-math -fopenmp -I include, as the oracle.  Arrays are
 * indexed by absolute pixel p = p0 + i of a W*H frame.
 */
#include <stddef.h>

#include "ugrt_fmath.h"

/* for a pixel with t > 0 and id >= 0 (a triangle id), whatever its material: P = cam + t*d, n = normalize(e1 x e2)
 * turned so that d.n <= 0, orays = {P + eps*n, n}, oactive 1; every other pixel of the band: six zeros and 0 */
void ao_rays(const float *cam_pos, const float *t_list, const float *dir_list, const int *id_list,
	     const float *vertlist, const int *trilist, float eps, int p0, int n, float *orays, int *oactive)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k, id = id_list[p];
		float t = t_list[p], e1[3], e2[3], nn[3], P[3], l, dn;
		const float *d = &dir_list[p * 3];
		oactive[p] = 0;
		for (k = 0; k < 6; k++)
			orays[p * 6 + k] = 0.0f;
		if (!(t > 0) || id < 0)
			continue;
		for (k = 0; k < 3; k++) {
			float v0 = vertlist[3 * trilist[id * 3 + 0] + k];
			e1[k] = vertlist[3 * trilist[id * 3 + 1] + k] - v0;
			e2[k] = vertlist[3 * trilist[id * 3 + 2] + k] - v0;
			P[k] = cam_pos[k] + t * d[k];
		}
		nn[0] = e1[1] * e2[2] - e1[2] * e2[1];
		nn[1] = e1[2] * e2[0] - e1[0] * e2[2];
		nn[2] = e1[0] * e2[1] - e1[1] * e2[0];
		l = 1.0f / __builtin_sqrtf(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
		nn[0] *= l;
		nn[1] *= l;
		nn[2] *= l;
		dn = d[0] * nn[0] + d[1] * nn[1] + d[2] * nn[2];
		if (dn > 0) {
			nn[0] = -nn[0];
			nn[1] = -nn[1];
			nn[2] = -nn[2];
		}
		for (k = 0; k < 3; k++) {
			orays[p * 6 + k] = P[k] + eps * nn[k];
			orays[p * 6 + 3 + k] = nn[k];
		}
		oactive[p] = 1;
	}
}

/* the tangent frame over the normal n: a = the index of the smallest |n[k]| (strict <: 1 against 0, then 2 against the
 * winner, so ties go to the lowest k); u = n x e_a; T = u / |u|; B = n x T */
void ao_basis(const float *n, float *T, float *B)
{
	float a0 = __builtin_fabsf(n[0]), a1 = __builtin_fabsf(n[1]), a2 = __builtin_fabsf(n[2]);
	float best = a0, u0, u1, u2, l;
	int a = 0;
	if (a1 < best) {
		a = 1;
		best = a1;
	}
	if (a2 < best)
		a = 2;
	switch (a) {
	case 0: /* n x (1,0,0) */
		u0 = 0.0f;
		u1 = n[2];
		u2 = -n[1];
		break;
	case 1: /* n x (0,1,0) */
		u0 = -n[2];
		u1 = 0.0f;
		u2 = n[0];
		break;
	default: /* n x (0,0,1) */
		u0 = n[1];
		u1 = -n[0];
		u2 = 0.0f;
		break;
	}
	l = 1.0f / __builtin_sqrtf(u0 * u0 + u1 * u1 + u2 * u2);
	T[0] = u0 * l;
	T[1] = u1 * l;
	T[2] = u2 * l;
	B[0] = n[1] * T[2] - n[2] * T[1];
	B[1] = n[2] * T[0] - n[0] * T[2];
	B[2] = n[0] * T[1] - n[1] * T[0];
}

/* the explicit rays of ONE local direction dir = (x, y, z): for an active pixel rays = {o, (x*T + y*B) + z*n} over the
 * basis of its normal; every other pixel of the band: six zeros */
void ao_expand(const float *orays, const int *oactive, const float *dir, int p0, int n, float *rays)
{
	int i;
#pragma omp parallel for schedule(static)
	for (i = 0; i < n; i++) {
		int p = p0 + i, k;
		const float *nn = &orays[p * 6 + 3];
		float T[3], B[3];
		for (k = 0; k < 6; k++)
			rays[p * 6 + k] = 0.0f;
		if (!oactive[p])
			continue;
		ao_basis(nn, T, B);
		for (k = 0; k < 3; k++) {
			rays[p * 6 + k] = orays[p * 6 + k];
			rays[p * 6 + 3 + k] = (dir[0] * T[k] + dir[1] * B[k]) + dir[2] * nn[k];
		}
	}
}

/* open = num_dirs - popcount(mask & low num_dirs bits); each byte b of the pixel becomes (b * open) / num_dirs */
void ao_shade(unsigned char *img, const unsigned *mask, int num_dirs, int p0, int n)
{
	int i;
	for (i = 0; i < n; i++) {
		int p = p0 + i, s, k;
		unsigned closed = 0, open;
		for (s = 0; s < num_dirs; s++)
			closed += (mask[p] >> s) & 1u;
		open = (unsigned)num_dirs - closed;
		for (k = 0; k < 3; k++)
			img[p * 3 + k] = (unsigned char)(((unsigned)img[p * 3 + k] * open) / (unsigned)num_dirs);
	}
}
