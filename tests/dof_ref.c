/*
 * dof_ref.c -- CPU restatement of the depth of field, the checker of ugrt_dof_pixels and
 * ugrt_dof_gather (tests/test_dof.py and tests/test_dof_synthetic.py build and load it).
 *
 * Test infrastructure only.  One loop per sample: the eye ray of aa_ref.c through (col + sx, row + sy), moved onto the
 * point (lu, lv) of the lens and tilted towards the focus plane, then aa_ref.c's own walk, gate, shading and any-hit walk
 * on that ray -- aa_ref.c is included as it stands and its static functions are called.  dof_pixels is the definition
 * itself: one loop that forms every pixel's circle, one loop over the (2R + 1)^2 window of every pixel; the kernel
 * dilates integer reaches in two passes over LDS tiles.  Build: as aa_ref.c.  Arrays are indexed by absolute pixel p of
 * a W*H frame; a band is the pixels p0 .. p0 + n - 1; per-sample arrays lie at s * N + p.
 */
#include "aa_ref.c"

/* the circle of confusion of every pixel of the image: coc[W * H] */
void dof_coc(const float *t, const float *dir, const int *ids, const float *A, float F, float coc_scale, int W, int H,
	     float *coc)
{
	int q;
	for (q = 0; q < W * H; q++) {
		coc[q] = 0.0f;
		if (t[q] > 0 && ids[q] >= 0) {
			float z = t[q] * ((dir[3 * q] * A[0] + dir[3 * q + 1] * A[1]) + dir[3 * q + 2] * A[2]);
			if (z > 0)
				coc[q] = coc_scale * __builtin_fabsf(z - F) / z;
		}
	}
}

/* ugrt_dof_pixels; coc: W * H floats of scratch */
void dof_pixels(const float *t, const float *dir, const int *ids, const float *A, float F, float coc_scale, float coc_min,
		int R, int W, int H, int p0, int n, float *coc, int *flag)
{
	int i;
	dof_coc(t, dir, ids, A, F, coc_scale, W, H, coc);
	for (i = 0; i < n; i++) {
		int p = p0 + i, y = p / W, x = p - y * W, dx, dy, f = 0;
		for (dy = -R; dy <= R; dy++) {
			for (dx = -R; dx <= R; dx++) {
				int qx = x + dx, qy = y + dy, ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, m = ax > ay ? ax : ay;
				float c;
				if (qx < 0 || qx >= W || qy < 0 || qy >= H)
					continue;
				c = coc[qy * W + qx];
				if (c >= coc_min && c >= (float)m)
					f = 1;
			}
		}
		flag[p] = f;
	}
}

/* the lens ray of one table entry ent = (sx, sy, lu, lv) at pixel (x, y): o[3], d[3] */
static void dof_ray(const float *eye_cc, const float *tex, int strict, int W, int H, const float *lens, const float *ent, int x,
		    int y, float *o, float *d)
{
	const float *U = lens, *V = lens + 3, *A = lens + 6;
	float sx = ent[0] > -0.5f ? ent[0] : -0.5f, sy = ent[1] > -0.5f ? ent[1] : -0.5f, lu = ent[2], lv = ent[3], c, s_f;
	int k;
	sx = sx < 0.5f ? sx : 0.5f;
	sy = sy < 0.5f ? sy : 0.5f;
	lu = lu != lu ? 0.0f : (lu < -1.0f ? -1.0f : (lu > 1.0f ? 1.0f : lu));
	lv = lv != lv ? 0.0f : (lv < -1.0f ? -1.0f : (lv > 1.0f ? 1.0f : lv));
	aa_dir(eye_cc, tex, W, H, strict, (float)x + sx, (float)y + sy, d);
	for (k = 0; k < 3; k++)
		o[k] = eye_cc[k];
	c = (d[0] * A[0] + d[1] * A[1]) + d[2] * A[2];
	if (!(c > 0))
		return;
	s_f = lens[9] / c;
	for (k = 0; k < 3; k++) {
		float L = lu * U[k] + lv * V[k];
		o[k] = eye_cc[k] + L;
		d[k] = d[k] - L / s_f;
	}
}

/* dof_ray for n (pixel, entry) pairs, exported for the tests of the ray itself; px, py: [n]; ent: [n][4]; o, d: [n][3] */
void dof_rays(const float *eye_cc, const float *tex, int strict, int W, int H, const float *lens, int n, const int *px,
	      const int *py, const float *ent, float *o, float *d)
{
	int i;
	for (i = 0; i < n; i++)
		dof_ray(eye_cc, tex, strict, W, H, lens, ent + 4 * (size_t)i, px[i], py[i], o + 3 * (size_t)i, d + 3 * (size_t)i);
}

/* ugrt_dof_gather.  The arguments are aa_gather's, with the lens and a table of four floats per entry. */
void dof_gather(const float *g, const int *dims, const u32 *value_list, const u32 *span, const u32 *offset,
		const float *vertlist, const int *trilist, const float *eye_cc, const float *tex, int strict, int W, int H,
		const float *lens, const int *flags, int S, int set_w, int set_h, const float *table, const int *mat_idx,
		const float *mat_list, int mat_count, const float *cc, const float *light, const float *shadow_light, float eps,
		int p0, int n, long long N, u32 *sum, float *hit_t, int *hit_id)
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
		if (!flags[p])
			continue;
		for (s = 0; s < S; s++) {
			size_t q = (size_t)s * (size_t)N + (size_t)p;
			const float *ent = &table[4 * (((y % set_h) * set_w + x % set_w) * S + s)];
			float o[3], D[3], t = -1.0f, P[3], hz, hw, e1[3], e2[3], nn[3], hmat[6], L[3] = { 0.0f, 0.0f, 0.0f };
			unsigned char b[3];
			int id, hm, occ = 0;
			dof_ray(eye_cc, tex, strict, W, H, lens, ent, x, y, o, D);
			id = aa_closest(g, dims, value_list, span, offset, vertlist, trilist, o, D, &t);
			if (id < 0)
				continue;
			/* the primary epilogue's gate under the eye's MVP */
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
			if (shadow_light) { /* the occlusion ray of the hit, the light at t = 1 */
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
		for (k = 0; k < 3; k++)
			sum[4 * (size_t)p + k] = acc[k];
		sum[4 * (size_t)p + 3] = 1u;
	}
}
