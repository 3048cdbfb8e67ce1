/* texture_ref.c -- plain-C restatement of the texture calls (include/ugrt.h is the text), the
 * tests' checker.
 *
 * One loop per texel (tex_chain) and one per pixel (tex_albedo), nothing shared between iterations but the inputs.  Compiled
 * with -ffp-contract=off -fno-fast-math: every + - * / sqrt floor below is one IEEE fp32 operation, in the order it is
 * written.  Nothing here is taken from the library's sources: a texture's levels lie texture by texture in an array of
 * their own, the tap count is searched, not counted, and the reciprocal of the determinant is a division.  ugrt_fmath.h is
 * the ABI's own float-to-int rule. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ugrt_fmath.h"

typedef unsigned int u32;

#define EPSILON 1e-21f
#define MAX_DIM 4096
#define CROSS(d, a, b)                             \
	do {                                       \
		d[0] = a[1] * b[2] - a[2] * b[1];  \
		d[1] = a[2] * b[0] - a[0] * b[2];  \
		d[2] = a[0] * b[1] - a[1] * b[0];  \
	} while (0)
#define DOT(a, b) (a[0] * b[0] + a[1] * b[1] + a[2] * b[2])
#define NORMALIZE(a)                                                        \
	do {                                                                \
		float l_ = 1.0f / sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); \
		a[0] *= l_;                                                 \
		a[1] *= l_;                                                 \
		a[2] *= l_;                                                 \
	} while (0)

/* ---- the mip chain ---- */

int tex_levels(int w, int h)
{
	int n = 1;
	while (w > 1 || h > 1) {
		w = w > 1 ? w >> 1 : 1;
		h = h > 1 ? h >> 1 : 1;
		n++;
	}
	return n;
}

/* words of all levels of a w x h texture together */
int tex_chain_words(int w, int h)
{
	int n = w * h;
	while (w > 1 || h > 1) {
		w = w > 1 ? w >> 1 : 1;
		h = h > 1 ? h >> 1 : 1;
		n += w * h;
	}
	return n;
}

static int imin(int a, int b) { return a < b ? a : b; }

/* out: level 0, level 1, ... of the texture whose bytes are rgb[3 w h]; dims[2 l], dims[2 l + 1] = level l's size */
void tex_chain(const unsigned char *rgb, int w, int h, u32 *out, int *dims)
{
	int l = 0;
	for (int k = 0; k < w * h; k++)
		out[k] = (u32)rgb[3 * k] | (u32)rgb[3 * k + 1] << 8 | (u32)rgb[3 * k + 2] << 16 | 255u << 24;
	const u32 *src = out;
	for (;;) {
		if (dims) {
			dims[2 * l] = w;
			dims[2 * l + 1] = h;
		}
		if (w == 1 && h == 1)
			break;
		int nw = w > 1 ? w >> 1 : 1, nh = h > 1 ? h >> 1 : 1;
		u32 *dst = (u32 *)src + w * h;
		for (int y = 0; y < nh; y++)
			for (int x = 0; x < nw; x++) {
				int xa = imin(2 * x, w - 1), xb = imin(2 * x + 1, w - 1), ya = imin(2 * y, h - 1), yb = imin(2 * y + 1, h - 1);
				u32 word = 255u << 24;
				for (int c = 0; c < 3; c++) {
					u32 a = src[ya * w + xa] >> (8 * c) & 255u, b = src[ya * w + xb] >> (8 * c) & 255u;
					u32 d = src[yb * w + xa] >> (8 * c) & 255u, e = src[yb * w + xb] >> (8 * c) & 255u;
					word |= ((a + b + d + e + 2u) >> 2) << (8 * c);
				}
				dst[y * nw + x] = word;
			}
		src = dst;
		w = nw;
		h = nh;
		l++;
	}
}

/* ---- the per-pixel albedo ---- */

/* the primary pass's direction (trace_kernel.cu:96-114 as the oracle states it) at the image position (fcol, frow) */
static void eye_dir(const float *eye, const float *nodes, int W, int H, int strict, float fcol, float frow, float *d)
{
	float ftx = fcol / (float)W, fty = frow / (float)H;
	ftx = 1 - ftx;
	float xs = ftx * 4.0f, ys = fty * 4.0f;
	int i = ugrt_f2i(xs), j = ugrt_f2i(ys);
	i = i > 3 ? 3 : i;
	j = j > 3 ? 3 : j;
	float a = xs - (float)i, b = ys - (float)j;
	if (strict) {
		ugrt_tex_linear8(ftx * 0.8f + 0.1f, 5, &i, &a);
		ugrt_tex_linear8(fty * 0.8f + 0.1f, 5, &j, &b);
	}
	float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
	const float *n00 = nodes + (j * 5 + i) * 4, *n01 = nodes + ((j + 1) * 5 + i) * 4;
	for (int k = 0; k < 3; k++) {
		float T = ((w00 * n00[k] + w10 * n00[4 + k]) + w01 * n01[k]) + w11 * n01[4 + k];
		d[k] = T - eye[k];
	}
	NORMALIZE(d);
}

/* exported for the tests that aim triangles at chosen eye rays */
void tex_directions(const float *eye, const float *nodes, int W, int H, int strict, int n, const float *fcol, const float *frow,
		    float *d)
{
	for (int i = 0; i < n; i++)
		eye_dir(eye, nodes, W, H, strict, fcol[i], frow[i], d + 3 * (size_t)i);
}

/* uv of the ray (cam, d) on triangle (v0, v1, v2) with the corners' uvs c0, c1, c2; 0: the determinant failed */
static int ray_uv(const float *cam, const float *d, const float *v0, const float *v1, const float *v2, const float *c0,
		  const float *c1, const float *c2, float *uv)
{
	float tvec[3], e1[3], e2[3], pvec[3], qvec[3];
	for (int k = 0; k < 3; k++) {
		e1[k] = v1[k] - v0[k];
		e2[k] = v2[k] - v0[k];
		tvec[k] = cam[k] - v0[k];
	}
	CROSS(pvec, d, e2);
	float det = DOT(e1, pvec);
	int failed = det > -EPSILON && det < EPSILON;
	float inv = 1.0f / det;
	float u = DOT(tvec, pvec) * inv;
	CROSS(qvec, tvec, e1);
	float v = DOT(d, qvec) * inv;
	float w = (1.0f - u) - v;
	for (int k = 0; k < 2; k++)
		uv[k] = (w * c0[k] + u * c1[k]) + v * c2[k];
	return !failed;
}

static void axis(float a, int n, int *i0, int *i1, float *f)
{
	float a1 = a - floorf(a);
	float x = a1 * (float)n - 0.5f;
	float x0 = floorf(x);
	*f = x - x0;
	int c[2];
	c[0] = ugrt_f2i(x0);
	c[1] = (int)((u32)c[0] + 1u);
	for (int k = 0; k < 2; k++) {
		if (c[k] < 0)
			c[k] = (int)((u32)c[k] + (u32)n);
		if (c[k] >= n)
			c[k] -= n;
		if (c[k] < 0 || c[k] >= n)
			c[k] = 0;
	}
	*i0 = c[0];
	*i1 = c[1];
}

static void bilinear(const u32 *lv, int w, int h, float a, float b, float *out)
{
	int x0, x1, y0, y1;
	float fx, fy;
	axis(a, w, &x0, &x1, &fx);
	axis(b, h, &y0, &y1, &fy);
	for (int c = 0; c < 3; c++) {
		float c00 = (float)(lv[y0 * w + x0] >> (8 * c) & 255u), c10 = (float)(lv[y0 * w + x1] >> (8 * c) & 255u);
		float c01 = (float)(lv[y1 * w + x0] >> (8 * c) & 255u), c11 = (float)(lv[y1 * w + x1] >> (8 * c) & 255u);
		out[c] = (c00 * (1.0f - fx) + c10 * fx) * (1.0f - fy) + (c01 * (1.0f - fx) + c11 * fx) * fy;
	}
}

/* Pixels p0 .. p0 + n - 1 of a W x H frame.  Textures: ntex of them, wh[2 i], wh[2 i + 1], rgb = their bytes one behind
 * the other.  eye = camcoords[0..2] and eye_nodes = the node table of the current camera.  dbg (or null): per pixel {N, level, the fraction's bits, 1 = the pixel was filtered}. */
void tex_albedo(const float *t_value, const float *ray_dir, const int *ids, const float *cam, const float *verts,
		const int *tris, const float *uvlist, int num_uvs, const int *uv_faces, const int *mat_idx, const float *mat_list,
		int num_materials, const int *mat_texture, int ntex, const int *wh, const unsigned char *rgb, const float *eye, const float *eye_nodes,
		int W, int H, int strict, int max_aniso, int lod_bias, float *albedo, int p0, int n, int *dbg)
{
	u32 **chain = (u32 **)calloc((size_t)ntex + 1, sizeof(u32 *));
	int(*dims)[32] = (int(*)[32])calloc((size_t)ntex + 1, sizeof(int[32]));
	const unsigned char *at = rgb;
	for (int i = 0; i < ntex; i++) {
		chain[i] = (u32 *)malloc(sizeof(u32) * (size_t)tex_chain_words(wh[2 * i], wh[2 * i + 1]));
		tex_chain(at, wh[2 * i], wh[2 * i + 1], chain[i], dims[i]);
		at += 3 * (size_t)wh[2 * i] * wh[2 * i + 1];
	}
	float bias_scale = 1.0f;
	for (int k = 0; k < (lod_bias < 0 ? -lod_bias : lod_bias); k++)
		bias_scale = lod_bias < 0 ? bias_scale / 2.0f : bias_scale * 2.0f;
	for (int p = p0; p < p0 + n; p++) {
		float *out = albedo + 3 * (size_t)p;
		int id = ids[p];
		float t = t_value[p];
		if (dbg)
			dbg[4 * p] = dbg[4 * p + 1] = dbg[4 * p + 2] = dbg[4 * p + 3] = 0;
		out[0] = out[1] = out[2] = 0.0f;
		if (id < 0 || !(t > 0.0f))
			continue;
		int m = mat_idx[id];
		if (m < 0 || m >= num_materials)
			continue;
		const float *kd = mat_list + 6 * m + 3;
		out[0] = kd[0], out[1] = kd[1], out[2] = kd[2];
		int T = mat_texture[m];
		if (T < 0 || T >= ntex)
			continue;
		const int *ui = uv_faces + 3 * (size_t)id;
		if (ui[0] < 0 || ui[0] >= num_uvs || ui[1] < 0 || ui[1] >= num_uvs || ui[2] < 0 || ui[2] >= num_uvs)
			continue;
		const float *v0 = verts + 3 * tris[3 * id], *v1 = verts + 3 * tris[3 * id + 1], *v2 = verts + 3 * tris[3 * id + 2];
		const float *c0 = uvlist + 2 * ui[0], *c1 = uvlist + 2 * ui[1], *c2 = uvlist + 2 * ui[2];
		float uv[2], uvx[2], uvy[2], dn[3];
		if (!ray_uv(cam, ray_dir + 3 * (size_t)p, v0, v1, v2, c0, c1, c2, uv))
			continue;
		if (!(fabsf(uv[0]) < INFINITY) || !(fabsf(uv[1]) < INFINITY))
			continue;
		int row = p / W, col = p - row * W;
		eye_dir(eye, eye_nodes, W, H, strict, (float)(col + 1), (float)row, dn);
		int okx = ray_uv(cam, dn, v0, v1, v2, c0, c1, c2, uvx);
		eye_dir(eye, eye_nodes, W, H, strict, (float)col, (float)(row + 1), dn);
		int oky = ray_uv(cam, dn, v0, v1, v2, c0, c1, c2, uvy);
		const int *dm = dims[T];
		int last = tex_levels(dm[0], dm[1]) - 1;
		float W0 = (float)dm[0], H0 = (float)dm[1];
		float dx[2] = { (uvx[0] - uv[0]) * W0, (uvx[1] - uv[1]) * H0 }, dy[2] = { (uvy[0] - uv[0]) * W0, (uvy[1] - uv[1]) * H0 };
		float Lx = sqrtf(dx[0] * dx[0] + dx[1] * dx[1]), Ly = sqrtf(dy[0] * dy[0] + dy[1] * dy[1]);
		float LIM = (float)(2 * MAX_DIM * 16);
		float major[2] = { 0.0f, 0.0f };
		int N = 1, e = last;
		float f = 0.0f;
		if (okx && oky && Lx < LIM && Ly < LIM) {
			float Lmax = Lx, Lmin = Ly;
			major[0] = dx[0], major[1] = dx[1];
			if (Ly > Lx) {
				Lmax = Ly, Lmin = Lx;
				major[0] = dy[0], major[1] = dy[1];
			}
			N = max_aniso;
			for (int k = 1; k <= max_aniso; k++)
				if (Lmin * (float)k >= Lmax) {
					N = k;
					break;
				}
			float lambda = (Lmax / (float)N) * bias_scale;
			e = 0;
			if (lambda > 1.0f) {
				u32 bits;
				memcpy(&bits, &lambda, 4);
				e = (int)(bits >> 23 & 255u) - 127;
				float pw = 1.0f;
				for (int k = 0; k < e; k++)
					pw = pw * 2.0f;
				f = lambda / pw - 1.0f;
				if (e >= last) {
					e = last;
					f = 0.0f;
				}
			}
		}
		const u32 *lvA = chain[T], *lvB;
		for (int l = 0; l < e; l++)
			lvA += dm[2 * l] * dm[2 * l + 1];
		lvB = lvA + dm[2 * e] * dm[2 * e + 1];
		float acc[3] = { 0.0f, 0.0f, 0.0f };
		for (int i = 0; i < N; i++) {
			float s = (float)(2 * i + 1) / (float)(2 * N) - 0.5f;
			float a = uv[0] + (s * major[0]) / W0, b = uv[1] + (s * major[1]) / H0;
			float A[3], B[3];
			bilinear(lvA, dm[2 * e], dm[2 * e + 1], a, b, A);
			if (f != 0.0f) {
				bilinear(lvB, dm[2 * e + 2], dm[2 * e + 3], a, b, B);
				for (int c = 0; c < 3; c++)
					A[c] = (1.0f - f) * A[c] + f * B[c];
			}
			for (int c = 0; c < 3; c++)
				acc[c] = acc[c] + A[c];
		}
		for (int c = 0; c < 3; c++)
			out[c] = kd[c] * ((acc[c] / (float)N) / 255.0f);
		if (dbg) {
			dbg[4 * p] = N;
			dbg[4 * p + 1] = e;
			memcpy(&dbg[4 * p + 2], &f, 4);
			dbg[4 * p + 3] = 1;
		}
	}
	for (int i = 0; i < ntex; i++)
		free(chain[i]);
	free(chain);
	free(dims);
}

/* The reference image of the aliasing figure: sub x sub eye rays per pixel, at (col + (i + 1/2) / sub - 1/2,
 * row + (j + 1/2) / sub - 1/2) -- the square of one pixel's side around the pixel's own ray, which the filter's taps are
 * centred on --, each met with the plane of the pixel's triangle as
 * above, its uv sampled bilinearly on level 0, the samples averaged in double.  The pixels tex_albedo does not filter get
 * what it gives them; a sample whose determinant fails is left out.  Not compared to the bit with anything. */
void tex_albedo_super(const float *t_value, const float *ray_dir, const int *ids, const float *cam, const float *verts,
		      const int *tris, const float *uvlist, int num_uvs, const int *uv_faces, const int *mat_idx,
		      const float *mat_list, int num_materials, const int *mat_texture, int ntex, const int *wh,
		      const unsigned char *rgb, const float *eye, const float *eye_nodes, int W, int H, int sub, float *albedo, int p0,
		      int n)
{
	tex_albedo(t_value, ray_dir, ids, cam, verts, tris, uvlist, num_uvs, uv_faces, mat_idx, mat_list, num_materials, mat_texture,
		   ntex, wh, rgb, eye, eye_nodes, W, H, 0, 1, 0, albedo, p0, n, NULL);
	u32 **level0 = (u32 **)calloc((size_t)ntex + 1, sizeof(u32 *));
	const unsigned char *at = rgb;
	for (int i = 0; i < ntex; i++) {
		int w = wh[2 * i], h = wh[2 * i + 1];
		level0[i] = (u32 *)malloc(sizeof(u32) * (size_t)w * h);
		for (int k = 0; k < w * h; k++)
			level0[i][k] = (u32)at[3 * k] | (u32)at[3 * k + 1] << 8 | (u32)at[3 * k + 2] << 16 | 255u << 24;
		at += 3 * (size_t)w * h;
	}
	for (int p = p0; p < p0 + n; p++) {
		int id = ids[p];
		if (id < 0 || !(t_value[p] > 0.0f))
			continue;
		int m = mat_idx[id];
		if (m < 0 || m >= num_materials)
			continue;
		int T = mat_texture[m];
		const int *ui = uv_faces + 3 * (size_t)id;
		if (T < 0 || T >= ntex || ui[0] < 0 || ui[0] >= num_uvs || ui[1] < 0 || ui[1] >= num_uvs || ui[2] < 0 || ui[2] >= num_uvs)
			continue;
		const float *v0 = verts + 3 * tris[3 * id], *v1 = verts + 3 * tris[3 * id + 1], *v2 = verts + 3 * tris[3 * id + 2];
		const float *c0 = uvlist + 2 * ui[0], *c1 = uvlist + 2 * ui[1], *c2 = uvlist + 2 * ui[2];
		float uv[2], d[3];
		if (!ray_uv(cam, ray_dir + 3 * (size_t)p, v0, v1, v2, c0, c1, c2, uv) || !(fabsf(uv[0]) < INFINITY) ||
		    !(fabsf(uv[1]) < INFINITY))
			continue;
		int row = p / W, col = p - row * W, count = 0;
		double sum[3] = { 0.0, 0.0, 0.0 };
		for (int j = 0; j < sub; j++)
			for (int i = 0; i < sub; i++) {
				float s[3];
				eye_dir(eye, eye_nodes, W, H, 0, ((float)col - 0.5f) + ((float)i + 0.5f) / (float)sub,
					((float)row - 0.5f) + ((float)j + 0.5f) / (float)sub, d);
				if (!ray_uv(cam, d, v0, v1, v2, c0, c1, c2, uv) || !(fabsf(uv[0]) < INFINITY) || !(fabsf(uv[1]) < INFINITY))
					continue;
				bilinear(level0[T], wh[2 * T], wh[2 * T + 1], uv[0], uv[1], s);
				for (int c = 0; c < 3; c++)
					sum[c] += s[c];
				count++;
			}
		if (count)
			for (int c = 0; c < 3; c++)
				albedo[3 * (size_t)p + c] = (float)(mat_list[6 * m + 3 + c] * (sum[c] / count / 255.0));
	}
	for (int i = 0; i < ntex; i++)
		free(level0[i]);
	free(level0);
}
