/* smooth_ref.c -- plain-C restatement of the smooth-shading calls, the tests' checker.
 *
 * One loop per corner and one per pixel, nothing shared between iterations but the inputs.  Compiled with
 * -ffp-contract=off -fno-fast-math: every + - * / sqrt below is one IEEE fp32 operation, in the order it is written.
 * Nothing here is taken from the library's sources; the macros restate the reference's CROSS / DOT / NORMALIZE. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define EPSILON 1e-21f
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

static int finite3(const float *v)
{
	return fabsf(v[0]) < INFINITY && fabsf(v[1]) < INFINITY && fabsf(v[2]) < INFINITY;
}

static int key_of(const int *faces, const int *vkey, int c)
{
	return vkey ? vkey[faces[c]] : faces[c];
}

/* corners[3F]: the corner indices stably sorted by key; start[V + 1] */
void smooth_adjacency(const int *faces, int F, int V, const int *vkey, unsigned *corners, unsigned *start)
{
	int n = 3 * F;
	unsigned *fill = (unsigned *)calloc((size_t)V + 1, sizeof(unsigned));
	memset(start, 0, ((size_t)V + 1) * sizeof(unsigned));
	for (int c = 0; c < n; c++)
		start[key_of(faces, vkey, c) + 1]++;
	for (int k = 0; k < V; k++)
		start[k + 1] += start[k];
	for (int c = 0; c < n; c++) {
		int k = key_of(faces, vkey, c);
		corners[start[k] + fill[k]++] = (unsigned)c;
	}
	free(fill);
}

static void face_normals(const int *faces, const float *verts, int g, float *A, float *N)
{
	const float *v0 = verts + 3 * faces[3 * g], *v1 = verts + 3 * faces[3 * g + 1], *v2 = verts + 3 * faces[3 * g + 2];
	float e1[3], e2[3];
	for (int k = 0; k < 3; k++) {
		e1[k] = v1[k] - v0[k];
		e2[k] = v2[k] - v0[k];
	}
	CROSS(A, e1, e2);
	N[0] = A[0], N[1] = A[1], N[2] = A[2];
	NORMALIZE(N);
}

/* out[9F]; corners / start: smooth_adjacency's */
void smooth_corner_normals(const int *faces, const float *verts, int F, const int *vkey, const unsigned *corners,
			   const unsigned *start, float crease_cos, float *out)
{
	for (int c = 0; c < 3 * F; c++) {
		int f = c / 3, K = key_of(faces, vkey, c);
		float Af[3], Nf[3], S[3] = { 0.0f, 0.0f, 0.0f };
		face_normals(faces, verts, f, Af, Nf);
		for (unsigned j = start[K]; j < start[K + 1]; j++) {
			int g = (int)(corners[j] / 3u);
			float Ag[3], Ng[3];
			face_normals(faces, verts, g, Ag, Ng);
			int in = g == f;
			if (!in && crease_cos <= -1.0f)
				in = 1;
			else if (!in && !(crease_cos > 1.0f))
				in = (Nf[0] * Ng[0] + Nf[1] * Ng[1]) + Nf[2] * Ng[2] >= crease_cos;
			if (in) {
				S[0] = S[0] + Ag[0];
				S[1] = S[1] + Ag[1];
				S[2] = S[2] + Ag[2];
			}
		}
		NORMALIZE(S);
		int ok = finite3(S);
		for (int k = 0; k < 3; k++)
			out[3 * c + k] = ok ? S[k] : Nf[k];
	}
}

/* pixels p0 .. p0 + n - 1; normal_out may be normal_in */
void smooth_normals(const float *t_value, const float *ray_dir, const int *ids, const float *cam_pos, const float *verts,
		    const int *tris, const float *cn, const float *normal_in, int fold, float *normal_out, int p0, int n)
{
	for (int p = p0; p < p0 + n; p++) {
		int id = ids[p];
		float t = t_value[p];
		if (id < 0 || !(t > 0.0f)) {
			for (int k = 0; k < 3; k++)
				normal_out[3 * p + k] = normal_in[3 * p + k];
			continue;
		}
		const float *v0 = verts + 3 * tris[3 * id], *v1 = verts + 3 * tris[3 * id + 1], *v2 = verts + 3 * tris[3 * id + 2];
		const float *d = ray_dir + 3 * p, *c0 = cn + 9 * (size_t)id;
		float tvec[3], e1[3], e2[3], pvec[3], qvec[3], nn[3], ng[3];
		for (int k = 0; k < 3; k++) {
			e1[k] = v1[k] - v0[k];
			e2[k] = v2[k] - v0[k];
			tvec[k] = cam_pos[k] - v0[k];
		}
		CROSS(pvec, d, e2);
		float det = DOT(e1, pvec);
		int failed = det > -EPSILON && det < EPSILON;
		float inv_det = 1.0f / det;
		float u = DOT(tvec, pvec) * inv_det;
		CROSS(qvec, tvec, e1);
		float v = DOT(d, qvec) * inv_det;
		float w = (1.0f - u) - v;
		for (int k = 0; k < 3; k++)
			nn[k] = (w * c0[k] + u * c0[3 + k]) + v * c0[6 + k];
		NORMALIZE(nn);
		CROSS(ng, e1, e2);
		NORMALIZE(ng);
		int keep = !failed && finite3(nn) && DOT(nn, ng) > 0.0f;
		for (int k = 0; k < 3; k++) {
			float c = keep ? nn[k] : ng[k];
			if (fold)
				c = c < 0 ? c * -1 : c;
			normal_out[3 * p + k] = c;
		}
	}
}
