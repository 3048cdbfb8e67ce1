// ugrt_smooth.hip -- smooth shading: crease-aware vertex normals, interpolated per pixel (not in the reference;
// DESIGN.md section 6.15).
//
// Three calls.  ugrt_smooth_adjacency (topology): the corners c = 3f + k of the face list, stably sorted by the key of
// their vertex, and start[] per key -- the context's own radix sort on ceil(log2 V) key bits and one binary search per
// key, no host pass.  ugrt_smooth_corner_normals (geometry): per face the area-weighted normal A = e1 x e2 and its unit
// N, then per corner the sum of the A of the faces around its key that lie within the crease angle of its own face, in
// list order, by ONE thread (the order of a float sum is part of the specification: no atomics, no sum split across
// lanes).  ugrt_smooth_normals (per pixel): the barycentric mix of the hit triangle's three corner normals.
//   * the corner kernel's thread i serves the corner at position i of the SORTED list: the lanes of a wave then walk the
//     lists of the same or of neighbouring keys -- equal trip counts, and the same face records, which the first lane's
//     miss brings into the cache for the others.  In face order the three corners of a face would walk three unrelated
//     lists side by side.  The price is the scattered 12-byte store per corner;
//   * A and N are stored per face (two float4: 32 bytes, one aligned gather each), not recomputed per list entry: a
//     vertex shared by k faces costs k * k additions and dot products (accepted: DESIGN.md 6.15), it should not cost
//     k * k cross products, square roots and divisions as well.
// Arithmetic: DESIGN.md section 3 -- no contraction, D_CROSS / D_DOT / D_NORMALIZE of ugrt_dev.h.
#include "ugrt_dev.h"

#define SM_THREADS 256

// which faces of a key's list a corner sums: by the crease test, all of them (crease_cos <= -1), its own only (> 1)
enum { SM_TEST = 0, SM_ALL = 1, SM_OWN = 2 };

__device__ __forceinline__ bool d_finite3(const float *v)
{
	return __builtin_fabsf(v[0]) < __builtin_inff() && __builtin_fabsf(v[1]) < __builtin_inff() &&
	       __builtin_fabsf(v[2]) < __builtin_inff(); // (a NaN compares false)
}

// key and value of every corner: the key of its vertex, its own index.  An index outside 0..V-1 is a broken promise
// (ugrt.h); it is pulled into the range so that nothing is read or, later, written out of bounds.
__global__ __launch_bounds__(SM_THREADS) void k_smooth_keys(const int *__restrict__ faces, const int *__restrict__ vkey,
							     u32 n, u32 V, u32 *__restrict__ key, u32 *__restrict__ val)
{
	const u32 c = blockIdx.x * SM_THREADS + threadIdx.x;
	if (c >= n)
		return;
	u32 v = (u32)faces[c];
	v = v < V ? v : V - 1u;
	if (vkey) {
		v = (u32)vkey[v];
		v = v < V ? v : V - 1u;
	}
	key[c] = v;
	val[c] = c;
}

// start[k] = the first position of the sorted keys that holds a key >= k, for k = 0..V (start[V] = n)
__global__ __launch_bounds__(SM_THREADS) void k_smooth_starts(const u32 *__restrict__ sorted, u32 n, u32 V,
							       u32 *__restrict__ start)
{
	const u32 k = blockIdx.x * SM_THREADS + threadIdx.x;
	if (k > V)
		return;
	u32 lo = 0u, hi = n;
	while (lo < hi) {
		const u32 mid = lo + ((hi - lo) >> 1);
		if (sorted[mid] < k)
			lo = mid + 1u;
		else
			hi = mid;
	}
	start[k] = lo;
}

// per face: {A, .} and {N, .}
__global__ __launch_bounds__(SM_THREADS) void k_smooth_faces(const int *__restrict__ faces, const float *__restrict__ verts,
							      u32 F, float4 *__restrict__ rec)
{
	const u32 f = blockIdx.x * SM_THREADS + threadIdx.x;
	if (f >= F)
		return;
	float t9[9], A[3], N[3];
	d_stage_triangle(verts, faces, f, 0.0f, 0.0f, 0.0f, t9);
	const float *e1 = &t9[3], *e2 = &t9[6];
	D_CROSS(A, e1, e2);
	N[0] = A[0], N[1] = A[1], N[2] = A[2];
	D_NORMALIZE(N);
	rec[2 * (size_t)f] = make_float4(A[0], A[1], A[2], 0.0f);
	rec[2 * (size_t)f + 1] = make_float4(N[0], N[1], N[2], 0.0f);
}

// thread i: the corner at position i of the sorted list
template <int MODE>
__global__ __launch_bounds__(SM_THREADS) void k_smooth_corners(const u32 *__restrict__ corners, const u32 *__restrict__ skeys,
								const u32 *__restrict__ start, const float4 *__restrict__ rec, u32 n,
								float crease_cos, float *__restrict__ out)
{
	const u32 i = blockIdx.x * SM_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const u32 c = corners[i], K = skeys[i];
	const u32 f = c / 3u;
	const float4 nf = rec[2 * (size_t)f + 1];
	const float Nf[3] = { nf.x, nf.y, nf.z };
	float S[3] = { 0.0f, 0.0f, 0.0f };
	const u32 end = start[K + 1u];
	for (u32 j = start[K]; j < end; j++) {
		const u32 g = corners[j] / 3u;
		bool in = g == f || MODE == SM_ALL;
		if (MODE == SM_TEST && !in) {
			const float4 ng = rec[2 * (size_t)g + 1];
			in = (Nf[0] * ng.x + Nf[1] * ng.y) + Nf[2] * ng.z >= crease_cos; // (a NaN rejects)
		}
		if (in) {
			const float4 a = rec[2 * (size_t)g];
			S[0] = S[0] + a.x;
			S[1] = S[1] + a.y;
			S[2] = S[2] + a.z;
		}
	}
	D_NORMALIZE(S);
	const bool ok = d_finite3(S);
	out[3 * (size_t)c + 0] = ok ? S[0] : Nf[0];
	out[3 * (size_t)c + 1] = ok ? S[1] : Nf[1];
	out[3 * (size_t)c + 2] = ok ? S[2] : Nf[2];
}

extern "C" int ugrt_smooth_adjacency(ugrt_ctx *ctx, const int *d_facelist, int num_faces, int num_vertices,
				     const int *d_vertex_key)
{
	if (!ctx)
		return ugrt_fail(UGRT_EINVAL, "smooth_adjacency: null ctx");
	if (num_faces < 0 || num_vertices < 0)
		return ugrt_fail(UGRT_EINVAL, "smooth_adjacency: negative count (%d faces, %d vertices)", num_faces, num_vertices);
	if (num_faces > 0 && !d_facelist)
		return ugrt_fail(UGRT_EINVAL, "smooth_adjacency: null d_facelist with %d faces", num_faces);
	if (num_faces > 0 && num_vertices == 0)
		return ugrt_fail(UGRT_EINVAL, "smooth_adjacency: %d faces over no vertex", num_faces);
	if ((size_t)num_faces * 3u > ((size_t)1 << 30))
		return ugrt_fail(UGRT_EINVAL, "smooth_adjacency: %d faces exceed 2^30 corners", num_faces);
	UGRT_HIP(hipSetDevice(ctx->device));
	const u32 n = 3u * (u32)num_faces, V = (u32)num_vertices;
	ctx->sm_valid = false;
	int rc;
	for (int j = 0; j < 2; j++)
		if ((rc = ugrt_buf_reserve(ctx, ctx->sm_key[j], (size_t)n * 4)) || (rc = ugrt_buf_reserve(ctx, ctx->sm_val[j], (size_t)n * 4)))
			return rc;
	if ((rc = ugrt_buf_reserve(ctx, ctx->sm_start, ((size_t)V + 1) * 4)))
		return rc;
	int bits = 1;
	while (bits < 32 && ((size_t)1 << bits) < (size_t)V)
		bits++;
	ugrt_prof_begin(ctx, UGRT_ST_BUILD_SORT);
	if (n) {
		hipLaunchKernelGGL(k_smooth_keys, dim3((n + SM_THREADS - 1) / SM_THREADS), dim3(SM_THREADS), 0, ctx->stream, d_facelist,
				   d_vertex_key, n, V, (u32 *)ctx->sm_key[0].p, (u32 *)ctx->sm_val[0].p);
		rc = ugrt_sort_pairs_u32(ctx, (const u32 *)ctx->sm_key[0].p, (u32 *)ctx->sm_key[1].p, (const u32 *)ctx->sm_val[0].p,
					 (u32 *)ctx->sm_val[1].p, n, bits);
	}
	if (!rc)
		hipLaunchKernelGGL(k_smooth_starts, dim3((V + 1u + SM_THREADS - 1) / SM_THREADS), dim3(SM_THREADS), 0, ctx->stream,
				   (const u32 *)ctx->sm_key[1].p, n, V, (u32 *)ctx->sm_start.p);
	ugrt_prof_end(ctx, UGRT_ST_BUILD_SORT);
	if (rc)
		return rc;
	UGRT_HIP(hipGetLastError());
	ctx->sm_faces = num_faces;
	ctx->sm_vertices = num_vertices;
	ctx->sm_valid = true;
	ctx->sm_adjacency_builds++;
	return UGRT_OK;
}

extern "C" int ugrt_smooth_get_adjacency(ugrt_ctx *ctx, const unsigned **d_corners, const unsigned **d_start)
{
	if (!ctx || !d_corners || !d_start)
		return ugrt_fail(UGRT_EINVAL, "smooth_get_adjacency: null argument");
	if (!ctx->sm_valid)
		return ugrt_fail(UGRT_EINVAL, "smooth_get_adjacency: the adjacency has not been built");
	*d_corners = (const unsigned *)ctx->sm_val[1].p;
	*d_start = (const unsigned *)ctx->sm_start.p;
	return UGRT_OK;
}

extern "C" int ugrt_smooth_corner_normals(ugrt_ctx *ctx, const int *d_facelist, const float *d_vertlist, int num_faces,
					  float crease_cos, float *d_corner_normals)
{
	if (!ctx)
		return ugrt_fail(UGRT_EINVAL, "smooth_corner_normals: null ctx");
	if (num_faces < 0)
		return ugrt_fail(UGRT_EINVAL, "smooth_corner_normals: negative face count %d", num_faces);
	if (num_faces > 0 && (!d_facelist || !d_vertlist || !d_corner_normals))
		return ugrt_fail(UGRT_EINVAL, "smooth_corner_normals: null argument");
	if (crease_cos != crease_cos)
		return ugrt_fail(UGRT_EINVAL, "smooth_corner_normals: crease_cos is not a number");
	if (!ctx->sm_valid)
		return ugrt_fail(UGRT_EINVAL, "smooth_corner_normals: build the adjacency first (ugrt_smooth_adjacency)");
	if (num_faces != ctx->sm_faces)
		return ugrt_fail(UGRT_EINVAL, "smooth_corner_normals: %d faces, the adjacency was built for %d", num_faces, ctx->sm_faces);
	UGRT_HIP(hipSetDevice(ctx->device));
	const u32 F = (u32)num_faces, n = 3u * F;
	if (n) {
		if (int rc = ugrt_buf_reserve(ctx, ctx->sm_rec, (size_t)F * 32))
			return rc;
		const auto kernel = crease_cos <= -1.0f ? k_smooth_corners<SM_ALL>
							: (crease_cos > 1.0f ? k_smooth_corners<SM_OWN> : k_smooth_corners<SM_TEST>);
		ugrt_prof_begin(ctx, UGRT_ST_BUILD_FILL);
		hipLaunchKernelGGL(k_smooth_faces, dim3((F + SM_THREADS - 1) / SM_THREADS), dim3(SM_THREADS), 0, ctx->stream, d_facelist,
				   d_vertlist, F, (float4 *)ctx->sm_rec.p);
		hipLaunchKernelGGL(kernel, dim3((n + SM_THREADS - 1) / SM_THREADS), dim3(SM_THREADS), 0, ctx->stream,
				   (const u32 *)ctx->sm_val[1].p, (const u32 *)ctx->sm_key[1].p, (const u32 *)ctx->sm_start.p,
				   (const float4 *)ctx->sm_rec.p, n, crease_cos, d_corner_normals);
		ugrt_prof_end(ctx, UGRT_ST_BUILD_FILL);
		UGRT_HIP(hipGetLastError());
	}
	ctx->sm_normal_builds++;
	return UGRT_OK;
}

// One pixel of the band.  u and v are d_mt_core's (ugrt_dev.h), which keeps them to itself: the same operations in the
// same order from the camera and the stored direction; the containment tests are left out (u, v are not clamped).
__global__ __launch_bounds__(PX_THREADS) void k_smooth_normals(const float *__restrict__ t_value, const float *__restrict__ ray_dir,
							       const int *__restrict__ intersect_id, const float *__restrict__ cam_pos,
							       const float *__restrict__ verts, const int *__restrict__ tris,
							       const float *__restrict__ cn, const float *normal_in, int fold,
							       float *normal_out, int p0, int n)
{
	const int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const size_t p = (size_t)(p0 + i);
	const int id = intersect_id[p];
	const float t = t_value[p];
	if (id < 0 || !(t > 0.0f)) {
		const float a = normal_in[3 * p], b = normal_in[3 * p + 1], c = normal_in[3 * p + 2];
		normal_out[3 * p] = a;
		normal_out[3 * p + 1] = b;
		normal_out[3 * p + 2] = c;
		return;
	}
	float t9[9];
	d_stage_triangle(verts, tris, (u32)id, cam_pos[0], cam_pos[1], cam_pos[2], t9);
	const float tvec[3] = { t9[0], t9[1], t9[2] }, e1[3] = { t9[3], t9[4], t9[5] }, e2[3] = { t9[6], t9[7], t9[8] };
	const float dir[3] = { ray_dir[3 * p], ray_dir[3 * p + 1], ray_dir[3 * p + 2] };
	float pvec[3], qvec[3], ng[3], nn[3];
	D_CROSS(pvec, dir, e2);
	const float det = D_DOT(e1, pvec);
	const bool failed = det > -D_EPSILON && det < D_EPSILON;
	const float inv_det = d_recip_det(det);
	const float u = D_DOT(tvec, pvec) * inv_det;
	D_CROSS(qvec, tvec, e1);
	const float v = D_DOT(dir, qvec) * inv_det;
	const float w = (1.0f - u) - v;
	const float *c0 = cn + 9 * (size_t)id;
#pragma unroll
	for (int k = 0; k < 3; k++)
		nn[k] = (w * c0[k] + u * c0[3 + k]) + v * c0[6 + k];
	D_NORMALIZE(nn);
	D_CROSS(ng, e1, e2);
	D_NORMALIZE(ng);
	const bool keep = !failed && d_finite3(nn) && D_DOT(nn, ng) > 0.0f;
	// (three selects of values: a select between the two arrays would put both into scratch)
	float r0 = keep ? nn[0] : ng[0], r1 = keep ? nn[1] : ng[1], r2 = keep ? nn[2] : ng[2];
	if (fold) {
		r0 = r0 < 0 ? r0 * -1 : r0;
		r1 = r1 < 0 ? r1 * -1 : r1;
		r2 = r2 < 0 ? r2 * -1 : r2;
	}
	normal_out[3 * p] = r0;
	normal_out[3 * p + 1] = r1;
	normal_out[3 * p + 2] = r2;
}

extern "C" int ugrt_smooth_normals(ugrt_ctx *ctx, const float *d_t_value, const float *d_ray_dir, const int *d_intersect_id,
				   const float *d_cam_position, const float *d_vertlist, const int *d_trilist,
				   const float *d_corner_normals, const float *d_normal_in, int fold, float *d_normal_out)
{
	if (!ctx || !d_t_value || !d_ray_dir || !d_intersect_id || !d_cam_position || !d_vertlist || !d_trilist ||
	    !d_corner_normals || !d_normal_in || !d_normal_out)
		return ugrt_fail(UGRT_EINVAL, "smooth_normals: null argument");
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_smooth_normals, d_t_value, d_ray_dir, d_intersect_id, d_cam_position,
				  d_vertlist, d_trilist, d_corner_normals, d_normal_in, fold, d_normal_out);
}
