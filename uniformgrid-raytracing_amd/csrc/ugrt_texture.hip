// ugrt_texture.hip -- texture mapping: the mip atlas and the per-pixel albedo (not in the reference, which parses texture
// coordinates and a texture name and shades with Kd alone).  The normative text is ugrt.h's.
//
// ugrt_texture_set: level 0 of every texture packed on the host and copied in one piece, then one launch of k_texture_mips
// per further level over all textures that have it.  The atlas lies level-major -- all level 0, all level 1, ... -- so
// that a level's texels of all textures are one range of words and one launch.
// ugrt_texture_albedo: one thread per pixel.  The triangle is staged as k_smooth_normals stages it and serves three rays
// (the pixel's stored direction and the eye rays of its two neighbours, formed in the kernel); CROSS(tvec, e1) is the same
// for the three.  The tap loop runs N times per lane (N differs between neighbouring lanes: a wave takes its longest
// lane's trips); a trip issues the four -- or, between two levels, eight -- texel loads of its tap before the arithmetic.
// The table of levels is 16 bytes per (texture, level), read by one aligned load that the whole wave shares in the common
// case of one texture per wave.
// Arithmetic: DESIGN.md section 3 -- no contraction, D_CROSS / D_DOT of ugrt_dev.h.
#include "ugrt_dev.h"

#define TX_THREADS 256
#define TX_LEVELS UGRT_MAX_TEXTURE_LEVELS

// level `level` (>= 1) of every texture that has one: thread i writes word base + i of the atlas
__global__ __launch_bounds__(TX_THREADS) void k_texture_mips(const TexLevel *__restrict__ table, int count, int level, u32 base,
							      u32 total, u32 *words)
{
	const u32 i = blockIdx.x * TX_THREADS + threadIdx.x;
	if (i >= total)
		return;
	const u32 word = base + i;
	for (int t = 0; t < count; t++) {
		const TexLevel D = table[t * TX_LEVELS + level];
		if (D.levels == 0u || word < D.offset || word - D.offset >= D.w * D.h)
			continue;
		const TexLevel S = table[t * TX_LEVELS + level - 1];
		const u32 k = word - D.offset, y = k / D.w, x = k - y * D.w;
		const u32 xa = min(2u * x, S.w - 1u), xb = min(2u * x + 1u, S.w - 1u);
		const u32 ya = min(2u * y, S.h - 1u), yb = min(2u * y + 1u, S.h - 1u);
		const u32 *src = words + S.offset;
		const u32 a = src[ya * S.w + xa], b = src[ya * S.w + xb], c = src[yb * S.w + xa], d = src[yb * S.w + xb];
		u32 out = 0xFF000000u;
#pragma unroll
		for (int sh = 0; sh < 24; sh += 8)
			out |= (((a >> sh & 255u) + (b >> sh & 255u) + (c >> sh & 255u) + (d >> sh & 255u) + 2u) >> 2) << sh;
		words[word] = out;
		return;
	}
}

extern "C" int ugrt_texture_set(ugrt_ctx *ctx, int n, const int *wh, const unsigned char *const *rgb_host)
{
	if (!ctx)
		return ugrt_fail(UGRT_EINVAL, "texture_set: null ctx");
	if (n < 0 || n > UGRT_MAX_TEXTURES)
		return ugrt_fail(UGRT_EINVAL, "texture_set: n %d is not in 0..%d", n, UGRT_MAX_TEXTURES);
	if (n > 0 && (!wh || !rgb_host))
		return ugrt_fail(UGRT_EINVAL, "texture_set: null argument");
	size_t texels = 0;
	int max_levels = 0;
	std::vector<TexLevel> table((size_t)n * TX_LEVELS, TexLevel{ 0u, 0u, 0u, 0u });
	for (int t = 0; t < n; t++) {
		const int w = wh[2 * t], h = wh[2 * t + 1];
		if (w < 1 || w > UGRT_MAX_TEXTURE_DIM || h < 1 || h > UGRT_MAX_TEXTURE_DIM)
			return ugrt_fail(UGRT_EINVAL, "texture_set: texture %d is %d x %d, outside 1..%d", t, w, h, UGRT_MAX_TEXTURE_DIM);
		if (!rgb_host[t])
			return ugrt_fail(UGRT_EINVAL, "texture_set: null bytes of texture %d", t);
		texels += (size_t)w * (size_t)h;
		int levels = 1;
		for (int m = w > h ? w : h; m > 1; m >>= 1)
			levels++;
		u32 lw = (u32)w, lh = (u32)h;
		for (int l = 0; l < levels; l++) {
			table[(size_t)t * TX_LEVELS + l] = TexLevel{ lw, lh, 0u, (u32)levels };
			lw = lw > 1u ? lw >> 1 : 1u;
			lh = lh > 1u ? lh >> 1 : 1u;
		}
		max_levels = levels > max_levels ? levels : max_levels;
	}
	if (texels > (size_t)UGRT_MAX_TEXTURE_TEXELS)
		return ugrt_fail(UGRT_EINVAL, "texture_set: %zu texels exceed %u", texels, UGRT_MAX_TEXTURE_TEXELS);
	UGRT_HIP(hipSetDevice(ctx->device));
	// the copies of the call before read tx_stage and tx_levels: they are written again, or released, behind those copies
	// (a wait for that call's two copies, not for the device)
	if (ctx->tx_copied)
		UGRT_HIP(hipEventSynchronize(ctx->tx_copied));
	if (n == 0) {
		ctx->tx_count = 0;
		ctx->tx_levels.clear();
		std::vector<u32>().swap(ctx->tx_stage);
		// the device arrays go too, behind whatever the stream still reads them for (ugrt_texture_albedo reads neither
		// while the count is 0)
		if (ctx->tx_words.p || ctx->tx_table.p) {
			UGRT_HIP(hipStreamSynchronize(ctx->stream));
			if (ctx->tx_words.p)
				(void)hipFree(ctx->tx_words.p);
			if (ctx->tx_table.p)
				(void)hipFree(ctx->tx_table.p);
			ctx->tx_words = DevBuf();
			ctx->tx_table = DevBuf();
		}
		return UGRT_OK;
	}
	if (!ctx->tx_copied)
		UGRT_HIP(hipEventCreateWithFlags(&ctx->tx_copied, hipEventDisableTiming));
	// level-major offsets: base[l] = the first word of level l, base[max_levels] = the atlas' size (below 2^27)
	u32 base[TX_LEVELS + 1], at = 0u;
	for (int l = 0; l < max_levels; l++) {
		base[l] = at;
		for (int t = 0; t < n; t++) {
			TexLevel &L = table[(size_t)t * TX_LEVELS + l];
			if (L.levels) {
				L.offset = at;
				at += L.w * L.h;
			}
		}
	}
	base[max_levels] = at;
	int rc;
	ctx->tx_count = 0; // (a failure below leaves no atlas rather than a half-written one)
	if ((rc = ugrt_buf_reserve(ctx, ctx->tx_words, (size_t)at * 4)) ||
	    (rc = ugrt_buf_reserve(ctx, ctx->tx_table, table.size() * sizeof(TexLevel))))
		return rc;
	// (the packed level 0 and the table stay with the context until tx_copied has passed: the copies below may still read
	// them when the call returns)
	std::vector<u32> &level0 = ctx->tx_stage;
	level0.assign(texels, 0u);
	for (int t = 0; t < n; t++) {
		const TexLevel &L = table[(size_t)t * TX_LEVELS];
		const unsigned char *src = rgb_host[t];
		u32 *dst = level0.data() + L.offset;
		const size_t count = (size_t)L.w * L.h;
		for (size_t k = 0; k < count; k++)
			dst[k] = (u32)src[3 * k] | ((u32)src[3 * k + 1] << 8) | ((u32)src[3 * k + 2] << 16) | 0xFF000000u;
	}
	ctx->tx_levels.swap(table);
	UGRT_HIP(hipMemcpyAsync(ctx->tx_words.p, level0.data(), texels * 4, hipMemcpyHostToDevice, ctx->stream));
	UGRT_HIP(hipMemcpyAsync(ctx->tx_table.p, ctx->tx_levels.data(), ctx->tx_levels.size() * sizeof(TexLevel), hipMemcpyHostToDevice,
				ctx->stream));
	UGRT_HIP(hipEventRecord(ctx->tx_copied, ctx->stream));
	ugrt_prof_begin(ctx, UGRT_ST_BUILD_FILL);
	for (int l = 1; l < max_levels; l++) {
		const u32 total = base[l + 1] - base[l];
		hipLaunchKernelGGL(k_texture_mips, dim3((total + TX_THREADS - 1) / TX_THREADS), dim3(TX_THREADS), 0, ctx->stream,
				   (const TexLevel *)ctx->tx_table.p, n, l, base[l], total, (u32 *)ctx->tx_words.p);
	}
	ugrt_prof_end(ctx, UGRT_ST_BUILD_FILL);
	UGRT_HIP(hipGetLastError());
	ctx->tx_count = n;
	ctx->tx_builds++;
	return UGRT_OK;
}

extern "C" int ugrt_texture_get_level(ugrt_ctx *ctx, int tex, int level, int *width, int *height, const unsigned **d_words)
{
	if (!ctx || !width || !height || !d_words)
		return ugrt_fail(UGRT_EINVAL, "texture_get_level: null argument");
	if (tex < 0 || tex >= ctx->tx_count)
		return ugrt_fail(UGRT_EINVAL, "texture_get_level: texture %d of %d", tex, ctx->tx_count);
	if (level < 0 || level >= TX_LEVELS || ctx->tx_levels[(size_t)tex * TX_LEVELS + level].levels == 0u)
		return ugrt_fail(UGRT_EINVAL, "texture_get_level: texture %d has no level %d", tex, level);
	const TexLevel &L = ctx->tx_levels[(size_t)tex * TX_LEVELS + level];
	*width = (int)L.w;
	*height = (int)L.h;
	*d_words = (const unsigned *)ctx->tx_words.p + L.offset;
	return UGRT_OK;
}

// ---------------------------------------------------------------------------
// the per-pixel albedo
// ---------------------------------------------------------------------------
struct TexIn {
	const u32 *words;
	const TexLevel *table;
	int count;
};

// u, v of direction d on the staged triangle (k_smooth_normals' operations; qvec = CROSS(tvec, e1) is the caller's) and the
// uv they mix from the corners' {uv0, uv1, uv2}; false: the determinant failed
__device__ __forceinline__ bool d_ray_uv(const float *tvec, const float *e1, const float *e2, const float *qvec, const float *d,
					  const float *c, float *uv)
{
	float pvec[3];
	D_CROSS(pvec, d, e2);
	const float det = D_DOT(e1, pvec);
	const bool failed = det > -D_EPSILON && det < D_EPSILON;
	const float inv_det = d_recip_det(det);
	const float u = D_DOT(tvec, pvec) * inv_det;
	const float v = D_DOT(d, qvec) * inv_det;
	const float w = (1.0f - u) - v;
	uv[0] = (w * c[0] + u * c[2]) + v * c[4];
	uv[1] = (w * c[1] + u * c[3]) + v * c[5];
	return !failed;
}

// one axis of the bilinear footprint on n texels: the two indices and the weight of the second
__device__ __forceinline__ void d_tex_axis(float a, int n, int *i0, int *i1, float *f)
{
	const float a1 = a - __builtin_floorf(a);
	const float x = a1 * (float)n - 0.5f;
	const float x0 = __builtin_floorf(x);
	*f = x - x0;
	int c0 = ugrt_f2i(x0), c1 = (int)((u32)c0 + 1u);
	c0 = c0 < 0 ? c0 + n : c0;
	c0 = c0 >= n ? c0 - n : c0;
	c1 = c1 < 0 ? c1 + n : c1;
	c1 = c1 >= n ? c1 - n : c1;
	*i0 = (u32)c0 < (u32)n ? c0 : 0;
	*i1 = (u32)c1 < (u32)n ? c1 : 0;
}

struct TexTap { // the four texels of a bilinear fetch and its weights
	u32 t00, t10, t01, t11;
	float fx, fy;
};

__device__ __forceinline__ TexTap d_tex_fetch(const u32 *__restrict__ words, const TexLevel L, float a, float b)
{
	int x0, x1, y0, y1;
	TexTap r;
	d_tex_axis(a, (int)L.w, &x0, &x1, &r.fx);
	d_tex_axis(b, (int)L.h, &y0, &y1, &r.fy);
	const u32 *lv = words + L.offset;
	const u32 r0 = (u32)y0 * L.w, r1 = (u32)y1 * L.w;
	r.t00 = lv[r0 + (u32)x0];
	r.t10 = lv[r0 + (u32)x1];
	r.t01 = lv[r1 + (u32)x0];
	r.t11 = lv[r1 + (u32)x1];
	return r;
}

__device__ __forceinline__ float d_tex_mix(const TexTap &s, int shift)
{
	const float c00 = (float)(s.t00 >> shift & 255u), c10 = (float)(s.t10 >> shift & 255u);
	const float c01 = (float)(s.t01 >> shift & 255u), c11 = (float)(s.t11 >> shift & 255u);
	return (c00 * (1.0f - s.fx) + c10 * s.fx) * (1.0f - s.fy) + (c01 * (1.0f - s.fx) + c11 * s.fx) * s.fy;
}

__global__ __launch_bounds__(PX_THREADS) void k_texture_albedo(CamBlock cam, const float *__restrict__ nodes,
								const float *__restrict__ t_value, const float *__restrict__ ray_dir,
								const int *__restrict__ intersect_id, const float *__restrict__ cam_pos,
								const float *__restrict__ verts, const int *__restrict__ tris,
								const float *__restrict__ uvlist, int num_uvs,
								const int *__restrict__ uv_faces, const int *__restrict__ mat_idx,
								const float *__restrict__ mat_list, int mat_count,
								const int *__restrict__ mat_texture, TexIn tx, int max_aniso,
								float bias_scale, float *__restrict__ albedo, int p0, int n)
{
	const int i = blockIdx.x * PX_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const int pixel = p0 + i;
	const size_t p = (size_t)pixel;
	const int id = intersect_id[p];
	const float t = t_value[p];
	float out0 = 0.0f, out1 = 0.0f, out2 = 0.0f;
	int m = -1;
	if (id >= 0 && t > 0.0f) {
		m = mat_idx[id];
		m = m >= 0 && m < mat_count ? m : -1;
	}
	if (m >= 0) {
		out0 = mat_list[m * 6 + 3];
		out1 = mat_list[m * 6 + 4];
		out2 = mat_list[m * 6 + 5];
		const int T = mat_texture[m];
		const int i0 = uv_faces[3 * (size_t)id], i1 = uv_faces[3 * (size_t)id + 1], i2 = uv_faces[3 * (size_t)id + 2];
		const bool mapped = T >= 0 && T < tx.count && (u32)i0 < (u32)num_uvs && (u32)i1 < (u32)num_uvs && (u32)i2 < (u32)num_uvs;
		if (mapped) {
			float t9[9], qvec[3], uv[2], uvx[2], uvy[2], dn[3];
			const float c[6] = { uvlist[2 * (size_t)i0], uvlist[2 * (size_t)i0 + 1], uvlist[2 * (size_t)i1],
					     uvlist[2 * (size_t)i1 + 1], uvlist[2 * (size_t)i2], uvlist[2 * (size_t)i2 + 1] };
			d_stage_triangle(verts, tris, (u32)id, cam_pos[0], cam_pos[1], cam_pos[2], t9);
			const float *tvec = &t9[0], *e1 = &t9[3], *e2 = &t9[6];
			const float dir[3] = { ray_dir[3 * p], ray_dir[3 * p + 1], ray_dir[3 * p + 2] };
			D_CROSS(qvec, tvec, e1);
			const bool centre = d_ray_uv(tvec, e1, e2, qvec, dir, c, uv);
			if (centre && __builtin_fabsf(uv[0]) < __builtin_inff() && __builtin_fabsf(uv[1]) < __builtin_inff()) {
				const int row = pixel / cam.W, col = pixel - row * cam.W;
				d_ray_dir_at(cam, nodes, (float)(col + 1), (float)row, dn);
				bool wide = d_ray_uv(tvec, e1, e2, qvec, dn, c, uvx);
				d_ray_dir_at(cam, nodes, (float)col, (float)(row + 1), dn);
				wide = d_ray_uv(tvec, e1, e2, qvec, dn, c, uvy) && wide;
				const TexLevel *levels = tx.table + (size_t)T * TX_LEVELS;
				const TexLevel L0 = levels[0];
				const float W0 = (float)L0.w, H0 = (float)L0.h;
				const int last = (int)L0.levels - 1;
				const float dx0 = (uvx[0] - uv[0]) * W0, dx1 = (uvx[1] - uv[1]) * H0;
				const float dy0 = (uvy[0] - uv[0]) * W0, dy1 = (uvy[1] - uv[1]) * H0;
				const float Lx = __builtin_sqrtf(dx0 * dx0 + dx1 * dx1), Ly = __builtin_sqrtf(dy0 * dy0 + dy1 * dy1);
				const float LIM = (float)(2 * UGRT_MAX_TEXTURE_DIM * 16);
				wide = wide && Lx < LIM && Ly < LIM;
				const bool ymajor = Ly > Lx;
				float mj0 = ymajor ? dy0 : dx0, mj1 = ymajor ? dy1 : dx1;
				const float Lmax = ymajor ? Ly : Lx, Lmin = ymajor ? Lx : Ly;
				int N = 1, e = last;
				float f = 0.0f;
				if (wide) {
					// Lmin * n does not fall as n grows: the smallest n that reaches Lmax is one more than the n that do not
					for (int k = 1; k < max_aniso; k++)
						N += !(Lmin * (float)k >= Lmax) ? 1 : 0;
					const float lambda = (Lmax / (float)N) * bias_scale;
					e = 0;
					if (lambda > 1.0f) {
						const u32 bits = __float_as_uint(lambda);
						e = (int)(bits >> 23 & 255u) - 127;
						f = lambda / __uint_as_float(bits & 0x7F800000u) - 1.0f;
						if (e >= last) {
							e = last;
							f = 0.0f;
						}
					}
				} else {
					mj0 = 0.0f;
					mj1 = 0.0f;
				}
				const TexLevel LA = levels[e];
				const bool two = f != 0.0f;
				const TexLevel LB = levels[two ? e + 1 : e];
				const float twoN = (float)(2 * N);
				float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f;
				for (int k = 0; k < N; k++) {
					const float s = (float)(2 * k + 1) / twoN - 0.5f;
					const float a = uv[0] + (s * mj0) / W0, b = uv[1] + (s * mj1) / H0;
					const TexTap A = d_tex_fetch(tx.words, LA, a, b);
					float v0 = d_tex_mix(A, 0), v1 = d_tex_mix(A, 8), v2 = d_tex_mix(A, 16);
					if (two) {
						const TexTap B = d_tex_fetch(tx.words, LB, a, b);
						v0 = (1.0f - f) * v0 + f * d_tex_mix(B, 0);
						v1 = (1.0f - f) * v1 + f * d_tex_mix(B, 8);
						v2 = (1.0f - f) * v2 + f * d_tex_mix(B, 16);
					}
					acc0 = acc0 + v0;
					acc1 = acc1 + v1;
					acc2 = acc2 + v2;
				}
				const float fn = (float)N;
				out0 = out0 * ((acc0 / fn) / 255.0f);
				out1 = out1 * ((acc1 / fn) / 255.0f);
				out2 = out2 * ((acc2 / fn) / 255.0f);
			}
		}
	}
	albedo[3 * p] = out0;
	albedo[3 * p + 1] = out1;
	albedo[3 * p + 2] = out2;
}

extern "C" int ugrt_texture_albedo(ugrt_ctx *ctx, const float *d_t_value, const float *d_ray_dir, const int *d_intersect_id,
				   const float *d_cam_position, const float *d_vertlist, const int *d_facelist, const float *d_uvlist,
				   int num_uvs, const int *d_uv_facelist, const int *d_mat_idx, const float *d_mat_list,
				   int num_materials, const int *d_mat_texture, const int *mat_texture_host, int max_aniso,
				   int lod_bias, float *d_albedo)
{
	if (!ctx || !d_t_value || !d_ray_dir || !d_intersect_id || !d_cam_position || !d_vertlist || !d_facelist || !d_uv_facelist ||
	    !d_mat_idx || !d_mat_list || !d_mat_texture || !mat_texture_host || !d_albedo || (!d_uvlist && num_uvs > 0))
		return ugrt_fail(UGRT_EINVAL, "texture_albedo: null argument");
	if (num_uvs < 0 || num_materials < 0)
		return ugrt_fail(UGRT_EINVAL, "texture_albedo: negative count (%d uvs, %d materials)", num_uvs, num_materials);
	if (max_aniso < 1 || max_aniso > UGRT_MAX_TEXTURE_ANISO)
		return ugrt_fail(UGRT_EINVAL, "texture_albedo: max_aniso %d is not in 1..%d", max_aniso, UGRT_MAX_TEXTURE_ANISO);
	if (lod_bias < -16 || lod_bias > 16)
		return ugrt_fail(UGRT_EINVAL, "texture_albedo: lod_bias %d is not in -16..16", lod_bias);
	for (int m = 0; m < num_materials; m++)
		if (mat_texture_host[m] >= ctx->tx_count)
			return ugrt_fail(UGRT_EINVAL, "texture_albedo: material %d names texture %d, the atlas holds %d", m,
					 mat_texture_host[m], ctx->tx_count);
	const float bias_scale = lod_bias >= 0 ? (float)(1u << lod_bias) : 1.0f / (float)(1u << -lod_bias);
	UGRT_HIP(hipSetDevice(ctx->device));
	const TexIn tx = { (const u32 *)ctx->tx_words.p, (const TexLevel *)ctx->tx_table.p, ctx->tx_count };
	const float *nodes = ugrt_ctx_tex(ctx); // (stores the current camera's direction table first, if it is new)
	return ugrt_launch_pixels(ctx, UGRT_ST_SHADE, k_texture_albedo, ctx->cam, nodes, d_t_value, d_ray_dir, d_intersect_id,
				  d_cam_position, d_vertlist, d_facelist, d_uvlist, num_uvs, d_uv_facelist, d_mat_idx, d_mat_list,
				  num_materials, d_mat_texture, tx, max_aniso, bias_scale, d_albedo);
}
