// ugrt_fresnel.hip -- Fresnel glass: a reflected and a transmitted ray per glass hit, the whole ray tree of a pixel in one
// launch (not in the reference).
//
// Spec: an active pixel p of ugrt_refract_rays' level-1 rays is the root of a tree of depth D.  A node is a ray {o, d} with
// a weight w and a hit; a mirror hit has one child (d_reflect_ray, w*k), a glass hit past the critical angle one
// (d_refract_ray's mirrored ray, w*k), any other glass hit two: child 0 d_refract_ray's transmitted ray with (w*k)*(1 - F),
// child 1 d_reflect_ray's ray with (w*k)*F, F = scale * Schlick's share.  A child is followed where its weight is above
// min_weight.  A node that goes on (its level below D, a child followed) adds (w*(1 - k))*L, any other w*L, L the level's
// clamped Lambert colour, a third of it where the shadow light is hidden.
//   * 2^D neighbouring lanes are the leaves of one pixel's tree: lane bit j is the child taken at level j's split.  The node
//     of prefix (b_0 .. b_{j-1}) is walked once, by the lane whose remaining bits are 0 (its owner); t and id go to the
//     other lanes of the prefix by a lane shuffle, and every lane forms its own child from its own bit;
//   * every lane of the wave calls the walks at every level (they are cooperative); a lane without a node serves the rounds;
//   * the owner adds its nodes' terms front to back from +0; the leaves' sums are added pairwise from the deepest bit up
//     (step j: leaf b < 2^j takes leaf b + 2^j) and leaf 0 stores the pixel's 16 bytes.  No atomics on the sums;
//   * the words that only the code between the walks reads (the material arrays, the primary arrays, the view rotation,
//     the lights) are staged in LDS (ugrt_gather.h's reason: kept in scalar registers over both walks they spill);
//   * groups of pixels are drawn from a ticket.
// ugrt_fresnel_shade (ugrt_shade.hip) turns the sums into the image's bytes.
#include "ugrt_gather.h" // (gather_launch, d_ticket_draw)

struct FresnelArg {
	const float *t_value, *ray_dir, *normal; // the primary hits
	const int *ids;                          // their triangles (no shading call has run yet)
	const float *cam_pos;
	const int *mat_idx;
	const float *mat_list, *reflect, *transmit, *ior;
	int mat_count;
	int depth;
	float scale, min_weight;
	float light[3]; // the shadow light (SHADOW only)
	float eps;
};

// The Fresnel share of a glass hit (o, d, t, tri) of index ior_m: nn, dn, front, u, c, ior, eta and k2 are d_refract_ray's,
// operation for operation.  False past the critical angle (k2 < 0: no split); else *F = scale * Schlick's approximation at
// the cosine on the air side.
__device__ __forceinline__ bool d_fresnel_share(const float *o, const float *d, float t, const float *tri, float ior_m,
						float scale, float *F)
{
	float nn[3], P[3], dn;
	bool front;
	D_HIT_FRAME_SIDED(o, d, t, tri, P, nn, dn, front);
	(void)P;
	(void)dn;
	float u[3] = { d[0], d[1], d[2] };
	D_NORMALIZE(u);
	const float c = -D_DOT(u, nn);
	const float ior = ior_m > 0 ? ior_m : 1.0f;
	const float eta = front ? 1.0f / ior : ior;
	const float k2 = 1.0f - (eta * eta) * (1.0f - c * c);
	if (k2 < 0)
		return false;
	const float q = (1.0f - ior) / (1.0f + ior);
	const float r0 = q * q;
	const float cs = front ? c : __builtin_sqrtf(k2);
	const float x = 1.0f - cs;
	*F = scale * (r0 + (1.0f - r0) * (((x * x) * (x * x)) * x));
	return true;
}

// what the code between the walks reads, staged in LDS by lane 0
struct FresnelLate {
	FresnelArg a;
	float cc[12];   // cam.cc[16..27]: d_lambert reads the rotation and the light, nothing else
	float light[3]; // the context's light
	const float *rays;
	float *acc_out;
	u32 *ticket;
};

// `acc` of the band was cleared in stream order before the launch: only the words of active pixels are written
template <bool REC, bool SHADOW>
__global__ __launch_bounds__(64) void k_fresnel_gather(DGrid g, const u32 *__restrict__ value_list, const u32 *__restrict__ span,
						       const u32 *__restrict__ offset, const u32 *__restrict__ bitmap,
						       const float *__restrict__ verts, const int *__restrict__ tris,
						       const float4 *__restrict__ rec, const float *__restrict__ rays,
						       const u32 *__restrict__ list, const u32 *__restrict__ count_p, u32 PPW,
						       u32 COOP, const FresnelArg a, const CamBlock cam, float *__restrict__ acc_out,
						       u32 *__restrict__ ticket, unsigned long long *__restrict__ nodes)
{
	__shared__ FresnelLate s_late;
	const int lane = threadIdx.x;
	const u32 count = *count_p;
	const int D = a.depth;
	if (lane == 0) {
		s_late.a = a;
#pragma unroll
		for (int i = 0; i < 12; i++)
			s_late.cc[i] = cam.cc[16 + i];
#pragma unroll
		for (int k = 0; k < 3; k++)
			s_late.light[k] = cam.light[k];
		s_late.rays = rays;
		s_late.acc_out = acc_out;
		s_late.ticket = ticket;
	}
	__syncthreads();
	const u32 b = (u32)lane & ((1u << D) - 1u), apix = (u32)lane >> D;
	const int first = lane & ~((1 << D) - 1); // the pixel's leaf 0
	u32 walked = 0u;
	// groups of PPW pixels, the first gridDim.x by workgroup id, the others drawn from the ticket
	for (u32 grp = blockIdx.x; grp * PPW < count;) {
		// (the staged words are read where they are used: an offset the compiler cannot see through keeps their loads
		// from being hoisted over the walks, into registers that live as long as the kernel)
		u32 late_at = 0u;
		asm volatile("" : "+v"(late_at));
		const FresnelLate &S0 = *(const FresnelLate *)((const char *)&s_late + late_at);
		const u32 slot = grp * PPW + apix;
		bool inb = apix < PPW && slot < count;
		const int p = inb ? (int)list[slot] : 0;
		inb = inb && p != -1; // (padding: k_dda_prepare)
		// the lane's node: the root {cam, dir} with the primary hit, then the node of its prefix at every level
		float o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 }, w = 1.0f, ht = -1.0f;
		float acc[3] = { 0.0f, 0.0f, 0.0f };
		int hid = -2;
		bool alive = inb;
		if (inb) {
#pragma unroll
			for (int k = 0; k < 3; k++) {
				o[k] = S0.a.cam_pos[k];
				d[k] = S0.a.ray_dir[p * 3 + k];
			}
			ht = S0.a.t_value[p];
			hid = S0.a.ids[p];
		}
		for (int j = 0;; j++) {
			const bool owner = alive && (b >> j) == 0u;
			if (j > 0) {
				// ---- level j's nodes: the closest hit, walked by the owner, handed to the lanes of the prefix ----
				float res_t;
				int res_id;
				d_closest_walk<REC, false>(g, value_list, span, offset, bitmap, verts, tris, rec, o, d, 0.0f, owner, COOP, lane,
							   res_t, res_id);
				walked += (u32)__popcll(__ballot(owner));
				const int src = first | (int)(b & ((1u << j) - 1u));
				ht = __shfl(res_t, src);
				hid = __shfl(res_id, src);
			}
			// ---- the node: its material, its children and their weights; the owner's colour and occlusion ray ----
			asm volatile("" : "+v"(late_at));
			const FresnelLate &S = *(const FresnelLate *)((const char *)&s_late + late_at);
			int m = -1;
			if (alive && hid >= 0) {
				m = S.a.mat_idx[hid];
				m = m >= 0 && m < S.a.mat_count ? m : -1;
			}
			float L[3] = { 0.0f, 0.0f, 0.0f }, o2[3] = { 0.0f, 0.0f, 0.0f }, d2[3] = { 0.0f, 0.0f, 0.0f };
			float kw = 0.0f, w0 = 0.0f, w1 = 0.0f, c0[6] = { 0, 0, 0, 0, 0, 0 }, c1[6] = { 0, 0, 0, 0, 0, 0 };
			bool f0 = false, f1 = false;
			if (m >= 0) {
				float t9[9];
				d_stage_triangle(verts, tris, (u32)hid, 0.0f, 0.0f, 0.0f, t9);
				const float kt = S.a.transmit[m], kr = S.a.reflect[m];
				kw = kt > 0 ? kt : kr;
				const float wk = w * kw;
				bool two = false;
				if (j < D) {
					if (kt > 0) {
						float F;
						two = d_fresnel_share(o, d, ht, t9, S.a.ior[m], S.a.scale, &F);
						d_refract_ray(o, d, ht, t9, S.a.eps, kt, S.a.ior[m], c0);
						if (two) {
							d_reflect_ray(o, d, ht, t9, S.a.eps, c1);
							w0 = wk * (1.0f - F);
							w1 = wk * F;
						} else {
							w0 = wk;
						}
					} else if (kr > 0) {
						d_reflect_ray(o, d, ht, t9, S.a.eps, c0);
						w0 = wk;
					}
					if (j == 0) { // (child 0 of the root: the level-1 ray the caller made)
#pragma unroll
						for (int k = 0; k < 6; k++)
							c0[k] = S.rays[p * 6 + k];
					}
					f0 = w0 > S.a.min_weight;
					f1 = two && w1 > S.a.min_weight;
				}
				if (owner) {
					if constexpr (SHADOW) {
						if (j > 0) { // k_occlusion_rays' ray: d_reflect_ray's origin, the direction light - o'' not normalised
							float out[6];
							d_reflect_ray(o, d, ht, t9, S.a.eps, out);
#pragma unroll
							for (int k = 0; k < 3; k++) {
								o2[k] = out[k];
								d2[k] = S.a.light[k] - out[k];
							}
						}
					}
					CamBlock view; // (d_lambert reads the rotation and the light, nothing else)
#pragma unroll
					for (int i = 0; i < 12; i++)
						view.cc[16 + i] = S.cc[i];
#pragma unroll
					for (int k = 0; k < 3; k++)
						view.light[k] = S.light[k];
					if (j > 0) {
						d_hit_color(view, o, d, ht, t9, S.a.mat_list, m, L);
					} else if (ht > 0) { // the root: the stored normal, as k_shade_reflect_depth shades the primary hit
						float hmat[6], hp[3], nrm[3];
#pragma unroll
						for (int k = 0; k < 3; k++) {
							hp[k] = o[k] + ht * d[k];
							nrm[k] = S.a.normal[p * 3 + k];
						}
						d_material_kd(S.a.mat_list, m, hmat);
						d_lambert<false>(view, hp, nrm, L, hmat, 1.0f);
						d_clamp1(L);
					}
				}
			}
			// ---- is the shadow light hidden from the hit (the any-hit walk that sees through glass, the light at t = 1) ----
			if constexpr (SHADOW) {
				if (j > 0) {
					const WalkThru thru = { S.a.mat_idx, S.a.transmit, S.a.mat_count };
					const bool occ = d_any_walk<REC, true>(g, value_list, span, offset, bitmap, verts, tris, rec, o2, d2, 1.0f,
									       owner && m >= 0, COOP, lane, &thru);
					if (occ) {
#pragma unroll
						for (int k = 0; k < 3; k++)
							L[k] = L[k] / 3.0f;
					}
				}
			}
			// ---- the owner's term (k_shade_reflect_depth's two statements), then the lane's child ----
			const bool goes_on = f0 || f1;
			if (owner) {
				if (goes_on) {
#pragma unroll
					for (int k = 0; k < 3; k++)
						acc[k] = acc[k] + (w * (1.0f - kw)) * L[k];
				} else {
#pragma unroll
					for (int k = 0; k < 3; k++)
						acc[k] = acc[k] + w * L[k];
				}
			}
			const bool second = ((b >> j) & 1u) != 0u;
			alive = alive && (second ? f1 : f0);
			w = second ? w1 : w0;
#pragma unroll
			for (int k = 0; k < 3; k++) {
				o[k] = second ? c1[k] : c0[k];
				d[k] = second ? c1[3 + k] : c0[3 + k];
			}
			if (j >= D || __ballot(alive) == 0ull)
				break;
		}
		// ---- the leaves' sums, pairwise from the deepest bit up (dead leaves and idle lanes hold +0) ----
		for (int j = D - 1; j >= 0; j--) {
#pragma unroll
			for (int k = 0; k < 3; k++)
				acc[k] = acc[k] + __shfl_down(acc[k], 1u << j);
		}
		if (inb && b == 0u)
			*(float4 *)(S0.acc_out + 4u * (size_t)p) = make_float4(acc[0], acc[1], acc[2], 1.0f);
		grp = d_ticket_draw(lane, grp, S0.ticket);
	}
	if (lane == 0 && walked != 0u)
		atomicAdd(nodes, (unsigned long long)walked);
}

extern "C" int ugrt_fresnel_gather(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span, const unsigned *d_offset,
				   const float *d_vertlist, const int *d_trilist, const float *d_rays, const int *d_active,
				   const float *d_normal, const float *d_t_value, const float *d_ray_dir, const int *d_intersect_id,
				   const float *d_cam_position, const int *d_mat_idx, const float *d_mat_list, const float *d_reflect,
				   const float *d_transmit, const float *d_ior, int num_materials, int depth, float scale,
				   float min_weight, const float *shadow_light, float eps, float *d_acc)
{
	if (!ctx || !d_value_list || !d_span || !d_offset || !d_vertlist || !d_trilist || !d_rays || !d_active || !d_normal ||
	    !d_t_value || !d_ray_dir || !d_intersect_id || !d_cam_position || !d_mat_idx || !d_mat_list || !d_reflect ||
	    !d_transmit || !d_ior || !d_acc)
		return ugrt_fail(UGRT_EINVAL, "fresnel_gather: null argument");
	if (depth < 1 || depth > UGRT_MAX_FRESNEL_DEPTH)
		return ugrt_fail(UGRT_EINVAL, "fresnel_gather: depth %d is not in 1..%d", depth, UGRT_MAX_FRESNEL_DEPTH);
	if (!(scale >= 0.0f && scale <= 1.0f))
		return ugrt_fail(UGRT_EINVAL, "fresnel_gather: scale must lie in [0, 1]");
	if (!(min_weight >= 0.0f))
		return ugrt_fail(UGRT_EINVAL, "fresnel_gather: min_weight must not be negative");
	if (eps != eps)
		return ugrt_fail(UGRT_EINVAL, "fresnel_gather: eps is not a number");
	if (num_materials < 1)
		return ugrt_fail(UGRT_EINVAL, "fresnel_gather: num_materials %d is less than 1", num_materials);
	if (((size_t)d_acc & 15u) != 0u)
		return ugrt_fail(UGRT_EINVAL, "fresnel_gather: d_acc is not 16-byte aligned");
	FresnelArg a = {};
	a.t_value = d_t_value;
	a.ray_dir = d_ray_dir;
	a.normal = d_normal;
	a.ids = d_intersect_id;
	a.cam_pos = d_cam_position;
	a.mat_idx = d_mat_idx;
	a.mat_list = d_mat_list;
	a.reflect = d_reflect;
	a.transmit = d_transmit;
	a.ior = d_ior;
	a.mat_count = num_materials;
	a.depth = depth;
	a.scale = scale;
	a.min_weight = min_weight;
	for (int k = 0; k < 3; k++)
		a.light[k] = shadow_light ? shadow_light[k] : 0.0f;
	a.eps = eps;
	// a pixel takes 2^depth lanes; the node counter is cleared with the band
	static const GatherKernel<FresnelArg, CamBlock, float *, u32 *, unsigned long long *> kernel[2][2] = {
		{ k_fresnel_gather<false, false>, k_fresnel_gather<false, true> },
		{ k_fresnel_gather<true, false>, k_fresnel_gather<true, true> },
	};
	unsigned long long *nodes = (unsigned long long *)(ctx->d_small + UGRT_DSMALL_FRESNEL);
	if (int rc = gather_launch({ ctx, d_value_list, d_span, d_offset, d_vertlist, d_trilist, d_rays, d_active, d_acc }, 1u << depth, 0,
				   kernel, shadow_light != nullptr, nodes, a, ctx->cam, d_acc, ctx->d_small + UGRT_DSMALL_TICKET, nodes))
		return rc;
	ctx->fresnel_gathers++;
	return UGRT_OK;
}
