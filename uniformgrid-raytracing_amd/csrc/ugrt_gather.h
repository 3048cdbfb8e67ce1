// ugrt_gather.h -- the pixel-major gather, written once: a pixel's S rays in neighbouring lanes of one wave, each ray's
// closest hit, the hit's colour, its occlusion ray to the shadow light, and the pixel's byte sums in one 16-byte store
// (ugrt_gi.hip, ugrt_glossy.hip, ugrt_aa.hip: DESIGN.md sections 6.10, 6.13, 6.11).  What differs between the three is a
// `Kind`, a policy struct in the style of ugrt_dda_any.hip's aims:
//   * Arg: its by-value block.  It starts with GatherArg (the table and the tile of sets) and holds `late`, a Kind::Late;
//   * entry: floats per table entry; radius: d_closest_walk's RADIUS; extra and stage(): LDS floats between the table
//     and the staged words, and their copy;
//   * ray(): {o, d} of a lane; shade(): what {o, d, t, id} becomes -- a Kind::Colour, the occlusion ray and whether the
//     hit has a colour at all; darken(): the packed bytes of that colour, a third of it where the light is hidden.
// The index space is ugrt_trace_dda_any_area's (pixel group, sample); the two walks are ugrt_walks.h's.  The host half,
// gather_launch, also serves ugrt_fresnel.hip, whose kernel is a tree and its own.
#ifndef UGRT_GATHER_H
#define UGRT_GATHER_H

#include "ugrt_walks.h"

// (dynamic LDS, its base 16-byte aligned: the table, padded to four floats; Kind::extra floats; the Kind's Late)
extern __shared__ __attribute__((aligned(16))) float s_gather[];

// A table of `total` floats in LDS: float4 per lane while four are left (a 16-byte aligned table), then single floats.
// The caller synchronises.
__device__ __forceinline__ void d_stage_table(float *lds, const float *src, u32 total, int lane)
{
	u32 done = 0u;
	if (((size_t)src & 15u) == 0u) {
		for (u32 i = 4u * (u32)lane; i + 4u <= total; i += 256u)
			*(float4 *)(lds + i) = *(const float4 *)(src + i);
		done = total & ~3u;
	}
	for (u32 i = done + (u32)lane; i < total; i += 64u)
		lds[i] = src[i];
}

// the next group of a persistent wave: the first gridDim.x go by workgroup id, the others are drawn from the ticket
__device__ __forceinline__ u32 d_ticket_draw(int lane, u32 grp, u32 *ticket)
{
	if (lane == 0)
		grp = gridDim.x + atomicAdd(ticket, 1u);
	return (u32)__builtin_amdgcn_readfirstlane((int)grp);
}

// Which pixel p = (x, y) of the ray list and which table entry a lane serves in group grp: slot grp * PPW + lane / S,
// entry k(p) * S + lane % S of set k(p) = (y % set_h) * set_w + x % set_w.  False: an idle lane, a slot behind the list
// or padding (k_dda_prepare's -1); p is 0 then.
// (the divisors are made opaque here: their reciprocals are formed per group, not kept over the walks)
__device__ __forceinline__ bool d_gather_lane(int lane, u32 S, u32 grp, u32 PPW, u32 count, const u32 *__restrict__ list,
					      u32 width, u32 set_w, u32 set_h, int &p, u32 &x, u32 &y, u32 &entry)
{
	u32 apix;
	d_area_lane(lane, S, apix, entry);
	const u32 slot = grp * PPW + apix;
	bool inb = apix < PPW && slot < count;
	p = inb ? (int)list[slot] : 0;
	inb = inb && p != -1;
	asm volatile("" : "+s"(width), "+s"(set_w), "+s"(set_h));
	y = (u32)p / width;
	x = (u32)p - y * width;
	entry += ((y % set_h) * set_w + x % set_w) * S;
	return inb;
}

// The sums of rg = r | g << 16 and bb = b over a pixel's S neighbouring lanes (idle and padding lanes hold zeros; a sum
// is at most 32 * 255 < 2^13), stored with the count word by the pixel's first lane.
__device__ __forceinline__ void d_gather_store(int lane, u32 S, u32 rg, u32 bb, bool inb, int p, u32 *sum)
{
	u32 apix, asmp;
	d_area_lane(lane, S, apix, asmp);
	// lane i of a pixel holds the sum over its lanes i .. min(i + 2 * off - 1, S - 1) after the step with `off`
	for (u32 off = 1u; off < S; off <<= 1) {
		const u32 org = (u32)__shfl_down((int)rg, off), obb = (u32)__shfl_down((int)bb, off);
		if (asmp + off < S) {
			rg += org;
			bb += obb;
		}
	}
	if (inb && asmp == 0u)
		*(uint4 *)(sum + 4u * (size_t)p) = make_uint4(rg & 0xFFFFu, rg >> 16, bb, 1u);
}

// what every Kind::Arg starts with: read in front of the first walk and by the walks
struct GatherArg {
	const float *table; // device memory [set_w * set_h][S][Kind::entry]
	int count;          // S
	u32 set_w, set_h;   // 1..4 each
	u32 width;          // of the full image
	float radius;       // (Kind::radius only)
};

// What only the code around the walks reads.  Lane 0 stages it in LDS behind the table and it is read from there where
// it is used: kept in scalar registers over both walks these words cost 12 to 23 spilled ones.  A Kind::Late is this or
// derives from it.
struct GatherLate {
	const int *mat_idx;
	const float *mat_list;
	u32 *sum, *ticket;
	float view[12];  // the context's current block, cc[16..27], and its light: what d_lambert reads
	float clight[3];
	float light[3];  // the shadow light (SHADOW only)
	float eps;
	int mat_count;
};

static inline GatherLate gather_late_of(const ugrt_ctx *ctx, const int *d_mat_idx, const float *d_mat_list, int num_materials,
					const float *shadow_light, float eps, unsigned *d_sum)
{
	GatherLate l = {};
	l.mat_idx = d_mat_idx;
	l.mat_list = d_mat_list;
	l.sum = d_sum;
	l.ticket = ctx->d_small + UGRT_DSMALL_TICKET;
	for (int k = 0; k < 12; k++)
		l.view[k] = ctx->cam.cc[16 + k];
	for (int k = 0; k < 3; k++) {
		l.clight[k] = ctx->cam.light[k];
		l.light[k] = shadow_light ? shadow_light[k] : 0.0f;
	}
	l.eps = eps;
	l.mat_count = num_materials;
	return l;
}

// (d_lambert reads the rotation and the light, nothing else)
__device__ __forceinline__ void d_gather_view(const GatherLate &late, CamBlock &view)
{
#pragma unroll
	for (int i = 0; i < 12; i++)
		view.cc[16 + i] = late.view[i];
#pragma unroll
	for (int k = 0; k < 3; k++)
		view.light[k] = late.clight[k];
}

// k_occlusion_rays' ray from the hit (o, d, t) on the staged triangle t9: d_reflect_ray's origin, the direction
// light - o'' not normalised
__device__ __forceinline__ void d_gather_occlusion_ray(const GatherLate &late, const float *o, const float *d, float t,
						       const float *t9, float *o2, float *d2)
{
	float out[6];
	d_reflect_ray(o, d, t, t9, late.eps, out);
#pragma unroll
	for (int k = 0; k < 3; k++) {
		o2[k] = out[k];
		d2[k] = late.light[k] - out[k];
	}
}

// What ugrt_gi.hip and ugrt_glossy.hip share: no LDS of their own, and the hit shaded as a level's hit is shaded
// (d_hit_color), a third of the float colour where the light is hidden, then d_to_u8.
struct GatherLevelShade {
	static constexpr bool radius = true;
	static constexpr u32 extra = 0u;
	struct Colour {
		float L[3];
	};
	template <class Arg> static __device__ __forceinline__ void stage(float *, const Arg &, int)
	{
	}
	// false: a miss or a material out of range, which stay 0, occluded or not
	template <bool SHADOW>
	static __device__ __forceinline__ bool shade(const GatherLate &late, const float *__restrict__ verts,
						     const int *__restrict__ tris, const float *o, const float *d, float res_t,
						     int res_id, Colour &c, float *o2, float *d2)
	{
		if (res_id < 0)
			return false;
		const int hm = late.mat_idx[res_id];
		if (!(hm >= 0 && hm < late.mat_count))
			return false;
		float t9[9];
		d_stage_triangle(verts, tris, (u32)res_id, 0.0f, 0.0f, 0.0f, t9);
		if constexpr (SHADOW)
			d_gather_occlusion_ray(late, o, d, res_t, t9, o2, d2);
		CamBlock view;
		d_gather_view(late, view);
		d_hit_color(view, o, d, res_t, t9, late.mat_list, hm, c.L);
		return true;
	}
	static __device__ __forceinline__ void darken(Colour &c, bool occ, bool lit_hit, u32 &rg, u32 &bb)
	{
		if (occ) {
#pragma unroll
			for (int k = 0; k < 3; k++)
				c.L[k] = c.L[k] / 3.0f;
		}
		rg = bb = 0u;
		if (lit_hit) {
			rg = (u32)d_to_u8(c.L[0]) | ((u32)d_to_u8(c.L[1]) << 16);
			bb = (u32)d_to_u8(c.L[2]);
		}
	}
};

// `sum` of the band was cleared in stream order before the launch: only the words of the list's pixels are written
template <bool REC, bool SHADOW, class Kind>
__global__ __launch_bounds__(64) void k_pixel_gather(DGrid g, const u32 *__restrict__ value_list, const u32 *__restrict__ span,
						     const u32 *__restrict__ offset, const u32 *__restrict__ bitmap,
						     const float *__restrict__ verts, const int *__restrict__ tris,
						     const float4 *__restrict__ rec, const float *__restrict__ rays,
						     const u32 *__restrict__ list, const u32 *__restrict__ count_p, u32 PPW, u32 COOP,
						     const typename Kind::Arg a)
{
	const int lane = threadIdx.x;
	const u32 count = *count_p;
	const u32 S = (u32)a.count;
	const u32 total = Kind::entry * S * a.set_w * a.set_h;
	const float *more = s_gather + ((total + 3u) & ~3u);
	const typename Kind::Late &late = *(const typename Kind::Late *)(more + Kind::extra);
	d_stage_table(s_gather, a.table, total, lane);
	Kind::stage((float *)more, a, lane);
	if (lane == 0)
		*(typename Kind::Late *)(more + Kind::extra) = a.late;
	__syncthreads();
	for (u32 grp = blockIdx.x; grp * PPW < count; grp = d_ticket_draw(lane, grp, late.ticket)) {
		int p;
		u32 x, y, entry;
		const bool inb = d_gather_lane(lane, S, grp, PPW, count, list, a.width, a.set_w, a.set_h, p, x, y, entry);
		// ---- phase A: the closest hit of the lane's ray (k_trace_dda_ray's loop) ----
		float o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 }, res_t;
		int res_id;
		if (inb)
			Kind::ray(late, s_gather + Kind::entry * entry, more, rays, p, x, y, o, d);
		d_closest_walk<REC, Kind::radius>(g, value_list, span, offset, bitmap, verts, tris, rec, o, d,
						  Kind::radius ? a.radius : 0.0f, inb, COOP, lane, res_t, res_id);
		// ---- the hit's colour and its occlusion ray, formed here so that phase B holds neither o nor d ----
		typename Kind::Colour c = {};
		float o2[3] = { 0.0f, 0.0f, 0.0f }, d2[3] = { 0.0f, 0.0f, 0.0f };
		const bool lit_hit = Kind::template shade<SHADOW>(late, verts, tris, o, d, res_t, res_id, c, o2, d2);
		// ---- phase B: is the shadow light hidden from the hit (k_trace_dda_any's loop, the light at t = 1) ----
		bool occ = false;
		if constexpr (SHADOW)
			occ = d_any_walk<REC>(g, value_list, span, offset, bitmap, verts, tris, rec, o2, d2, 1.0f, lit_hit, COOP, lane);
		u32 rg, bb;
		Kind::darken(c, occ, lit_hit, rg, bb);
		d_gather_store(lane, S, rg, bb, inb, p, late.sum);
	}
}

// ---------------------------------------------------------------------------
// the host side: one path for every gather.  An export checks its arguments, fills its Arg and calls this.
// ---------------------------------------------------------------------------
// what every export is given; band: the 16 bytes per pixel the kernel stores
struct GatherCall {
	ugrt_ctx *ctx;
	const unsigned *value_list, *span, *offset;
	const float *verts;
	const int *tris;
	const float *rays;
	const int *active;
	void *band;
};

// a gather kernel's arguments: the grid, the scene, the ray list, the launch shape, the gather's block, its own
template <class Arg, class... More>
using GatherKernel = void (*)(DGrid, const u32 *, const u32 *, const u32 *, const u32 *, const float *, const int *,
			      const float4 *, const float *, const u32 *, const u32 *, u32, u32, Arg, More...);

// The prepare launch and kernel[rec][shadow] for a gather whose pixels take `lanes` lanes each.
//   * the launch shape (ugrt_ctx_set_option; no effect on results) is ugrt_trace_dda_any_area's: L = "any_rays_per_wave"
//     of a wave's lanes (at most and unset: all 64), PPW = max(1, L / lanes) pixels per group, "dda_blocks" caps the waves;
//   * one prepare launch and one ray list, in the form that writes no hit defaults, with the bitmap workgroups and without
//     the split walks' chunk table.  That form clears one int per pixel of the band at [pixel]; the band's words here lie
//     at [4 * pixel .. 4 * pixel + 3], so it is handed the band's own words to write into (band + 3 * p0 + pixel lies
//     inside them for every pixel of the band) and the whole band is cleared behind it, in stream order;
//   * nodes, where not null, is a 64-bit counter cleared with the band.
template <class Arg, class... More>
static int gather_launch(const GatherCall &c, u32 lanes, size_t lds, const GatherKernel<Arg, More...> (&kernel)[2][2],
			 bool shadow, unsigned long long *nodes, const Arg &a, More... more)
{
	ugrt_ctx *ctx = c.ctx;
	Grid &G = ctx->grid[UGRT_GRID_UNIFORM];
	if (!G.valid)
		return ugrt_fail(UGRT_EINVAL, "trace_dda: build the uniform grid first (it defines the cell geometry)");
	UGRT_HIP(hipSetDevice(ctx->device));
	const DGrid g = ugrt_dgrid_of(G);
	const float4 *rec = ugrt_trirec_of(ctx, c.verts, c.tris);
	const u32 L = ctx->opt[UGRT_OPT_ANY_RPW] > 0 ? (ctx->opt[UGRT_OPT_ANY_RPW] < 64 ? (u32)ctx->opt[UGRT_OPT_ANY_RPW] : 64u) : 64u;
	const u32 PPW = L / lanes > 0u ? L / lanes : 1u;
	const u32 COOP = ctx->opt[UGRT_OPT_ANY_COOP] > 0 ? (u32)ctx->opt[UGRT_OPT_ANY_COOP] : 8u;
	u32 *list, *dcount;
	ugrt_prof_begin(ctx, UGRT_ST_WORKLIST);
	const int rc = ugrt_dda_prepare(ctx, g, c.active, nullptr, (int *)c.band + (size_t)3 * (size_t)ctx->p0, c.span, true, nullptr,
					&list, &dcount);
	hipError_t he = hipSuccess;
	if (!rc)
		he = hipMemsetAsync((u32 *)c.band + (size_t)4 * (size_t)ctx->p0, 0, (size_t)ctx->npix * 16u, ctx->stream);
	if (!rc && he == hipSuccess && nodes)
		he = hipMemsetAsync(nodes, 0, 8, ctx->stream);
	ugrt_prof_end(ctx, UGRT_ST_WORKLIST);
	if (rc)
		return rc;
	UGRT_HIP(he);
	int blocks = launch_blocks_for((u32)ctx->npix / PPW + 1u);
	if (ctx->opt[UGRT_OPT_DDA_BLOCKS] > 0 && blocks > ctx->opt[UGRT_OPT_DDA_BLOCKS])
		blocks = ctx->opt[UGRT_OPT_DDA_BLOCKS];
	ugrt_prof_begin(ctx, UGRT_ST_TRACE_DDA);
	hipLaunchKernelGGL(kernel[rec ? 1 : 0][shadow ? 1 : 0], dim3(blocks), dim3(64), lds, ctx->stream, g, c.value_list, c.span,
			   c.offset, (const u32 *)ctx->ubitmap.p, c.verts, c.tris, rec, c.rays, (const u32 *)list, (const u32 *)dcount,
			   PPW, COOP, a, more...);
	ugrt_prof_end(ctx, UGRT_ST_TRACE_DDA);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}

// k_pixel_gather<., ., Kind>: S lanes a pixel, the table padded to the 16 bytes of the copy's float4 stores, Kind::extra
// floats and the Late, padded alike
template <class Kind> static int pixel_gather(const GatherCall &c, const typename Kind::Arg &a, bool shadow)
{
	static const GatherKernel<typename Kind::Arg> kernel[2][2] = {
		{ k_pixel_gather<false, false, Kind>, k_pixel_gather<false, true, Kind> },
		{ k_pixel_gather<true, false, Kind>, k_pixel_gather<true, true, Kind> },
	};
	const size_t lds = (((size_t)(4u * Kind::entry) * (size_t)(a.set_w * a.set_h * (u32)a.count) + 15u) & ~(size_t)15u) +
			   4u * Kind::extra + ((sizeof(typename Kind::Late) + 15u) & ~(size_t)15u);
	return gather_launch(c, (u32)a.count, lds, kernel, shadow, nullptr, a);
}

#endif
