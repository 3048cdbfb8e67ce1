// ugrt_dda_any.hip -- any-hit traversal of the uniform grid: "is anything in the way between here and there"
// (not in the reference).
//
// Spec: a ray is occluded iff some triangle in the list of some VISITED cell passes ugrt_trace_dda's exact test
// (d_mt_core, same operands) with 0 < t < t_max.  The visited cells are those of ugrt_trace_dda's walk -- d_dda_clip,
// d_dda_axes and d_dda_step of ugrt_dda.h, which the per-ray kernel calls too, and its dims-sum guard -- from the entry cell onwards for as long
// as a cell's entry parameter (tenter, then the exit parameter of the cell before) is below t_max.  The result is an OR
// over a fixed set of cells, so none of what the closest-hit kernels order their work by is needed here:
//   * a lane (= ray) is done at its first accepted test, a wave leaves when no lane walks any more;
//   * a window of ANY_AHEAD steps is planned in registers.  The plan is the cells alone: no exit parameter is kept per
//     step, because no cell has to be compared with a closest hit -- where the walk ends is decided while planning;
//   * the window's cells are looked up in the occupancy bitmap (83 % of the visited cells are empty on the bench
//     frame), and span / offset are fetched for the occupied ones only;
//   * a short list is tested by its lane; a long one by the wave, 64 triangles per round with the owner's ray
//     broadcast, and a round is accepted with one ballot: no 64-bit minimum, no LDS, no list position.
// The kernel reads the grid and the rays and writes its flags: it neither reads nor writes the split walks' history.
// ugrt_trace_dda_any_lights is the same kernel over (light, ray group): the walk towards several
// points from one set of origins, with one prepare launch and one ray list.  ugrt_trace_dda_any_hemi (DESIGN.md section
// 6.5) is the same kernel over (direction, ray group): S directions of the hemisphere over each stored normal, formed in
// registers, one bit of a mask word per direction.  ugrt_trace_dda_any_thru and ugrt_trace_dda_any_lights_thru (DESIGN.md
// section 6.6) are the same kernel with THRU: an accepted test counts only if the triangle's material does not transmit.
// ugrt_trace_dda_any_area and its _thru form are the same kernel over (pixel group, sample): the S
// rays of a pixel towards S points of a light's disk in neighbouring lanes of one wave, one mask word per pixel.
// ugrt_trace_dda_any_area_sets and its _thru form are that walk with one sample set per pixel of a
// set_w x set_h tile of the image: the sets lie in device memory, a workgroup copies them to LDS once.
// ugrt_trace_dda_any_hemi_sets is the hemisphere walk in that index space: the S directions of a
// pixel in neighbouring lanes, one set of local directions per pixel of the tile, the word stored whole from one ballot.
#include "ugrt_gather.h" // (d_stage_table, d_ticket_draw)
#include <type_traits>

#define ANY_AHEAD 8 // steps planned (and looked up in the bitmap) per window

// What the rays of a launch aim at.  AnyRays: the rays as they are stored, up to t_max (ugrt_trace_dda_any).  AnyLights: from
// the stored origins towards num_lights points (ugrt_trace_dda_any_lights): the index space is
// (light, ray group), light-major -- group G of the launch is group G % per_light of the ray list under light
// G / per_light, so a wave never mixes lights, its light's position is three scalars of the by-value block, and waves
// that run side by side walk neighbouring rays towards one light.  The direction light - o is formed in the kernel, per
// component, as k_occlusion_rays forms it: the rays' own last three floats are not read.  The light lies at t = 1, and
// light l's flags lie at l * level.
struct AnyRays {
	typedef float Arg; // t_max
	static constexpr bool lights = false, hemi = false, area = false, sets = false;
};
struct AnyLights {
	struct Arg {
		float pos[3 * UGRT_MAX_LIGHTS]; // by value: uniform over the launch, read from the kernarg segment
		int count;
		size_t level; // W*H
	};
	static constexpr bool lights = true, hemi = false, area = false, sets = false;
};
// AnyHemi: from the stored origins along num_dirs directions of the hemisphere over the stored normal
// (ugrt_trace_dda_any_hemi), up to `radius`.  The index space is (direction, ray group),
// direction-major as AnyLights is light-major: a wave never mixes directions, its local direction is three scalars of the
// by-value block, and waves side by side walk neighbouring pixels along one local direction.  The slot's last three floats
// are the unit normal; d_hemi_dir turns the local direction into the world's.  Direction s is bit s of the pixel's mask.
struct AnyHemi {
	struct Arg {
		float dirs[3 * UGRT_MAX_AO_DIRS]; // by value: uniform over the launch, read from the kernarg segment
		int count;
		float radius;
	};
	static constexpr bool lights = false, hemi = true, area = false, sets = false;
};
// AnyArea: from the stored origins towards `count` = S points (ugrt_trace_dda_any_area); the sample
// lies at t = 1.  The index space is (pixel group, sample), pixel-major: a group is PPW = max(1, L / S) slots of the ray
// list (the kernel's RPW argument carries PPW), lane l < PPW * S walks slot lgrp * PPW + l / S towards sample l % S and
// the lanes behind idle.  The S rays of a pixel share the origin, the entry cell and most cells behind it, and they sit
// side by side: bit s of the pixel's word is one bit of the wave's ballot, and the pixel's first lane stores the word.
// The sample is per lane here, so the by-value block cannot be read with scalar loads where it is used: lane 0 copies
// it to LDS once per wave (uniform indices: scalar loads), and a lane reads its three floats from there per group.
struct AnyArea {
	struct Arg {
		float pos[3 * UGRT_MAX_AREA_SAMPLES]; // by value: uniform over the launch, read from the kernarg segment
		int count;
	};
	static constexpr bool lights = false, hemi = false, area = true, sets = false;
};
// AnyAreaSets: AnyArea with a sample set per pixel (ugrt_trace_dda_any_area_sets): pixel p = (x, y)
// of the full image aims at set k(p) = (y % set_h) * set_w + (x % set_w) of `pos`, device memory [set_w * set_h][S][3].
// The table is too large for the by-value block (6 KB at 16 sets of 32): every workgroup copies it to dynamic LDS once,
// with the whole wave's loads, and a lane reads its three floats at 3 * (k(p) * S + sample).  k(p) is formed from the
// pixel id behind the list's load and used there only: it costs the walk no register.
struct AnyAreaSets {
	struct Arg {
		const float *pos;
		int count;          // S
		u32 set_w, set_h;   // 1..4 each
		u32 width;          // of the full image
	};
	static constexpr bool lights = false, hemi = false, area = true, sets = true;
};
// AnyHemiSets: AnyHemi in AnyAreaSets' index space (ugrt_trace_dda_any_hemi_sets): pixel p walks
// along set k(p) of `pos`, device memory [set_w * set_h][S][3] LOCAL directions, up to `radius`.  The fields AnyAreaSets
// has carry its names: the table's copy, k(p), the lane mapping and the ballot store are its code.  A lane reads the
// pixel's normal and its three local floats from LDS, and d_hemi_dir forms the world direction per lane: the S lanes of
// a pixel repeat the basis, which is dead before the first cell (no register of the walk) and needs no lane exchange.
struct AnyHemiSets {
	struct Arg {
		const float *pos;
		int count;          // S
		u32 set_w, set_h;   // 1..4 each
		u32 width;          // of the full image
		float radius;
	};
	static constexpr bool lights = false, hemi = true, area = true, sets = true;
};
// (dynamic LDS, its base 16-byte aligned; the aims over sets are the only ones that have any)
extern __shared__ __attribute__((aligned(16))) float s_sets_pos[];
// (d_area_lane, which slot of its group and which sample a lane serves: ugrt_dda.h)
// (function-scope LDS: only the kernels that call this carry it)
__device__ __forceinline__ float *d_area_lds()
{
	__shared__ float s_pos[3 * UGRT_MAX_AREA_SAMPLES];
	return s_pos;
}

// THRU: which triangles a ray passes: f is see-through when m = mat_idx[f] is in range and
// transmit[m] > 0.  The plain kernels take the empty block: their arguments and their code stay what they were.
struct ThruArg {
	const int *mat_idx;
	const float *transmit;
	int mat_count;
};
struct NoThru {};
__device__ __forceinline__ bool d_see_through(const ThruArg &a, const u32 *__restrict__ value_list, u32 at)
{
	// (the list entry is read again: kept in a register over the exact test it would cost the walk a wave per SIMD)
	asm volatile("" : "+v"(at));
	const int m = a.mat_idx[value_list[at]];
	return m >= 0 && m < a.mat_count && a.transmit[m] > 0;
}

// (d_hemi_dir, the world direction of a local one over a normal: ugrt_dda.h)

// `occluded` of the band was cleared by the prepare kernel (AnyLights: layer 0; the layers behind by the host call): only
// the flags of occluded rays are written (AnyHemi: `occluded` is the mask words, bit s is OR-ed in by direction s's lane;
// AnyArea: the mask words, a non-zero word is stored whole by its pixel's first lane)
template <bool REC, class Aim, bool THRU = false>
__global__ __launch_bounds__(64) void k_trace_dda_any(DGrid g, const u32 *__restrict__ value_list,
							const u32 *__restrict__ span, const u32 *__restrict__ offset,
							const u32 *__restrict__ bitmap, const float *__restrict__ verts,
							const int *__restrict__ tris, const float4 *__restrict__ rec,
							const float *__restrict__ rays, const u32 *__restrict__ list,
							const u32 *__restrict__ count_p, const typename Aim::Arg aim, int *__restrict__ occluded,
							u32 RPW, u32 COOP, u32 *__restrict__ ticket,
							const std::conditional_t<THRU, ThruArg, NoThru> thru)
{
	const int lane = threadIdx.x;
	const u32 count = *count_p;
	constexpr bool layered = Aim::lights || (Aim::hemi && !Aim::area); // the index space is (light or direction, ray group)
	float t_max;
	if constexpr (Aim::lights)
		t_max = 1.0f;
	else if constexpr (Aim::hemi)
		t_max = aim.radius;
	else if constexpr (Aim::area)
		t_max = 1.0f;
	else
		t_max = aim;
	// AnyArea: the samples in LDS
	if constexpr (Aim::sets) {
		d_stage_table(s_sets_pos, aim.pos, 3u * (u32)aim.count * aim.set_w * aim.set_h, lane); // 3 * K * S floats
		__syncthreads();
	} else if constexpr (Aim::area) {
		const u32 S = (u32)aim.count;
		float *s_pos = d_area_lds();
		for (u32 i = 0; i < 3u * S; i++) {
			const float v = aim.pos[i]; // (uniform index)
			if (lane == 0)
				s_pos[i] = v;
		}
		__syncthreads();
	}
	// AnyLights: the ray count is the device's, so is the number of groups per light (no ray: no group, no division)
	u32 per_light = 0u, groups = 0u;
	if constexpr (layered) {
		per_light = (count + RPW - 1u) / RPW;
		groups = per_light * (u32)aim.count;
	}
	// groups of RPW rays, the first gridDim.x by workgroup id, the others drawn from the ticket
	for (u32 grp = blockIdx.x; layered ? grp < groups : grp * RPW < count;) {
		u32 light = 0u, lgrp = grp; // (uniform; AnyHemi: the direction)
		if constexpr (layered) {
			light = grp / per_light;
			lgrp = grp - light * per_light;
		}
		u32 slot = lgrp * RPW + (u32)lane;
		bool inb = (u32)lane < RPW && slot < count;
		u32 asmp = 0u;
		if constexpr (Aim::area) { // (RPW is the pixels per wave)
			u32 apix;
			d_area_lane(lane, (u32)aim.count, apix, asmp);
			slot = lgrp * RPW + apix;
			inb = apix < RPW && slot < count;
		}
		const int p = inb ? (int)list[slot] : 0;
		inb = inb && p != -1; // (padding: k_dda_prepare)
		if constexpr (Aim::sets) { // the lane's sample becomes its index into the table: set k(p), sample asmp
			// (the divisors are made opaque here: their reciprocals are formed per group, not kept over the walk)
			u32 width = aim.width, set_w = aim.set_w, set_h = aim.set_h;
			asm volatile("" : "+s"(width), "+s"(set_w), "+s"(set_h));
			const u32 y = (u32)p / width, x = (u32)p - y * width;
			asmp += ((y % set_h) * set_w + x % set_w) * (u32)aim.count;
		}
		float o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 0 }, tmax[3] = { 0, 0, 0 }, tdelta[3] = { 0, 0, 0 };
		int c[3] = { 0, 0, 0 }, step[3] = { 0, 0, 0 };
		bool walking = false, occ = false;
		if (inb) {
#pragma unroll
			for (int k = 0; k < 3; k++) {
				o[k] = rays[p * 6 + k];
				if constexpr (Aim::lights)
					d[k] = aim.pos[3u * light + (u32)k] - o[k];
				else if constexpr (Aim::sets && !Aim::hemi)
					d[k] = s_sets_pos[3u * asmp + (u32)k] - o[k];
				else if constexpr (Aim::area && !Aim::hemi)
					d[k] = d_area_lds()[3u * asmp + (u32)k] - o[k];
				else
					d[k] = rays[p * 6 + 3 + k];
			}
			if constexpr (Aim::hemi && Aim::sets) { // (d is the normal; the local direction is the lane's own)
				const float nrm[3] = { d[0], d[1], d[2] };
				d_hemi_dir(nrm, s_sets_pos[3u * asmp], s_sets_pos[3u * asmp + 1u], s_sets_pos[3u * asmp + 2u], d);
			} else if constexpr (Aim::hemi) {
				const float nrm[3] = { d[0], d[1], d[2] };
				d_hemi_dir(nrm, aim.dirs[3u * light], aim.dirs[3u * light + 1u], aim.dirs[3u * light + 2u], d);
			}
			float tenter;
			if (d_dda_clip(g, o, d, tenter)) {
				walking = tenter < t_max; // the entry cell's entry parameter
				d_dda_axes(g, o, d, tenter, c, step, tmax, tdelta);
			}
		}
		int guard = g.dims[0] + g.dims[1] + g.dims[2] + 3;
		while (__ballot(walking) != 0ull) {
			// 1. the window's cells.  The walk ends behind a cell when the ray leaves the grid there, when the guard runs
			// out, or when the cell's exit parameter -- the next cell's entry parameter -- is not below t_max.
			u32 pcell[ANY_AHEAD], pvalid = 0u;
			bool planning = walking;
#pragma unroll
			for (int q = 0; q < ANY_AHEAD; q++) {
				pcell[q] = 0u;
				if (planning) {
					pvalid |= 1u << q;
					pcell[q] = (u32)((c[0] * g.dims[1] + c[1]) * g.dims[2] + c[2]);
					float tnext;
					const bool outside = d_dda_step(g, c, step, tmax, tdelta, tnext);
					if (outside || --guard <= 0 || !(tnext < t_max))
						planning = false;
				}
			}
			// 2. which of them hold a triangle: one bitmap word per step, then the headers of the occupied cells only
			u32 pword[ANY_AHEAD], psp[ANY_AHEAD], poff[ANY_AHEAD];
#pragma unroll
			for (int q = 0; q < ANY_AHEAD; q++)
				pword[q] = ((pvalid >> q) & 1u) ? bitmap[pcell[q] >> 5] : 0u;
#pragma unroll
			for (int q = 0; q < ANY_AHEAD; q++) {
				const bool full = (pword[q] >> (pcell[q] & 31u)) & 1u;
				psp[q] = full ? span[pcell[q]] : 0u;
				poff[q] = full ? offset[pcell[q]] : 0u;
			}
			// 3. the tests, until the ray's first accepted one
#pragma unroll
			for (int q = 0; q < ANY_AHEAD; q++) {
				const u32 sp = walking ? psp[q] : 0u, off = poff[q];
				if (__ballot(sp != 0u) == 0ull)
					continue;
				// short lists: the owning lane
				if (sp < COOP) {
					for (u32 r = 0; r < sp; r++) {
						float t9[9], t;
						d_load_triangle<REC>(rec, verts, tris, value_list[off + r], o[0], o[1], o[2], t9);
						if (d_mt_core(&t9[0], &t9[3], &t9[6], d, &t) && t > 0.0f && t < t_max) {
							if constexpr (THRU) { // (the two loads: behind an accepted test only)
								if (d_see_through(thru, value_list, off + r))
									continue;
							}
							occ = true;
							break;
						}
					}
				}
				// long lists: one owner at a time, 64 triangles per round, accepted by one ballot
				unsigned long long heavy = __ballot(sp >= COOP);
				while (heavy != 0ull) {
					const int l = (int)__builtin_ctzll(heavy);
					heavy &= heavy - 1ull;
					const float ox = d_readlane(o[0], l), oy = d_readlane(o[1], l), oz = d_readlane(o[2], l);
					const float dl[3] = { d_readlane(d[0], l), d_readlane(d[1], l), d_readlane(d[2], l) };
					const u32 spl = (u32)__builtin_amdgcn_readlane((int)sp, l), offl = (u32)__builtin_amdgcn_readlane((int)off, l);
					bool hit = false;
					for (u32 base = 0; base < spl && !hit; base += 64u) {
						const u32 r = base + (u32)lane;
						bool acc = false;
						if (r < spl) {
							float t9[9], t;
							d_load_triangle<REC>(rec, verts, tris, value_list[offl + r], ox, oy, oz, t9);
							acc = d_mt_core(&t9[0], &t9[3], &t9[6], dl, &t) && t > 0.0f && t < t_max;
							if constexpr (THRU) {
								if (acc && d_see_through(thru, value_list, offl + r))
									acc = false;
							}
						}
						hit = __ballot(acc) != 0ull;
					}
					if (hit && lane == l)
						occ = true;
				}
				walking = walking && !occ;
			}
			walking = walking && planning; // (planning: the walk goes on behind this window)
		}
		if constexpr (Aim::area) {
			// the pixel's S flags are S neighbouring bits of the ballot (idle and out-of-range lanes hold occ = false)
			const u32 S = (u32)aim.count;
			u32 apix, asmp;
			d_area_lane(lane, S, apix, asmp);
			const unsigned long long flags = __ballot(occ);
			const u32 word = (u32)(flags >> ((apix * S) & 63u)) & (S == 32u ? 0xFFFFFFFFu : (1u << S) - 1u);
			if (inb && asmp == 0u && word != 0u)
				((u32 *)occluded)[p] = word;
		} else if (occ) {
			if constexpr (Aim::lights)
				(occluded + (size_t)light * aim.level)[p] = 1; // (the layer's base is uniform)
			else if constexpr (Aim::hemi)
				atomicOr((u32 *)occluded + p, 1u << light); // (each (p, s) has one lane: this merges a word's S writers)
			else
				occluded[p] = 1;
		}
		grp = d_ticket_draw(lane, grp, ticket);
	}
}

// ---------------------------------------------------------------------------
// the host side: one path for every aim.  An export checks its arguments, fills its Aim::Arg and calls any_walk<Aim>.
// ---------------------------------------------------------------------------
// what every export is given; out: the flags, or the mask words; thru null: the plain kernel
struct AnyCall {
	ugrt_ctx *ctx;
	const char *who;
	const unsigned *value_list, *span, *offset;
	const float *verts;
	const int *tris;
	const float *rays;
	const int *active;
	int *out;
	const ThruArg *thru;
};

// own: the export's own pointer argument (the lights, the directions, the samples), where it has one
static int any_null_check(const AnyCall &c, const void *own = "")
{
	if (!c.ctx || !c.value_list || !c.span || !c.offset || !c.verts || !c.tris || !c.rays || !c.active || !own || !c.out ||
	    (c.thru && (!c.thru->mat_idx || !c.thru->transmit)))
		return ugrt_fail(UGRT_EINVAL, "%s: null argument", c.who);
	return UGRT_OK;
}

// The prepare launch and the kernel for one aim.  What differs between the aims is read from the aim's flags:
//   * the layers of the index space: AnyLights and AnyHemi walk (light or direction, ray group), aim.count layers
//     (AnyHemiSets is an area aim: one layer);
//   * the group: "any_rays_per_wave" rays (unset: 32); the area aims give L = "any_rays_per_wave" of a wave's lanes
//     (at most and unset: all 64) rays, PPW = max(1, L / S) pixels' S samples each, and the kernel's RPW carries PPW;
//   * dynamic LDS: the table of the aims over sets, rounded up to the 16 bytes of the copy's float4 stores (at most 6 KB);
//   * AnyLights' layers behind the first are cleared here; the hemisphere aims have no see-through kernel.
template <class Aim> static int any_walk(const AnyCall &c, const typename Aim::Arg &aim)
{
	ugrt_ctx *ctx = c.ctx;
	Grid &G = ctx->grid[UGRT_GRID_UNIFORM];
	if (!G.valid)
		return ugrt_fail(UGRT_EINVAL, "trace_dda: build the uniform grid first (it defines the cell geometry)");
	UGRT_HIP(hipSetDevice(ctx->device));
	const DGrid g = ugrt_dgrid_of(G);
	const float4 *rec = ugrt_trirec_of(ctx, c.verts, c.tris);
	// launch shape (ugrt_ctx_set_option; no effect on results)
	u32 RPW = ctx->opt[UGRT_OPT_ANY_RPW] > 0 ? (u32)ctx->opt[UGRT_OPT_ANY_RPW] : 32u, layers = 1u;
	const u32 COOP = ctx->opt[UGRT_OPT_ANY_COOP] > 0 ? (u32)ctx->opt[UGRT_OPT_ANY_COOP] : 8u;
	size_t lds = 0;
	if constexpr (Aim::area) {
		const u32 L = ctx->opt[UGRT_OPT_ANY_RPW] > 0 ? (ctx->opt[UGRT_OPT_ANY_RPW] < 64 ? (u32)ctx->opt[UGRT_OPT_ANY_RPW] : 64u) : 64u;
		RPW = L / (u32)aim.count > 0u ? L / (u32)aim.count : 1u;
	}
	if constexpr (Aim::lights || (Aim::hemi && !Aim::area))
		layers = (u32)aim.count;
	if constexpr (Aim::sets)
		lds = ((size_t)12 * (size_t)(aim.set_w * aim.set_h * (u32)aim.count) + 15u) & ~(size_t)15u;
	// ONE prepare launch and one ray list for all layers, in the form that writes no hit defaults (it clears the band's
	// flags or mask words instead: of AnyLights, layer 0), always with the bitmap workgroups, never with the split walks'
	// chunk table.  AnyLights' layers behind are cleared here in stream order: one fill where the band is the frame (the
	// layers are contiguous), one per layer otherwise.
	u32 *list, *dcount;
	hipError_t he = hipSuccess;
	ugrt_prof_begin(ctx, UGRT_ST_WORKLIST);
	const int rc = ugrt_dda_prepare(ctx, g, c.active, nullptr, c.out, c.span, true, nullptr, &list, &dcount);
	if constexpr (Aim::lights) {
		const size_t level = aim.level;
		if (!rc && aim.count > 1) {
			if ((size_t)ctx->npix == level)
				he = hipMemsetAsync(c.out + level, 0, (size_t)(aim.count - 1) * level * sizeof(int), ctx->stream);
			else
				for (int l = 1; l < aim.count && he == hipSuccess; l++)
					he = hipMemsetAsync(c.out + (size_t)l * level + (size_t)ctx->p0, 0, (size_t)ctx->npix * sizeof(int),
							    ctx->stream);
		}
	}
	ugrt_prof_end(ctx, UGRT_ST_WORKLIST);
	if (rc)
		return rc;
	UGRT_HIP(he);
	// persistent single-wave workgroups over (layer, group); "dda_blocks" caps them as it caps ugrt_trace_dda's
	int blocks = launch_blocks_for(((u32)ctx->npix / RPW + 1u) * layers);
	if (ctx->opt[UGRT_OPT_DDA_BLOCKS] > 0 && blocks > ctx->opt[UGRT_OPT_DDA_BLOCKS])
		blocks = ctx->opt[UGRT_OPT_DDA_BLOCKS];
	auto launch = [&](const auto &thru) {
		constexpr bool THRU = std::is_same_v<std::decay_t<decltype(thru)>, ThruArg>;
		hipLaunchKernelGGL((rec ? k_trace_dda_any<true, Aim, THRU> : k_trace_dda_any<false, Aim, THRU>), dim3(blocks), dim3(64),
				   lds, ctx->stream, g, c.value_list, c.span, c.offset, (const u32 *)ctx->ubitmap.p, c.verts, c.tris, rec,
				   c.rays, (const u32 *)list, (const u32 *)dcount, aim, c.out, RPW, COOP, ctx->d_small + UGRT_DSMALL_TICKET,
				   thru);
	};
	ugrt_prof_begin(ctx, UGRT_ST_TRACE_DDA);
	if constexpr (Aim::hemi)
		launch(NoThru());
	else if (c.thru)
		launch(*c.thru);
	else
		launch(NoThru());
	ugrt_prof_end(ctx, UGRT_ST_TRACE_DDA);
	UGRT_HIP(hipGetLastError());
	return UGRT_OK;
}

static int trace_dda_any(const AnyCall &c, float t_max)
{
	if (int rc = any_null_check(c))
		return rc;
	if (!(t_max > 0.0f))
		return ugrt_fail(UGRT_EINVAL, "%s: t_max must be greater than 0", c.who);
	return any_walk<AnyRays>(c, t_max);
}

static int trace_dda_any_lights(const AnyCall &c, int num_lights, const float *light_pos)
{
	if (int rc = any_null_check(c, light_pos))
		return rc;
	if (num_lights < 1 || num_lights > UGRT_MAX_LIGHTS)
		return ugrt_fail(UGRT_EINVAL, "%s: num_lights %d is not in 1..%d", c.who, num_lights, UGRT_MAX_LIGHTS);
	AnyLights::Arg lights = {};
	for (int k = 0; k < 3 * num_lights; k++)
		lights.pos[k] = light_pos[k];
	lights.count = num_lights;
	lights.level = (size_t)c.ctx->cfg.width * (size_t)c.ctx->cfg.height;
	return any_walk<AnyLights>(c, lights);
}

static int trace_dda_any_hemi(const AnyCall &c, int num_dirs, const float *dirs, float radius)
{
	if (int rc = any_null_check(c, dirs))
		return rc;
	if (num_dirs < 1 || num_dirs > UGRT_MAX_AO_DIRS)
		return ugrt_fail(UGRT_EINVAL, "%s: num_dirs %d is not in 1..%d", c.who, num_dirs, UGRT_MAX_AO_DIRS);
	if (!(radius > 0.0f))
		return ugrt_fail(UGRT_EINVAL, "%s: radius must be greater than 0", c.who);
	AnyHemi::Arg hemi = {};
	for (int k = 0; k < 3 * num_dirs; k++)
		hemi.dirs[k] = dirs[k];
	hemi.count = num_dirs;
	hemi.radius = radius;
	return any_walk<AnyHemi>(c, hemi);
}

static int trace_dda_any_area(const AnyCall &c, int num_samples, const float *sample_pos)
{
	if (int rc = any_null_check(c, sample_pos))
		return rc;
	if (num_samples < 1 || num_samples > UGRT_MAX_AREA_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "%s: num_samples %d is not in 1..%d", c.who, num_samples, UGRT_MAX_AREA_SAMPLES);
	AnyArea::Arg area = {};
	for (int k = 0; k < 3 * num_samples; k++)
		area.pos[k] = sample_pos[k];
	area.count = num_samples;
	return any_walk<AnyArea>(c, area);
}

static int trace_dda_any_area_sets(const AnyCall &c, int num_samples, int set_w, int set_h, const float *d_sample_pos)
{
	if (int rc = any_null_check(c, d_sample_pos))
		return rc;
	if (num_samples < 1 || num_samples > UGRT_MAX_AREA_SAMPLES)
		return ugrt_fail(UGRT_EINVAL, "%s: num_samples %d is not in 1..%d", c.who, num_samples, UGRT_MAX_AREA_SAMPLES);
	if (set_w < 1 || set_w > UGRT_MAX_AREA_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "%s: set_w %d is not in 1..%d", c.who, set_w, UGRT_MAX_AREA_SET_TILE);
	if (set_h < 1 || set_h > UGRT_MAX_AREA_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "%s: set_h %d is not in 1..%d", c.who, set_h, UGRT_MAX_AREA_SET_TILE);
	if (set_w * set_h * num_samples > UGRT_MAX_AREA_SET_POINTS)
		return ugrt_fail(UGRT_EINVAL, "%s: set_w * set_h * num_samples = %d is more than %d", c.who,
				 set_w * set_h * num_samples, UGRT_MAX_AREA_SET_POINTS);
	AnyAreaSets::Arg area = {};
	area.pos = d_sample_pos;
	area.count = num_samples;
	area.set_w = (u32)set_w;
	area.set_h = (u32)set_h;
	area.width = (u32)c.ctx->cfg.width;
	return any_walk<AnyAreaSets>(c, area);
}

static int trace_dda_any_hemi_sets(const AnyCall &c, int num_dirs, int set_w, int set_h, const float *d_dirs, float radius)
{
	if (int rc = any_null_check(c, d_dirs))
		return rc;
	if (num_dirs < 1 || num_dirs > UGRT_MAX_AO_DIRS)
		return ugrt_fail(UGRT_EINVAL, "%s: num_dirs %d is not in 1..%d", c.who, num_dirs, UGRT_MAX_AO_DIRS);
	if (set_w < 1 || set_w > UGRT_MAX_AO_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "%s: set_w %d is not in 1..%d", c.who, set_w, UGRT_MAX_AO_SET_TILE);
	if (set_h < 1 || set_h > UGRT_MAX_AO_SET_TILE)
		return ugrt_fail(UGRT_EINVAL, "%s: set_h %d is not in 1..%d", c.who, set_h, UGRT_MAX_AO_SET_TILE);
	if (set_w * set_h * num_dirs > UGRT_MAX_AO_SET_DIRS)
		return ugrt_fail(UGRT_EINVAL, "%s: set_w * set_h * num_dirs = %d is more than %d", c.who, set_w * set_h * num_dirs,
				 UGRT_MAX_AO_SET_DIRS);
	if (!(radius > 0.0f))
		return ugrt_fail(UGRT_EINVAL, "%s: radius must be greater than 0", c.who);
	AnyHemiSets::Arg hemi = {};
	hemi.pos = d_dirs;
	hemi.count = num_dirs;
	hemi.set_w = (u32)set_w;
	hemi.set_h = (u32)set_h;
	hemi.width = (u32)c.ctx->cfg.width;
	hemi.radius = radius;
	return any_walk<AnyHemiSets>(c, hemi);
}

extern "C" int ugrt_trace_dda_any(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				  const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				  const float *d_rays, const int *d_active, float t_max, int *d_occluded)
{
	return trace_dda_any({ ctx, "trace_dda_any", d_value_list, d_span, d_offset, d_vertlist, d_trilist, d_rays, d_active,
			       d_occluded, nullptr },
			     t_max);
}

extern "C" int ugrt_trace_dda_any_thru(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				       const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				       const float *d_rays, const int *d_active, float t_max, int *d_occluded,
				       const int *d_mat_idx, const float *d_transmit, int num_materials)
{
	const ThruArg thru = { d_mat_idx, d_transmit, num_materials };
	return trace_dda_any({ ctx, "trace_dda_any_thru", d_value_list, d_span, d_offset, d_vertlist, d_trilist, d_rays,
			       d_active, d_occluded, &thru },
			     t_max);
}

extern "C" int ugrt_trace_dda_any_lights(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
					 const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
					 const float *d_orays, const int *d_oactive, int num_lights, const float *light_pos,
					 int *d_occluded)
{
	return trace_dda_any_lights({ ctx, "trace_dda_any_lights", d_value_list, d_span, d_offset, d_vertlist, d_trilist,
				      d_orays, d_oactive, d_occluded, nullptr },
				    num_lights, light_pos);
}

extern "C" int ugrt_trace_dda_any_lights_thru(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
					      const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
					      const float *d_orays, const int *d_oactive, int num_lights, const float *light_pos,
					      int *d_occluded, const int *d_mat_idx, const float *d_transmit, int num_materials)
{
	const ThruArg thru = { d_mat_idx, d_transmit, num_materials };
	return trace_dda_any_lights({ ctx, "trace_dda_any_lights_thru", d_value_list, d_span, d_offset, d_vertlist, d_trilist,
				      d_orays, d_oactive, d_occluded, &thru },
				    num_lights, light_pos);
}

extern "C" int ugrt_trace_dda_any_hemi(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				       const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				       const float *d_orays, const int *d_oactive, int num_dirs, const float *dirs, float radius,
				       unsigned *d_mask)
{
	return trace_dda_any_hemi({ ctx, "trace_dda_any_hemi", d_value_list, d_span, d_offset, d_vertlist, d_trilist, d_orays,
				    d_oactive, (int *)d_mask, nullptr },
				  num_dirs, dirs, radius);
}

extern "C" int ugrt_trace_dda_any_area(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				       const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
				       const float *d_orays, const int *d_oactive, int num_samples, const float *sample_pos,
				       unsigned *d_mask)
{
	return trace_dda_any_area({ ctx, "trace_dda_any_area", d_value_list, d_span, d_offset, d_vertlist, d_trilist, d_orays,
				    d_oactive, (int *)d_mask, nullptr },
				  num_samples, sample_pos);
}

extern "C" int ugrt_trace_dda_any_area_thru(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
					    const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
					    const float *d_orays, const int *d_oactive, int num_samples, const float *sample_pos,
					    unsigned *d_mask, const int *d_mat_idx, const float *d_transmit, int num_materials)
{
	const ThruArg thru = { d_mat_idx, d_transmit, num_materials };
	return trace_dda_any_area({ ctx, "trace_dda_any_area_thru", d_value_list, d_span, d_offset, d_vertlist, d_trilist,
				    d_orays, d_oactive, (int *)d_mask, &thru },
				  num_samples, sample_pos);
}

extern "C" int ugrt_trace_dda_any_area_sets(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
					    const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
					    const float *d_orays, const int *d_oactive, int num_samples, int set_w, int set_h,
					    const float *d_sample_pos, unsigned *d_mask)
{
	return trace_dda_any_area_sets({ ctx, "trace_dda_any_area_sets", d_value_list, d_span, d_offset, d_vertlist, d_trilist,
					 d_orays, d_oactive, (int *)d_mask, nullptr },
				       num_samples, set_w, set_h, d_sample_pos);
}

extern "C" int ugrt_trace_dda_any_area_sets_thru(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
						 const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
						 const float *d_orays, const int *d_oactive, int num_samples, int set_w, int set_h,
						 const float *d_sample_pos, unsigned *d_mask, const int *d_mat_idx,
						 const float *d_transmit, int num_materials)
{
	const ThruArg thru = { d_mat_idx, d_transmit, num_materials };
	return trace_dda_any_area_sets({ ctx, "trace_dda_any_area_sets_thru", d_value_list, d_span, d_offset, d_vertlist,
					 d_trilist, d_orays, d_oactive, (int *)d_mask, &thru },
				       num_samples, set_w, set_h, d_sample_pos);
}

extern "C" int ugrt_trace_dda_any_hemi_sets(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
					    const unsigned *d_offset, const float *d_vertlist, const int *d_trilist,
					    const float *d_orays, const int *d_oactive, int num_dirs, int set_w, int set_h,
					    const float *d_dirs, float radius, unsigned *d_mask)
{
	return trace_dda_any_hemi_sets({ ctx, "trace_dda_any_hemi_sets", d_value_list, d_span, d_offset, d_vertlist, d_trilist,
					 d_orays, d_oactive, (int *)d_mask, nullptr },
				       num_dirs, set_w, set_h, d_dirs, radius);
}

