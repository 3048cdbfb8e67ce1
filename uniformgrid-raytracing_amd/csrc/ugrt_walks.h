// ugrt_walks.h -- the two walks through the uniform grid of the kernels that give a pixel S rays in neighbouring lanes and
// keep each ray, its hit and what follows from it in registers (ugrt_gather.h: k_pixel_gather, the body of the indirect
// light's, the glossy lobe's and the sub-pixel eye rays' gathers; ugrt_fresnel.hip: the tree).  One ray per lane; every lane of the wave calls a walk, a lane without a ray only serves the
// cooperative rounds.  The windowed plan (WALK_AHEAD steps at a time) and the bitmap look-up in front of the headers are
// the any-hit kernel's (ugrt_dda_any.hip).
#ifndef UGRT_WALKS_H
#define UGRT_WALKS_H

#include "ugrt_dda.h"

#define WALK_AHEAD 8 // steps planned (and looked up in the bitmap) per window

// THRU: which triangles a ray passes (as ugrt_trace_dda_any_thru says it): f is see-through when
// m = mat_idx[f] is in range and transmit[m] > 0
struct WalkThru {
	const int *mat_idx;
	const float *transmit;
	int mat_count;
};
__device__ __forceinline__ bool d_walk_see_through(const WalkThru *a, u32 f)
{
	const int m = a->mat_idx[f];
	return m >= 0 && m < a->mat_count && a->transmit[m] > 0;
}

// k_trace_dda_any's loop: true = some triangle of a visited cell passes the exact test with 0 < t < t_max.  THRU: an
// accepted test counts only if the triangle is not see-through (thru; without THRU it is not read).
template <bool REC, bool THRU = false>
__device__ __forceinline__ bool d_any_walk(const DGrid &g, const u32 *__restrict__ value_list, const u32 *__restrict__ span,
					   const u32 *__restrict__ offset, const u32 *__restrict__ bitmap,
					   const float *__restrict__ verts, const int *__restrict__ tris,
					   const float4 *__restrict__ rec, const float *o, const float *d, float t_max,
					   bool walking, u32 COOP, int lane, const WalkThru *thru = nullptr)
{
	float tmax[3] = { 0, 0, 0 }, tdelta[3] = { 0, 0, 0 };
	int c[3] = { 0, 0, 0 }, step[3] = { 0, 0, 0 };
	bool occ = false;
	if (walking) {
		float tenter;
		walking = false;
		if (d_dda_clip(g, o, d, tenter)) {
			walking = tenter < t_max;
			d_dda_axes(g, o, d, tenter, c, step, tmax, tdelta);
		}
	}
	int guard = g.dims[0] + g.dims[1] + g.dims[2] + 3;
	while (__ballot(walking) != 0ull) {
		u32 pcell[WALK_AHEAD], pvalid = 0u;
		bool planning = walking;
#pragma unroll
		for (int q = 0; q < WALK_AHEAD; q++) {
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
		u32 pword[WALK_AHEAD], psp[WALK_AHEAD], poff[WALK_AHEAD];
#pragma unroll
		for (int q = 0; q < WALK_AHEAD; q++)
			pword[q] = ((pvalid >> q) & 1u) ? bitmap[pcell[q] >> 5] : 0u;
#pragma unroll
		for (int q = 0; q < WALK_AHEAD; q++) {
			const bool full = (pword[q] >> (pcell[q] & 31u)) & 1u;
			psp[q] = full ? span[pcell[q]] : 0u;
			poff[q] = full ? offset[pcell[q]] : 0u;
		}
#pragma unroll
		for (int q = 0; q < WALK_AHEAD; q++) {
			const u32 sp = walking ? psp[q] : 0u, off = poff[q];
			if (__ballot(sp != 0u) == 0ull)
				continue;
			if (sp < COOP) {
				for (u32 r = 0; r < sp; r++) {
					float t9[9], t;
					d_load_triangle<REC>(rec, verts, tris, value_list[off + r], o[0], o[1], o[2], t9);
					if (d_mt_core(&t9[0], &t9[3], &t9[6], d, &t) && t > 0.0f && t < t_max) {
						if constexpr (THRU) { // (the two loads: behind an accepted test only)
							if (d_walk_see_through(thru, value_list[off + r]))
								continue;
						}
						occ = true;
						break;
					}
				}
			}
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
							if (acc && d_walk_see_through(thru, value_list[offl + r]))
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
		walking = walking && planning;
	}
	return occ;
}

// k_trace_dda_ray's loop -- d_dda_clip, d_dda_axes, d_dda_step, the dims-sum guard, list order, strict acceptance
// 0 < t < best, the 64-bit wave minimum of the cooperative rounds, the walk ended behind the first cell whose exit
// parameter is not below an accepted t -- for the ray {o, d} of a lane with `start`: res_t / res_id get the closest hit,
// -1 / -2 without one.  RADIUS: best starts at min(3.0e38f, radius), the walk starts only where the entry parameter is
// below radius and also ends behind a cell whose exit parameter is not below radius (the any-hit walk's rule); without
// it `radius` is not read and the hit is ugrt_trace_dda's.
template <bool REC, bool RADIUS>
__device__ __forceinline__ void d_closest_walk(const DGrid &g, const u32 *__restrict__ value_list, const u32 *__restrict__ span,
					       const u32 *__restrict__ offset, const u32 *__restrict__ bitmap,
					       const float *__restrict__ verts, const int *__restrict__ tris,
					       const float4 *__restrict__ rec, const float *o, const float *d, float radius, bool start,
					       u32 COOP, int lane, float &res_t, int &res_id)
{
	float tmax[3] = { 0, 0, 0 }, tdelta[3] = { 0, 0, 0 };
	int c[3] = { 0, 0, 0 }, step[3] = { 0, 0, 0 };
	float best_t = RADIUS && radius < 3.0e38f ? radius : 3.0e38f;
	int best_id = -2;
	bool walking = false;
	res_t = -1.0f;
	res_id = -2;
	if (start) {
		float tenter;
		if (d_dda_clip(g, o, d, tenter)) {
			walking = RADIUS ? tenter < radius : true; // the entry cell's entry parameter
			d_dda_axes(g, o, d, tenter, c, step, tmax, tdelta);
		}
	}
	int guard = g.dims[0] + g.dims[1] + g.dims[2] + 3;
	while (__ballot(walking) != 0ull) {
		// 1. the window's cells and their exit parameters.  pend: the walk ends behind the cell -- the ray leaves the
		// grid there, the guard runs out, or (RADIUS) the exit parameter is not below radius
		u32 pcell[WALK_AHEAD], pvalid = 0u, pend = 0u;
		float ptnext[WALK_AHEAD];
		bool planning = walking;
#pragma unroll
		for (int q = 0; q < WALK_AHEAD; q++) {
			pcell[q] = 0u;
			ptnext[q] = 0.0f;
			if (planning) {
				pvalid |= 1u << q;
				pcell[q] = (u32)((c[0] * g.dims[1] + c[1]) * g.dims[2] + c[2]);
				const bool outside = d_dda_step(g, c, step, tmax, tdelta, ptnext[q]);
				if (outside || --guard <= 0 || (RADIUS && !(ptnext[q] < radius))) {
					pend |= 1u << q;
					planning = false;
				}
			}
		}
		// 2. which of them hold a triangle: one bitmap word per step, then the headers of the occupied cells only
		u32 pword[WALK_AHEAD], psp[WALK_AHEAD], poff[WALK_AHEAD];
#pragma unroll
		for (int q = 0; q < WALK_AHEAD; q++)
			pword[q] = ((pvalid >> q) & 1u) ? bitmap[pcell[q] >> 5] : 0u;
#pragma unroll
		for (int q = 0; q < WALK_AHEAD; q++) {
			const bool full = (pword[q] >> (pcell[q] & 31u)) & 1u;
			psp[q] = full ? span[pcell[q]] : 0u;
			poff[q] = full ? offset[pcell[q]] : 0u;
		}
		// 3. the tests, cell by cell, and behind each cell the question whether the walk ends there
#pragma unroll
		for (int q = 0; q < WALK_AHEAD; q++) {
			const bool here = walking && ((pvalid >> q) & 1u);
			const u32 sp = here ? psp[q] : 0u, off = poff[q];
			if (__ballot(sp != 0u) != 0ull) {
				// short lists: the owning lane, in list order
				if (sp < COOP) {
					for (u32 r = 0; r < sp; r++) {
						const u32 f = value_list[off + r];
						float t9[9], t;
						d_load_triangle<REC>(rec, verts, tris, f, o[0], o[1], o[2], t9);
						if (d_mt_core(&t9[0], &t9[3], &t9[6], d, &t) && t > 0.0f && t < best_t) {
							best_t = t;
							best_id = (int)f;
						}
					}
				}
				// long lists: one owner at a time, 64 triangles per round, the first r of the smallest t by a 64-bit minimum
				unsigned long long heavy = __ballot(sp >= COOP);
				while (heavy != 0ull) {
					const int l = (int)__builtin_ctzll(heavy);
					heavy &= heavy - 1ull;
					const float ox = d_readlane(o[0], l), oy = d_readlane(o[1], l), oz = d_readlane(o[2], l);
					const float dl[3] = { d_readlane(d[0], l), d_readlane(d[1], l), d_readlane(d[2], l) };
					const float bt = d_readlane(best_t, l);
					const u32 spl = (u32)__builtin_amdgcn_readlane((int)sp, l),
						  offl = (u32)__builtin_amdgcn_readlane((int)off, l);
					unsigned long long kbest = ~0ull;
					for (u32 base = 0; base < spl; base += 64u) {
						const u32 r = base + (u32)lane;
						unsigned long long key = ~0ull;
						if (r < spl) {
							float t9[9], t;
							d_load_triangle<REC>(rec, verts, tris, value_list[offl + r], ox, oy, oz, t9);
							if (d_mt_core(&t9[0], &t9[3], &t9[6], dl, &t) && t > 0.0f && t < bt)
								key = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)r;
						}
						key = d_wave_min_u64(key);
						kbest = key < kbest ? key : kbest;
					}
					if (lane == l && kbest != ~0ull) {
						best_t = __uint_as_float((u32)(kbest >> 32));
						best_id = (int)value_list[off + (u32)(kbest & 0xFFFFFFFFull)];
					}
				}
			}
			if (here) {
				if (best_id >= 0 && best_t <= ptnext[q]) {
					res_t = best_t;
					res_id = best_id;
					walking = false;
				} else if ((pend >> q) & 1u) {
					walking = false;
				}
			}
		}
	}
}

#endif
