// ugrt_dda.h -- pieces shared by the kernels that walk the uniform grid (ugrt_dda.hip: the per-ray kernel; ugrt_dda_walk.hip:
// the window kernel and the sort keys; ugrt_dda_any.hip: the any-hit kernel): grid geometry, the walk's arithmetic
// (d_dda_clip, d_dda_axes, d_dda_step: the one text of DESIGN.md A13's clip, start and step), the bundle cull, triangle records.
#ifndef UGRT_DDA_H
#define UGRT_DDA_H

#include "ugrt_packet.h"

struct DGrid {
	float lo[3], cs[3], inv[3];
	int dims[3];
};

// the cell geometry of a built uniform grid, as the bounce kernels take it
static inline DGrid ugrt_dgrid_of(const Grid &G)
{
	DGrid g;
	for (int k = 0; k < 3; k++) {
		g.lo[k] = G.ug[k];
		g.cs[k] = G.ug[3 + k];
		g.inv[k] = G.ug[6 + k];
		g.dims[k] = G.dims[k];
	}
	return g;
}

// the one k_dda_prepare launch of every call that walks the grid from a ray list (ugrt_dda.hip)
int ugrt_dda_prepare(ugrt_ctx *ctx, const DGrid &g, const int *d_active, float *d_hit_t, int *d_hit_id, const u32 *d_span,
		     bool with_bitmap, u32 *chunk, u32 **list_out, u32 **dcount_out);

// Segments of the window kernel's long ray groups (ugrt_dda_walk.hip, "split walks"); all pointers null: no splitting
#define WK_FBW 32      // windows of a group whose job counts are remembered (one byte each; later windows share the last)
#define WK_MAXSEG 4    // segments a group is cut into at most
struct WalkSplit {
	u32 *hdr;                // this launch: [0] rays, [1] rays per wave, [2] segments listed in `items`, [3] jobs of the launch before
	const uint2 *items;      // the cut groups' segments: x = group | segment << 24 | segments << 28, y = first window | end window << 16
	const unsigned char *cut; // per group: listed in `items` (its turn among the whole groups is skipped)
	unsigned char *fb;       // jobs of (group, window): written by this launch, read (and cleared) by the next one's k_dda_segments
	const u32 *chunk;        // per 64 list entries: span of pixels * 8 + chunk of the span (what the groups' history is kept under)
	u32 *walked_prev;        // per pixel: windows the ray walked in the launch before (which segments it is given to)
	u32 *walked;             // the same of this launch (the smallest over the segments that saw the ray end)
	u32 *done;               // per group: segments that have finished
	unsigned long long *key; // per pixel: closest hit over the segments, t bits << 32 | segment << 29 | behind << 28 | list position; (a later segment's hit behind its cell: walk again)
	u32 p0;                  // first pixel of the context's band: the per-pixel arrays below are indexed by pixel - p0
	u32 *tend;               // per pixel: exit parameter of the ray's last cell (all ones until a segment sees the ray leave)
	u32 *texam;              // per pixel: exit parameter of the last cell any segment has looked at for the ray (+inf: a segment stopped it)
};

// what the host passes to k_dda_segments beside WalkSplit (ugrt_dda_split_state)
struct WalkSplitHost {
	uint2 *items;
	unsigned char *cut;
	const u32 *hdr_prev;
	u32 *hdr_next;
	u32 load, force, maxg, maxseg;
};

// what a group's history is kept under: the list is made of chunks of 64 entries that belong to one span of pixels
// (k_dda_prepare), in an order that changes from launch to launch; `chunk` names every chunk's span and place in it
__device__ __forceinline__ u32 d_group_key(const u32 *__restrict__ chunk, u32 g, u32 RPW)
{
	const u32 slot0 = g * RPW;
	return chunk[slot0 >> 6] * (64u / RPW) + (slot0 & 63u) / RPW;
}

__device__ __forceinline__ int d_dcell(const DGrid &g, int k, float p)
{
	int c = ugrt_floor2i((p - g.lo[k]) * g.inv[k]);
	return d_clampi(c, 0, g.dims[k] - 1);
}

// The walk of DESIGN.md A13, written once: every kernel that walks the grid visits the same cells because it runs these
// float operations (the build is -ffp-contract=off), and the CPU restatements of the tests spell them out independently.
//
// Slab clip of the ray o + t d against the grid box: tenter = the parameter where it enters (0 for an origin inside);
// true = the ray meets the box.
__device__ __forceinline__ bool d_dda_clip(const DGrid &g, const float *o, const float *d, float &tenter)
{
	float texit = 3.0e38f;
	tenter = 0.0f;
#pragma unroll
	for (int k = 0; k < 3; k++) {
		float lo = g.lo[k], hi = g.lo[k] + g.cs[k] * (float)g.dims[k];
		if (d[k] != 0.0f) {
			float inv = 1.0f / d[k];
			float t0 = (lo - o[k]) * inv, t1 = (hi - o[k]) * inv;
			if (t0 > t1) {
				float s = t0;
				t0 = t1;
				t1 = s;
			}
			if (t0 > tenter)
				tenter = t0;
			if (t1 < texit)
				texit = t1;
		} else if (o[k] < lo || o[k] > hi) {
			texit = -1.0f;
		}
	}
	return tenter <= texit;
}

// Start of the walk per axis: the entry cell c, the direction of travel `step`, the parameter tmax at which the ray leaves
// the cell along the axis and its increment per cell, tdelta
__device__ __forceinline__ void d_dda_axes(const DGrid &g, const float *o, const float *d, float tenter, int *c, int *step,
					   float *tmax, float *tdelta)
{
#pragma unroll
	for (int k = 0; k < 3; k++) {
		float pe = o[k] + tenter * d[k];
		c[k] = d_dcell(g, k, pe);
		if (d[k] > 0.0f) {
			step[k] = 1;
			tmax[k] = ((g.lo[k] + (float)(c[k] + 1) * g.cs[k]) - o[k]) / d[k];
			tdelta[k] = g.cs[k] / d[k];
		} else if (d[k] < 0.0f) {
			step[k] = -1;
			tmax[k] = ((g.lo[k] + (float)c[k] * g.cs[k]) - o[k]) / d[k];
			tdelta[k] = -g.cs[k] / d[k];
		} else {
			step[k] = 0;
			tmax[k] = 3.0e38f;
			tdelta[k] = 3.0e38f;
		}
	}
}

// One step: to the neighbour across the nearest cell wall.  tnext = the exit parameter of the cell that is left (the entry
// parameter of the one entered); true = the ray has left the grid, c is no cell any more.
__device__ __forceinline__ bool d_dda_step(const DGrid &g, int *c, const int *step, float *tmax, const float *tdelta, float &tnext)
{
	const int ax = (tmax[0] < tmax[1]) ? ((tmax[0] < tmax[2]) ? 0 : 2) : ((tmax[1] < tmax[2]) ? 1 : 2);
	tnext = ax == 0 ? tmax[0] : (ax == 1 ? tmax[1] : tmax[2]);
	// step along ax (written out: no dynamically indexed registers)
	bool outside;
	if (ax == 0) {
		c[0] += step[0];
		outside = step[0] == 0 || c[0] < 0 || c[0] >= g.dims[0];
		tmax[0] += tdelta[0];
	} else if (ax == 1) {
		c[1] += step[1];
		outside = step[1] == 0 || c[1] < 0 || c[1] >= g.dims[1];
		tmax[1] += tdelta[1];
	} else {
		c[2] += step[2];
		outside = step[2] == 0 || c[2] < 0 || c[2] >= g.dims[2];
		tmax[2] += tdelta[2];
	}
	return outside;
}

// The pixel-major index space of the walks that give a pixel S rays (ugrt_dda_any.hip: the area aims; ugrt_gi.hip).
// Which slot of its group (pix) and which sample (smp) a lane serves: lane / S and lane % S, the quotient by a
// multiplication that is exact for lane < 64 and S <= 32.  They are formed again where they are used, before and behind
// the walk (the lane id is made opaque), so the walk carries no register for them.
__device__ __forceinline__ void d_area_lane(int lane, u32 S, u32 &pix, u32 &smp)
{
	u32 l = (u32)lane;
	asm volatile("" : "+v"(l));
	pix = (l * ((65536u + S - 1u) / S)) >> 16;
	smp = l - pix * S;
}

// The hemisphere rays' basis rule.
// D = (x*T + y*B) + z*n over the normal n: a = the axis of the smallest |n[k]| (strict <, 1 against 0, then 2 against the
// winner: ties go to the lowest k), T = normalize(n x e_a) -- a swizzle with one exact negation --, B = n x T.
__device__ __forceinline__ void d_hemi_dir(const float *n, float x, float y, float z, float *D)
{
	int a = 0;
	float m = __builtin_fabsf(n[0]);
	if (__builtin_fabsf(n[1]) < m) {
		a = 1;
		m = __builtin_fabsf(n[1]);
	}
	if (__builtin_fabsf(n[2]) < m)
		a = 2;
	float T[3], B[3];
	if (a == 0) {
		T[0] = 0.0f;
		T[1] = n[2];
		T[2] = -n[1];
	} else if (a == 1) {
		T[0] = -n[2];
		T[1] = 0.0f;
		T[2] = n[0];
	} else {
		T[0] = n[1];
		T[1] = -n[0];
		T[2] = 0.0f;
	}
	D_NORMALIZE(T);
	D_CROSS(B, n, T);
#pragma unroll
	for (int k = 0; k < 3; k++)
		D[k] = (x * T[k] + y * B[k]) + z * n[k];
}

// Cull of one triangle against a BUNDLE of rays with different origins.  Moller-Trumbore's numerators do
// not change when the origin slides along its ray (A = d.(e2 x tvec), and d.(e2 x d) = 0), so every ray of
// the bundle is represented by the point o' = o + t_in * d where it enters the current cell: the points of
// a bundle then lie within a fraction of a cell of each other.  With the boxes o' in oc +- orad, d in
// dc +- dr:
//     A = d.(e2 x (oc - v0)) + (o' - oc).(d x e2),   |second term| <= sum_k orad_k max|(d x e2)_k|
// and likewise for B (e1 x d) and A + B - det (d x (e2 - e1)), the maxima taken over the direction box; the
// first terms are the interval dot products of the single-origin cull (d_cull_cr).  (Bounding the second term
// by |d| |e2| |o' - oc| instead leaves twice as many triangles for the exact tests.)  The margins cover the rounding of the exact test, whose operands are
// tvec = o - v0 with the ray's own origin: `reach` bounds |o - oc|.  A culled triangle fails the exact
// float test on every ray of the bundle, so results do not change by a bit.
//
// The length of the directions.  ugrt_trace_dda takes directions of any finite length (ugrt.h), and everything the
// margins stand against grows with it.  With s = max_k max|d_k| over the bundle, a = max|tvec_k| (<= max|tc_k| + reach),
// b = max|e1_k|, c = max|e2_k| and u = 2^-24:
//   * the exact test forms A = tvec.(d x e2) from six products d_i e2_j tvec_k of at most s c a, each behind three
//     roundings (the product d_i e2_j, the difference of two of them, the product with tvec_k) and two additions:
//     |error| <= 6 * 5u * s a c < 2^-19 s a c; likewise B (s a b) and det (s b c);
//   * the cull forms the same numbers as n.dc from n = e2 x tc: the same bound with tc for tvec, and what tc differs
//     from the ray's own tvec by is the origin term's (orad) or, for the rounding of o' = o + t_in d itself, at most
//     u |t_in d| <= u reach per component: again u s c reach, inside s a c with a's `reach`.
// So the margins have to be K s a c, K s a b, K s b c: K = 6/65536 = 2^-13.4 leaves 2^5 over the bounds above, as the
// single-origin culls of ugrt_packet.h have for their unit directions (s <= 1 there).  Every number the cull compares
// with a margin is linear in the direction box (dc, dr), so instead of the margins the BOX is scaled: d_beam_box stores
// dc / s and dr / s, and d_cull_beam's K a c against A / s is K s a c against A.  s is wave-uniform: one reciprocal
// per bundle, carried by the box's own halving, nothing per triangle, and no value more to keep (the kernel has no
// scalar register to spare).  s = 1 is kept for shorter directions: 1 / 1 is exact, the box and every decision are
// then bit for bit those of a box that is not scaled, the margins merely wider than needed.  (reach is |t_in d|, a length in space: s
// is multiplied back into it.)  (tests/test_dda_cull_synthetic.py walks directions of length 1e-3 to 1e6.)
// The direction box's absolute floor follows s too: dc = (lo + hi) / 2 and hi - lo round by up to half an ulp of s
// (2^-24 s each), which 1e-6 covers only while s < 16: two adjacent floats lo, hi of magnitude 32 are 3.8e-6 apart,
// dc rounds onto one of them and the half width 0.5 (hi - lo) 1.0001 + 1e-6 = 2.9e-6 no longer reaches the other.
// 1e-6 s is 16 half-ulps of s at least; over s it is 1e-6 against components of at most 1, which
// also covers the reciprocal's and the products' rounding (2^-22.5 together).  (orad's floor is relative already:
// 7.63e-6 = 2^-17 of |o'|.)
struct BeamBox {
	float oc[3], orad[3];
	float dc[3], dr[3]; // the direction box over s = max(1, largest |direction component| of the bundle)
	float reach;        // >= |o - oc|_inf over the bundle
};

__device__ __forceinline__ float d_uniform(float v)
{
	return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

__device__ __forceinline__ BeamBox d_beam_box(const float *o, const float *d, float tin, bool in)
{
	BeamBox bx;
	const float inf = __builtin_huge_valf();
	float on2 = 0.0f, dm2 = 0.0f, s = 1.0f;
	float dlo[3], dhi[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const float p = o[k] + tin * d[k];
		const float lo = d_wave_fmin(in ? p : inf), hi = d_wave_fmax(in ? p : -inf);
		bx.oc[k] = 0.5f * (lo + hi);
		// half width + the distance of the computed o' from the exact point of the ray (a few ulps of |o'|)
		bx.orad[k] = 0.5f * (hi - lo) * 1.0001f + 7.63e-6f * fmaxf(fabsf(lo), fabsf(hi)) + 1e-6f;
		on2 += bx.orad[k] * bx.orad[k];
		dlo[k] = d_wave_fmin(in ? d[k] : inf);
		dhi[k] = d_wave_fmax(in ? d[k] : -inf);
		s = fmaxf(s, fmaxf(fabsf(dlo[k]), fabsf(dhi[k])));
	}
	// the direction box over s: the halving carries the division (h = 0.5 for s == 1: the box as it always was)
	const float h = 0.5f * __builtin_amdgcn_rcpf(s);
#pragma unroll
	for (int k = 0; k < 3; k++) {
		bx.dc[k] = h * (dlo[k] + dhi[k]);
		bx.dr[k] = h * (dhi[k] - dlo[k]) * 1.0001f + 1e-6f;
		const float da = fabsf(bx.dc[k]) + bx.dr[k];
		dm2 += da * da;
	}
	const float tmax = d_wave_fmax(in ? tin : 0.0f);
	// (reach is a length in space: the directions' own length goes back into it)
	const float on = __builtin_sqrtf(on2) * 1.0001f, dmax = __builtin_sqrtf(dm2) * 1.0001f * s;
	bx.reach = (tmax * dmax + on) * 1.001f;
	// uniform values: keep them in scalar registers
#pragma unroll
	for (int k = 0; k < 3; k++) {
		bx.oc[k] = d_uniform(bx.oc[k]);
		bx.dc[k] = d_uniform(bx.dc[k]);
		bx.dr[k] = d_uniform(bx.dr[k]);
		bx.orad[k] = d_uniform(bx.orad[k]);
	}
	bx.reach = d_uniform(bx.reach);
	return bx;
}

// true = no ray of the bundle can pass the exact test on triangle {v0, e1, e2}
__device__ __forceinline__ bool d_cull_beam(const float *v0, const float *e1, const float *e2, const BeamBox &bx)
{
#pragma clang fp contract(fast)
	const float tc[3] = { bx.oc[0] - v0[0], bx.oc[1] - v0[1], bx.oc[2] - v0[2] };
	float nA[3], nB[3], nD[3], nC[3];
	D_CROSS(nA, e2, tc);
	D_CROSS(nB, tc, e1);
	D_CROSS(nD, e2, e1);
#pragma unroll
	for (int k = 0; k < 3; k++)
		nC[k] = nA[k] + nB[k] - nD[k];
	const float a = fmaxf(fmaxf(fabsf(tc[0]), fabsf(tc[1])), fabsf(tc[2])) + bx.reach;
	const float b = fmaxf(fmaxf(fabsf(e1[0]), fabsf(e1[1])), fabsf(e1[2]));
	const float c = fmaxf(fmaxf(fabsf(e2[0]), fabsf(e2[1])), fabsf(e2[2]));
	const float K = 6.0f / 65536.0f; // (against numerators over the length of the bundle's directions: d_beam_box)
	const float mA = fmaxf(K * a * c, 1e-25f), mB = fmaxf(K * a * b, 1e-25f), mD = fmaxf(K * b * c, 1e-25f);
	const float Dm = nD[0] * bx.dc[0] + nD[1] * bx.dc[1] + nD[2] * bx.dc[2];
	const float Dr = fabsf(nD[0]) * bx.dr[0] + fabsf(nD[1]) * bx.dr[1] + fabsf(nD[2]) * bx.dr[2];
	if (!(Dm + Dr < 1e15f && Dm - Dr > -1e15f))
		return false;
	// |w . (d x e)| over the boxes of w = o' - oc and d: sum_k orad_k * (|(dc x e)_k| + the spread of d)
#define D_ORIGIN_TERM(E)                                                                                        \
	(bx.orad[0] * (fabsf(bx.dc[1] * E[2] - bx.dc[2] * E[1]) + bx.dr[1] * fabsf(E[2]) + bx.dr[2] * fabsf(E[1])) + \
	 bx.orad[1] * (fabsf(bx.dc[2] * E[0] - bx.dc[0] * E[2]) + bx.dr[2] * fabsf(E[0]) + bx.dr[0] * fabsf(E[2])) + \
	 bx.orad[2] * (fabsf(bx.dc[0] * E[1] - bx.dc[1] * E[0]) + bx.dr[0] * fabsf(E[1]) + bx.dr[1] * fabsf(E[0])))
	const float e21[3] = { e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2] };
	const float Am = nA[0] * bx.dc[0] + nA[1] * bx.dc[1] + nA[2] * bx.dc[2];
	const float Ar = (fabsf(nA[0]) * bx.dr[0] + fabsf(nA[1]) * bx.dr[1] + fabsf(nA[2]) * bx.dr[2] + D_ORIGIN_TERM(e2)) * 1.0001f;
	const float Bm = nB[0] * bx.dc[0] + nB[1] * bx.dc[1] + nB[2] * bx.dc[2];
	const float Br = (fabsf(nB[0]) * bx.dr[0] + fabsf(nB[1]) * bx.dr[1] + fabsf(nB[2]) * bx.dr[2] + D_ORIGIN_TERM(e1)) * 1.0001f;
	const float Cm = nC[0] * bx.dc[0] + nC[1] * bx.dc[1] + nC[2] * bx.dc[2];
	const float Cr = (fabsf(nC[0]) * bx.dr[0] + fabsf(nC[1]) * bx.dr[1] + fabsf(nC[2]) * bx.dr[2] + D_ORIGIN_TERM(e21)) * 1.0001f;
#undef D_ORIGIN_TERM
	const float mC = mA + mB + mD;
	if (Dm - Dr > mD) // det > 0 for every ray of the bundle
		return (Am + Ar < -mA) || (Bm + Br < -mB) || (Cm - Cr > mC);
	if (Dm + Dr < -mD) // det < 0
		return (Am - Ar > mA) || (Bm - Br > mB) || (Cm + Cr < -mC);
	return false;
}

// {v0, e1, e2} of one triangle: the 48-B record, or the gather + the reference's two edge subtractions
template <bool REC>
__device__ __forceinline__ void d_load_record(const float4 *__restrict__ rec, const float *__restrict__ verts,
					      const int *__restrict__ tris, u32 face, float *r9)
{
	if (REC) {
		const float4 a = rec[face * 3 + 0], b = rec[face * 3 + 1], c = rec[face * 3 + 2];
		r9[0] = a.x;
		r9[1] = a.y;
		r9[2] = a.z;
		r9[3] = a.w;
		r9[4] = b.x;
		r9[5] = b.y;
		r9[6] = b.z;
		r9[7] = b.w;
		r9[8] = c.x;
	} else {
		const int f1 = 3 * tris[face * 3 + 0], f2 = 3 * tris[face * 3 + 1], f3 = 3 * tris[face * 3 + 2];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			r9[k] = verts[f1 + k];
			r9[3 + k] = verts[f2 + k] - r9[k];
			r9[6 + k] = verts[f3 + k] - r9[k];
		}
	}
}

#endif
