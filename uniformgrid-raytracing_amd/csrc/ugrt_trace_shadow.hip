// ugrt_trace_shadow.hip -- the shadow tracer (spherical light grid): mod_light_rckernel, light_kernel.cu:52-270
// (cam = LIGHT camera).  The kernels first, then ugrt_trace_shadow as a sequence of host stages.
//
// Which sorted rays the reference traces: chunks [0, traced) = sorted rays [0, M) with
// M = prefix[traced] (or n when every chunk is traced).  Inside that set the grouping of rays is
// free, and so is the order in which a ray meets its cell's triangles: a ray's flag is 1 iff ANY
// triangle of its light cell passes the occlusion test (light_kernel.cu:186-203).  The reference
// gives a block 64 consecutive rays in PIXEL order (spread over the whole cell) and re-stages the
// cell's whole list for every such chunk.  Here, privately to this tracer (d_map / prefix / the
// light grid's arrays are not modified):
//   1. the traced rays of a cell are re-grouped by a Z code of their direction from the light (octahedral map, or
//      the cube's Morton code in 64-bit keys): `beam` rays are a narrow beam, summarised by its direction box (32 B).
//      Where the ray sort was put off (the map is the unsorted one, every ray is traced) the rays of an 8x8-pixel tile
//      that share a light cell are keyed, and sorted, as ONE item with the code of its first ray (FRAGMENTS below; option
//      "shadow_frags" 0, the sorted map, strict chunks, 64-bit keys and "sort_library" 1 key and sort every ray);
//   2. CULL pass, lane = triangle: a wave keeps 64 triangles of a cell in registers (with the
//      ray-independent halves of the interval test) and streams the cell's beam boxes past them;
//      the (beam, triangle) pairs that cannot be ruled out are appended to a list.  Triangles are
//      read once per cell instead of once per chunk;
//   3. the pairs are brought beam by beam, large apparent size first: counted per (beam, size class) bucket in the cull
//      pass, the counts scanned, the triangle ids placed (COUNTED BUCKETS below; option "shadow_pairs" 0: sorted by the
//      project's radix sort, ugrt_sort.hip; option "sort_library" 1: by rocPRIM's), and
//   4. EXACT pass, lane = ray: each beam runs the reference's per-ray test on its own short list.  One wave per
//      item of that list by default; option "shadow_xcd_run" 0 restores persistent waves.
// The cull is conservative with margins far above fp32 rounding, so the flags do not change.
#include <algorithm>
#include <cstdlib>
#include "ugrt_packet.h"
#include "ugrt_rs_hist.h"
#include "ugrt_scan.h"
#ifndef GCHUNK
#define GCHUNK 32u  // beams a cull work item streams past its 64 triangles
#endif

struct GBox { // one beam (re-grouped rays of one light cell)
	float cx, cy, cz; // centre of the direction box
	float rx, ry, rz; // half widths (slightly widened)
	u32 ray_start;    // into the re-grouped ray list
	u32 ray_count;
};

__device__ __forceinline__ u32 d_spread10(u32 v)
{
	v &= 0x3FFu;
	v = (v | (v << 16)) & 0x030000FFu;
	v = (v | (v << 8)) & 0x0300F00Fu;
	v = (v | (v << 4)) & 0x030C30C3u;
	v = (v | (v << 2)) & 0x09249249u;
	return v;
}

__device__ __forceinline__ u32 d_dir_morton(const float *unit)
{
	u32 q[3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		float f = (unit[k] * 0.5f + 0.5f) * 1023.0f;
		f = f > 0.0f ? f : 0.0f; // also drops NaN
		q[k] = f < 1023.0f ? (u32)f : 1023u;
	}
	return d_spread10(q[0]) | (d_spread10(q[1]) << 1) | (d_spread10(q[2]) << 2);
}

// bits 0..15 of v spread to the even bits
__device__ __forceinline__ u32 d_spread16(u32 v)
{
	v &= 0xFFFFu;
	v = (v | (v << 8)) & 0x00FF00FFu;
	v = (v | (v << 4)) & 0x0F0F0F0Fu;
	v = (v | (v << 2)) & 0x33333333u;
	v = (v | (v << 1)) & 0x55555555u;
	return v;
}

// Directions are points of a sphere: an octahedral map sends them to the unit square, whose Z curve
// needs two thirds of the bits of the cube's for the same angular resolution.  nu + nv code bits.
__device__ __forceinline__ u32 d_dir_oct(const float *unit, u32 nu, u32 nv)
{
	const float inv = 1.0f / (fabsf(unit[0]) + fabsf(unit[1]) + fabsf(unit[2]) + 1e-30f);
	float x = unit[0] * inv, y = unit[1] * inv;
	if (unit[2] < 0.0f) {
		const float ox = (1.0f - fabsf(y)) * (x >= 0.0f ? 1.0f : -1.0f);
		const float oy = (1.0f - fabsf(x)) * (y >= 0.0f ? 1.0f : -1.0f);
		x = ox;
		y = oy;
	}
	float fu = (x * 0.5f + 0.5f) * (float)(1u << nu), fv = (y * 0.5f + 0.5f) * (float)(1u << nv);
	fu = fu > 0.0f ? fu : 0.0f; // also drops NaN
	fv = fv > 0.0f ? fv : 0.0f;
	const u32 qu = fu < (float)((1u << nu) - 1u) ? (u32)fu : (1u << nu) - 1u;
	const u32 qv = fv < (float)((1u << nv) - 1u) ? (u32)fv : (1u << nv) - 1u;
	// nu >= nv >= nu - 1: u takes the even bits, so its extra bit is the top bit nu + nv - 1
	return d_spread16(qu) | (d_spread16(qv) << 1);
}

// KEY64: (cell << 30) | 30-bit Z code of the direction in the cube, in a 64-bit key; otherwise
// (cell << mbits) | mbits-bit octahedral code, in a 32-bit key (two radix passes fewer, half the key bytes)
template <bool KEY64>
__global__ __launch_bounds__(WL_THREADS) void k_shadow_keys(CamBlock cam, const float *__restrict__ t_value_list,
							     const float *__restrict__ ray_direction_list,
							     const u32 *__restrict__ d_map, const u32 *__restrict__ prefix,
							     u32 nchunks, u32 traced, u32 n, u32 C,
							     const u32 *__restrict__ span, const float *__restrict__ cmPt,
							     u32 mbits, void *__restrict__ keys, u32 *__restrict__ vals,
							     u32 *__restrict__ zero, u32 nzero,
							     const u32 *__restrict__ nchunks_dev, u32 launch_cap, u32 prefix_cap,
							     u32 *__restrict__ zero2, u32 nzero2, u32 *__restrict__ zero3, u32 nzero3, RsFirst hs)
{
	// (grid-stride: a bounded number of workgroups, which also count the first digit of the sort of these keys --
	// ugrt_rs_hist.h; 64-bit keys go to the library's sort and are not counted)
	__shared__ u32 s_rsh[RS_BINS * RS_PRIV];
	for (u32 z = blockIdx.x * WL_THREADS + threadIdx.x; z < nzero; z += gridDim.x * WL_THREADS)
		zero[z] = 0; // run starts/ends per light cell, written after the sort
	// (the pass's work counters + pair cursor, and the cull pass's output cursors: cleared here instead of by two fills)
	for (u32 z = blockIdx.x * WL_THREADS + threadIdx.x; z < nzero2; z += gridDim.x * WL_THREADS)
		zero2[z] = 0;
	for (u32 z = blockIdx.x * WL_THREADS + threadIdx.x; z < nzero3; z += gridDim.x * WL_THREADS)
		zero3[z] = 0;
	d_rs_zero(s_rsh, hs);
	__syncthreads();
	for (u32 i0 = blockIdx.x * WL_THREADS; i0 < n; i0 += gridDim.x * WL_THREADS) {
	const u32 i = i0 + threadIdx.x;
	u32 key32 = 0;
	if (i < n) {
	if (nchunks_dev) { // the chunk count never went to the host (UGRT_CHUNKS_ON_DEVICE): same rule, here
		nchunks = *nchunks_dev;
		// more chunks than the caller's prefix map holds: the host path refuses that (ugrt_sort_rays_chunks
		// reports it); here nothing past the written entries is read and nothing is traced
		if (nchunks > prefix_cap)
			nchunks = 0;
		const u32 lim = nchunks < launch_cap ? nchunks : launch_cap;
		traced = launch_cap == 0xFFFFFFFFu ? nchunks : (lim ? lim - 1u : 0u);
	}
	const u32 M = traced < nchunks ? prefix[traced] : n;
	const u32 pixel = d_map[i];
	u32 cell = d_map[n + i];
	u32 code = 0;
	if (i >= M) {
		cell = C + 1; // not traced by the reference's launch
	} else if (cell >= C || span[cell] == 0) {
		cell = C; // sentinel cell or empty list: nothing can shadow this ray
	} else {
		float tVal = t_value_list[pixel];
		float rd[3];
		rd[0] = (cmPt[0] + tVal * ray_direction_list[pixel * 3 + 0]) - cam.cc[0];
		rd[1] = (cmPt[1] + tVal * ray_direction_list[pixel * 3 + 1]) - cam.cc[1];
		rd[2] = (cmPt[2] + tVal * ray_direction_list[pixel * 3 + 2]) - cam.cc[2];
		D_NORMALIZE(rd);
		code = KEY64 ? d_dir_morton(rd) : d_dir_oct(rd, (mbits + 1u) / 2u, mbits / 2u);
	}
	if (KEY64)
		((u64 *)keys)[i] = ((u64)cell << 30) | (u64)code;
	else
		((u32 *)keys)[i] = key32 = (cell << mbits) | code;
	vals[i] = pixel;
	} // i < n
	if (!KEY64 && hs.hist)
		d_rs_count(s_rsh, key32 & 0xFFu, i < n);
	} // grid-stride
	__syncthreads();
	d_rs_flush(s_rsh, hs);
}

template <typename K>
__global__ __launch_bounds__(WL_THREADS) void k_shadow_runs(const K *__restrict__ keys, u32 n, u32 shift,
							     u32 *__restrict__ rstart, u32 *__restrict__ rend)
{
	u32 i = blockIdx.x * WL_THREADS + threadIdx.x;
	if (i >= n)
		return;
	u32 c = (u32)(keys[i] >> shift);
	if (i == 0 || (u32)(keys[i - 1] >> shift) != c)
		rstart[c] = i;
	if (i == n - 1 || (u32)(keys[i + 1] >> shift) != c)
		rend[c] = i + 1;
}

// FRAGMENTS (option "shadow_frags", the default where the ray sort is deferred and every chunk is traced).  The sort only
// has to make `beam` consecutive rays of a light cell a narrow beam, and its keys barely tell the rays apart: the rays of
// an 8x8-pixel tile that share a light cell and a block of direction codes (a fragment: 15 rays on average on the
// 1 M-triangle frame) lie next to each other on a surface and get ONE key, (cell << mbits) | code of the fragment's first ray.  The fragments are sorted
// instead of the rays (17 to 90 times fewer items through the same passes), their ray counts scanned, and every fragment
// then writes its rays' pixel ids to its place and, at a cell's first and last fragment, the cell's run bounds: the
// arrays behind this step are the per-ray path's (rstart / rend per light cell in ray units, the pixel ids in (cell, beam)
// order).  Rays that nothing can shadow (sentinel cell, empty list) belong to no fragment and to no run.
// A wave takes a tile: lane l reads entry (ty * 8 + l / 8) * W + tx * 8 + l % 8 of the band's map -- the pixel as well,
// so a map in another order only makes the fragments less coherent.  The tile's live lanes are split with ballots.  A workgroup keeps its fragments in LDS and appends them FRAG_BUF at a time: one add on the cursor per flush
// (10 k adds on one word take 0.12 ms, see PAIR_SEGS).  The flush also counts the first digit of the keys (RsFirst).
// The order of fragments with equal keys follows the order of the flushes and differs from run to run; a ray's flag does
// not depend on the grouping of the traced rays.
// The code is that of the fragment's first ray.  (The normalised mean direction of its rays -- three wave sums per
// fragment -- was measured: the frame was 1.6 % slower with it)
#define FRAG_BUF 1024u
// A light cell is not a compact patch of directions (the reference's cell row multiplies where it should add), so the
// rays of a tile that share a cell may lie far apart as seen from the light, interleaved pixel by pixel: split by cell
// alone, a fragment filed under its first ray's code carries strays into a beam and widens its box (the exact pass staged
// 30 % more candidates on the 1 M-triangle frame; quadrants of the tile did not help).  The tile's rays are therefore
// split by (cell, top FRAG_SPLIT_BITS bits of the ray's OWN code): 12 bits leave the staged candidates 4 % above the
// per-ray sort's with 136 k fragments; all 17 bits bring them level with 206 k fragments and a slower frame.
#ifndef FRAG_SPLIT_BITS
#define FRAG_SPLIT_BITS 12u
#endif
#define FRAG_TILES 2u                                // tiles a wave takes per round
#define FRAG_ROUND (FRAG_TILES * (WL_THREADS / 64u)) // ... and a workgroup
struct FragRec { // (16 bytes: one load)
	u32 tile, mask_lo, mask_hi, pad;
};

__global__ __launch_bounds__(WL_THREADS) void k_shadow_frags(CamBlock cam, const float *__restrict__ t_value_list,
							      const float *__restrict__ ray_direction_list,
							      const u32 *__restrict__ d_map, u32 n, u32 W, u32 C,
							      const u32 *__restrict__ span, const float *__restrict__ cmPt, u32 mbits,
							      u32 *__restrict__ keys, u32 *__restrict__ slots, FragRec *__restrict__ recs,
							      u32 *__restrict__ fw, u32 cap, u32 *__restrict__ status, u32 *__restrict__ report,
							      u32 *__restrict__ zero, u32 nzero, u32 *__restrict__ zero2, u32 nzero2,
							      u32 *__restrict__ zero3, u32 nzero3, RsFirst hs)
{
	__shared__ u32 s_rsh[RS_BINS * RS_PRIV];
	__shared__ u32 s_key[FRAG_BUF], s_tile[FRAG_BUF], s_mlo[FRAG_BUF], s_mhi[FRAG_BUF];
	__shared__ u32 s_cnt, s_base;
	// (the words k_shadow_keys clears: run bounds per light cell, the pass's counters, the cull pass's cursors)
	for (u32 z = blockIdx.x * WL_THREADS + threadIdx.x; z < nzero; z += gridDim.x * WL_THREADS)
		zero[z] = 0;
	for (u32 z = blockIdx.x * WL_THREADS + threadIdx.x; z < nzero2; z += gridDim.x * WL_THREADS)
		zero2[z] = 0;
	for (u32 z = blockIdx.x * WL_THREADS + threadIdx.x; z < nzero3; z += gridDim.x * WL_THREADS)
		zero3[z] = 0;
	d_rs_zero(s_rsh, hs);
	if (threadIdx.x == 0)
		s_cnt = 0;
	__syncthreads();
	const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const u32 ntiles = n >> 6, tilesx = W >> 3;
	// FRAG_BUF fragments of the workgroup go out with one add on the cursor (all threads)
	auto flush = [&]() {
		const u32 cnt = s_cnt;
		if (threadIdx.x == 0)
			s_base = atomicAdd(&fw[0], cnt);
		__syncthreads();
		const u32 base = s_base;
		for (u32 i0 = 0; i0 < cnt; i0 += WL_THREADS) {
			const u32 i = i0 + threadIdx.x;
			const bool ok = i < cnt && base + i < n; // (a fragment holds a ray: there are never more than n)
			u32 key = 0;
			if (ok) {
				key = s_key[i];
				keys[base + i] = key;
				slots[base + i] = base + i;
				FragRec r = { s_tile[i], s_mlo[i], s_mhi[i], 0u };
				recs[base + i] = r;
			}
			if (hs.hist)
				d_rs_count(s_rsh, key & 0xFFu, ok);
		}
		__syncthreads();
		if (threadIdx.x == 0)
			s_cnt = 0;
		__syncthreads();
	};
	// (a wave takes FRAG_TILES tiles a round, their loads side by side: the round is a chain of three dependent loads)
	for (u32 t0 = blockIdx.x * FRAG_ROUND; t0 < ntiles; t0 += gridDim.x * FRAG_ROUND) {
		u32 tile[FRAG_TILES], pixel[FRAG_TILES], cell[FRAG_TILES];
		bool live[FRAG_TILES];
		float rd[FRAG_TILES][3];
#pragma unroll
		for (u32 u = 0; u < FRAG_TILES; u++) {
			tile[u] = t0 + u * (WL_THREADS / 64u) + wave;
			pixel[u] = 0u, cell[u] = C;
			if (tile[u] < ntiles) { // (wave-uniform)
				const u32 ty = tile[u] / tilesx, tx = tile[u] - ty * tilesx;
				const u32 i = (ty * 8u + (lane >> 3)) * W + tx * 8u + (lane & 7u);
				pixel[u] = d_map[i];
				cell[u] = d_map[n + i];
			}
		}
#pragma unroll
		for (u32 u = 0; u < FRAG_TILES; u++)
			live[u] = cell[u] < C && span[cell[u] < C ? cell[u] : 0u] != 0u;
#pragma unroll
		for (u32 u = 0; u < FRAG_TILES; u++) {
			rd[u][0] = rd[u][1] = rd[u][2] = 0.0f;
			if (live[u]) {
				const float tVal = t_value_list[pixel[u]];
				rd[u][0] = (cmPt[0] + tVal * ray_direction_list[pixel[u] * 3 + 0]) - cam.cc[0];
				rd[u][1] = (cmPt[1] + tVal * ray_direction_list[pixel[u] * 3 + 1]) - cam.cc[1];
				rd[u][2] = (cmPt[2] + tVal * ray_direction_list[pixel[u] * 3 + 2]) - cam.cc[2];
			}
		}
#pragma unroll
		for (u32 u = 0; u < FRAG_TILES; u++) {
			unsigned long long left = __ballot(live[u]), mine = 0ull;
			if (left == 0ull) // (wave-uniform: no live ray, or no tile)
				continue;
			D_NORMALIZE(rd[u]);
			u32 nfrag = 0, rank = 0;
			const u32 code = d_dir_oct(rd[u], (mbits + 1u) / 2u, mbits / 2u);
			const u32 sb = FRAG_SPLIT_BITS < mbits ? FRAG_SPLIT_BITS : mbits;
			const u32 part = (cell[u] << sb) | (code >> (mbits - sb)); // (cell, block of the direction code)
			while (left != 0ull) { // 1 to 64 rounds: a fragment per (cell, code block) of the tile
				const u32 lead = (u32)__builtin_ctzll(left);
				const u32 c = (u32)__builtin_amdgcn_readlane((int)part, (int)lead);
				const unsigned long long same = __ballot(live[u] && part == c);
				if (lane == lead) {
					mine = same;
					rank = nfrag;
				}
				nfrag++;
				left &= ~same;
			}
			u32 base = 0;
			if (lane == 0u)
				base = atomicAdd(&s_cnt, nfrag);
			base = (u32)__shfl((int)base, 0);
			if (mine != 0ull) { // the fragment's first lane
				const u32 at = base + rank;
				s_key[at] = (cell[u] << mbits) | code;
				s_tile[at] = tile[u];
				s_mlo[at] = (u32)mine;
				s_mhi[at] = (u32)(mine >> 32);
			}
		}
		__syncthreads();
		if (s_cnt > FRAG_BUF - 64u * FRAG_ROUND) // (the next round adds up to 64 fragments per tile)
			flush();
	}
	if (s_cnt)
		flush();
	d_rs_flush(s_rsh, hs);
	// The last workgroup to get here checks the count against the capacity the launches behind this kernel were made for
	// (the sort, the scan, the expansion) and leaves {cursor, finished workgroups} at zero for the next pass.  Waiting
	// form: the capacity is n, which no count exceeds.  Asynchronous form: an estimate; a count beyond it raises
	// UGRT_STATUS_FRAG_OVERFLOW and no fragment counts (fw[2] = 0): no run, no beam, nothing is traced, the frame is
	// repeated.  The count found goes to the pass's report: the next asynchronous pass is sized by it.
	if (threadIdx.x == 0) {
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (this thread's adds on the cursor have been acknowledged)
		if (atomicAdd(&fw[1], 1u) == gridDim.x - 1u) {
			const u32 F = atomicExch(&fw[0], 0u);
			fw[1] = 0u;
			fw[2] = F <= cap ? F : 0u;
			report[3] = F;
			if (F > cap)
				atomicOr(status, UGRT_STATUS_FRAG_OVERFLOW);
		}
	}
}

// rays per sorted fragment, formed where their scan loads them (ugrt_scan.h); count: the checked fragment count
struct FragCountLoad {
	const u32 *slots;
	const FragRec *recs;
	const u32 *count;
	__device__ __forceinline__ void operator()(u32 base, u32 n, u32 (&v)[SC_ITEMS]) const
	{
		const u32 F = *count;
		u32 s[SC_ITEMS];
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++)
			s[k] = base + (u32)k < F && base + (u32)k < n ? slots[base + (u32)k] : 0xFFFFFFFFu;
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++) {
			u32 x = 0;
			if (s[k] != 0xFFFFFFFFu) {
				const FragRec r = recs[s[k]];
				x = (u32)__popc(r.mask_lo) + (u32)__popc(r.mask_hi);
			}
			v[k] = x;
		}
	}
};

// EXPANSION: sorted fragment j writes its rays' pixel ids to ray_pixels[incl[j] - rays(j) ...], in lane order, and the run
// bounds of its cell where its neighbour's cell differs.  A wave takes FRAG_PER_WAVE fragments: their records are loaded
// by as many lanes side by side, then the fragments are written out one after the other by all lanes, with nothing
// between their loads of the map.
#define FRAG_PER_WAVE 16u
__global__ __launch_bounds__(WL_THREADS) void k_shadow_expand(const u32 *__restrict__ skeys, const u32 *__restrict__ slots,
							       const FragRec *__restrict__ recs, const u32 *__restrict__ incl,
							       const u32 *__restrict__ count, u32 mbits, const u32 *__restrict__ d_map, u32 n, u32 W,
							       u32 *__restrict__ ray_pixels, u32 *__restrict__ rstart, u32 *__restrict__ rend)
{
	const u32 F = *count; // (checked)
	const u32 lane = threadIdx.x & 63u;
	const u32 tilesx = W >> 3;
	const u32 nwaves = gridDim.x * (WL_THREADS / 64u);
	for (u32 j0 = (blockIdx.x * (WL_THREADS / 64u) + (threadIdx.x >> 6)) * FRAG_PER_WAVE; j0 < F; j0 += nwaves * FRAG_PER_WAVE) {
		u32 tile = 0, mlo = 0, mhi = 0, first = 0;
		const u32 j = j0 + lane;
		if (lane < FRAG_PER_WAVE && j < F) {
			const FragRec r = recs[slots[j]];
			const u32 end = incl[j], c = skeys[j] >> mbits;
			tile = r.tile, mlo = r.mask_lo, mhi = r.mask_hi;
			first = end - ((u32)__popc(mlo) + (u32)__popc(mhi));
			if (j == 0u || (skeys[j - 1u] >> mbits) != c)
				rstart[c] = first;
			if (j == F - 1u || (skeys[j + 1u] >> mbits) != c)
				rend[c] = end;
		}
#pragma unroll
		for (u32 k = 0; k < FRAG_PER_WAVE; k++) {
			// (lanes without a fragment hold an empty mask)
			const u32 t = (u32)__builtin_amdgcn_readlane((int)tile, (int)k);
			const u32 lo = (u32)__builtin_amdgcn_readlane((int)mlo, (int)k), hi = (u32)__builtin_amdgcn_readlane((int)mhi, (int)k);
			const u32 at = (u32)__builtin_amdgcn_readlane((int)first, (int)k);
			const unsigned long long mask = ((unsigned long long)hi << 32) | lo;
			if ((mask >> lane) & 1ull) {
				const u32 ty = t / tilesx, tx = t - ty * tilesx;
				const u32 i = (ty * 8u + (lane >> 3)) * W + tx * 8u + (lane & 7u);
				const u32 to = at + (u32)__popcll(mask & ((1ull << lane) - 1ull));
				if (i < n && to < n)
					ray_pixels[to] = d_map[i];
			}
		}
	}
}

// per light cell: number of beams (ITEMS = false), or number of cull items = triangle batches x beam chunks -- formed
// where the scans of these counts load them (ugrt_scan.h)
struct ShadowCountLoad {
	const u32 *span, *rstart, *rend;
	u32 beam;
	unsigned long long *tests;
	bool ITEMS;
	__device__ __forceinline__ void operator()(u32 base, u32 C, u32 (&v)[SC_ITEMS]) const
	{
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++) {
			const u32 c = base + (u32)k;
			u32 x = 0;
			if (c < C) {
				const u32 g = (rend[c] - rstart[c] + beam - 1u) / beam, sp = span[c];
				x = ITEMS ? (sp + 63u) / 64u * ((g + GCHUNK - 1) / GCHUNK) : g;
				if (!ITEMS && g && sp)
					atomicAdd(tests, (unsigned long long)sp * (unsigned long long)g); // cells that matter are few
			}
			v[k] = x;
		}
	}
};

// smallest c with incl[c] > x (incl = inclusive scan over C cells, x < incl[C-1])
__device__ __forceinline__ u32 d_find_cell(const u32 *__restrict__ incl, u32 C, u32 x)
{
	u32 lo = 0, hi = C - 1;
	while (lo < hi) {
		u32 mid = (lo + hi) >> 1;
		if (incl[mid] > x)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}

// The same for a wave-uniform x with all 64 lanes probing at once: 64-ary instead of binary, three dependent
// loads for 16 k cells instead of fourteen.
__device__ __forceinline__ u32 d_find_cell_wave(const u32 *__restrict__ incl, u32 C, u32 x, int lane)
{
	u32 lo = 0, n = C; // the answer lies in [lo, lo + n) and incl[lo + n - 1] > x
	while (n > 1u) {
		const u32 stride = (n + 63u) / 64u;
		u32 idx = lo + ((u32)lane + 1u) * stride - 1u;
		idx = idx < lo + n - 1u ? idx : lo + n - 1u;
		const unsigned long long above = __ballot(incl[idx] > x);
		const u32 f = (u32)__builtin_ctzll(above);
		const u32 nlo = lo + f * stride;
		const u32 left = lo + n - nlo;
		lo = nlo;
		n = stride < left ? stride : left;
	}
	return lo;
}

// the rays of a beam, as the reference rebuilds them (light_kernel.cu:166-184)
struct ShadowRay {
	float rd[3];
	float distance_b;
	int pixel;
};

__device__ __forceinline__ ShadowRay d_shadow_ray(const CamBlock &cam, const float *__restrict__ t_value_list,
						  const float *__restrict__ ray_direction_list, const float *cm, int pixel)
{
	ShadowRay r;
	const float lx = cam.cc[0], ly = cam.cc[1], lz = cam.cc[2];
	float tVal = t_value_list[pixel];
	float pI[3];
	pI[0] = cm[0] + tVal * ray_direction_list[pixel * 3 + 0];
	pI[1] = cm[1] + tVal * ray_direction_list[pixel * 3 + 1];
	pI[2] = cm[2] + tVal * ray_direction_list[pixel * 3 + 2];
	r.rd[0] = pI[0] - lx;
	r.rd[1] = pI[1] - ly;
	r.rd[2] = pI[2] - lz;
	// isSmaller's distance_b (light_kernel.cu:6) depends on the ray only
	r.distance_b = __builtin_sqrtf((pI[0] - lx) * (pI[0] - lx) + (pI[1] - ly) * (pI[1] - ly) +
				       (pI[2] - lz) * (pI[2] - lz));
	D_NORMALIZE(r.rd);
	r.pixel = pixel;
	return r;
}

// one workgroup of four waves per beam (`beam` re-grouped rays of one light cell): direction box of its rays.  The
// waves take the beam's 64-ray runs in turn and keep per-lane minima and maxima; the lanes are folded once at the end
// (one wave and a wave reduction per run took 49 us beside other frames once the beams were 2048 rays long).
#define BOX_WAVES 4
struct CullItem;
// the cull pass's item table, written by the same launch (defined with the items below)
__device__ void d_cull_items_fill(const u32 *__restrict__ iincl, const u32 *__restrict__ gincl, const u32 *__restrict__ span,
				  const u32 *__restrict__ offset, u32 C, CullItem *__restrict__ items, u32 first, u32 stride);
__global__ __launch_bounds__(64 * BOX_WAVES) void k_shadow_boxes(CamBlock cam, const u32 *__restrict__ gincl, u32 C,
						     const u32 *__restrict__ rstart, const u32 *__restrict__ rend,
						     const u32 *__restrict__ ray_pixels, const float *__restrict__ t_value_list,
						     const float *__restrict__ ray_direction_list,
						     const float *__restrict__ cmPt, GBox *__restrict__ boxes, u32 beam,
						     u32 *__restrict__ zero, u32 nzero, float4 *__restrict__ sray,
						     const u32 *__restrict__ iincl, const u32 *__restrict__ span,
						     const u32 *__restrict__ offset, CullItem *__restrict__ citems,
						     u32 *__restrict__ bkt, u32 bkt_words, u32 sbits)
{
	__shared__ float s_box[BOX_WAVES][6];
	for (u32 z = blockIdx.x * (64u * BOX_WAVES) + threadIdx.x; z < nzero; z += gridDim.x * (64u * BOX_WAVES))
		zero[z] = 0; // candidate run starts/ends per beam, written after the pair sort
	// (the cull pass's items depend on the same two scans as the boxes: listed here instead of by a launch of their own)
	d_cull_items_fill(iincl, gincl, span, offset, C, citems, blockIdx.x * (64u * BOX_WAVES) + threadIdx.x, gridDim.x * (64u * BOX_WAVES));
	const u32 total = gincl[C - 1];
	if (bkt) { // counted candidate buckets: the (beam, size class) counters the cull pass adds to, for the beams there are
		const unsigned long long used = (unsigned long long)total << sbits;
		const u32 nb = used < bkt_words ? (u32)used : bkt_words;
		for (u32 z = blockIdx.x * (64u * BOX_WAVES) + threadIdx.x; z < nb; z += gridDim.x * (64u * BOX_WAVES))
			bkt[z] = 0;
	}
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const float cm[3] = { cmPt[0], cmPt[1], cmPt[2] };
	const float inf = __builtin_huge_valf();
	for (u32 g = blockIdx.x; g < total; g += gridDim.x) {
		const u32 c = d_find_cell(gincl, C, g);
		const u32 ngrp = (rend[c] - rstart[c] + beam - 1u) / beam;
		const u32 j = g - (gincl[c] - ngrp);
		const u32 start = rstart[c] + beam * j;
		const u32 left = rend[c] - start;
		const u32 cnt = left < beam ? left : beam;
		float lo[3] = { inf, inf, inf }, hi[3] = { -inf, -inf, -inf };
		for (u32 b = 64u * (u32)wave; b < cnt; b += 64u * BOX_WAVES) {
			if (b + (u32)lane < cnt) {
				ShadowRay r =
					d_shadow_ray(cam, t_value_list, ray_direction_list, cm, (int)ray_pixels[start + b + lane]);
				// the rebuilt ray, in beam order: the exact pass reads 64 of them as one 1-KB run instead of
				// gathering t and direction per pixel for every (segment, sub-group) item again
				sray[start + b + lane] = make_float4(r.rd[0], r.rd[1], r.rd[2], r.distance_b);
#pragma unroll
				for (int k = 0; k < 3; k++) {
					lo[k] = fminf(lo[k], r.rd[k]);
					hi[k] = fmaxf(hi[k], r.rd[k]);
				}
			}
		}
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const float l = d_wave_fmin(lo[k]), h = d_wave_fmax(hi[k]);
			if (lane == 0) {
				s_box[wave][k] = l;
				s_box[wave][3 + k] = h;
			}
		}
		__syncthreads();
		if (threadIdx.x == 0) {
#pragma unroll
			for (int k = 0; k < 3; k++) {
				lo[k] = s_box[0][k];
				hi[k] = s_box[0][3 + k];
				for (int w = 1; w < BOX_WAVES; w++) {
					lo[k] = fminf(lo[k], s_box[w][k]);
					hi[k] = fmaxf(hi[k], s_box[w][3 + k]);
				}
			}
			GBox o;
			o.cx = 0.5f * (lo[0] + hi[0]);
			o.cy = 0.5f * (lo[1] + hi[1]);
			o.cz = 0.5f * (lo[2] + hi[2]);
			// half widths, widened by far more than the rounding of centre and width
			o.rx = 0.5f * (hi[0] - lo[0]) + 1e-6f;
			o.ry = 0.5f * (hi[1] - lo[1]) + 1e-6f;
			o.rz = 0.5f * (hi[2] - lo[2]) + 1e-6f;
			o.ray_start = start;
			o.ray_count = cnt;
			boxes[g] = o;
		}
		__syncthreads();
	}
}

#define PAIR_BUF 512u

__device__ __forceinline__ void d_flush_pairs(const u32 *buf_beam, const u32 *buf_tri, u32 nbuf, int lane,
					      u32 *__restrict__ pair_count, u32 pair_cap, u32 *__restrict__ pair_beam,
					      u32 *__restrict__ pair_tri)
{
	__syncthreads(); // single-wave block: orders the LDS writes before the reads below
	u32 base = 0;
	if (lane == 0)
		base = atomicAdd(pair_count, nbuf);
	base = __shfl(base, 0);
	for (u32 i = (u32)lane; i < nbuf; i += 64u)
		if (base + i < pair_cap) {
			pair_beam[base + i] = buf_beam[i];
			pair_tri[base + i] = buf_tri[i];
		}
	__syncthreads();
}

// The cull pass appends its pairs through PAIR_SEGS cursors instead of one: every wave ends with an append, and 10 k
// atomics on ONE word take 12 ns each -- 0.12 ms, the whole kernel (per-wave cycle stamps: a third of a wave's time
// went by in the appends).  Wave w appends to segment w % PAIR_SEGS of the staging arrays (cursors 256 B apart);
// k_pair_compact then moves the segments together and leaves the total where the single cursor used to be.  A segment
// that ran over reports a total that no buffer of this size could hold, so the caller's overflow handling applies.
#define PAIR_SEGS 64u
#define PAIR_SEG_STRIDE 64u // words between two cursors

// asynchronous shadow pass: the counts of the cull pass against the capacities the later launches were sized for
// (pg == nullptr: the waiting form, which reads the counts back instead)
struct PairCheck {
	const u32 *gcount;
	u32 cap, gbound;
	u32 *pg, *status, *report;
};

__global__ __launch_bounds__(256) void k_pair_compact(const u32 *__restrict__ segcnt, u32 segcap,
						       const u32 *__restrict__ sbeam, const u32 *__restrict__ stri,
						       u32 *__restrict__ pair_beam, u32 *__restrict__ pair_tri,
						       u32 *__restrict__ pair_count, PairCheck chk, RsFirst hs)
{
	__shared__ u32 s_cnt[PAIR_SEGS], s_base[PAIR_SEGS];
	__shared__ u32 s_over;
	__shared__ u32 s_rsh[RS_BINS * RS_PRIV]; // first digit of the pair sort that follows (ugrt_rs_hist.h)
	if (threadIdx.x == 0)
		s_over = 0u;
	d_rs_zero(s_rsh, hs);
	__syncthreads();
	if (threadIdx.x < PAIR_SEGS) {
		const u32 c = segcnt[threadIdx.x * PAIR_SEG_STRIDE];
		if (c > segcap)
			atomicMax(&s_over, c);
		s_cnt[threadIdx.x] = c < segcap ? c : segcap;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		u32 acc = 0;
		for (u32 k = 0; k < PAIR_SEGS; k++) {
			s_base[k] = acc;
			acc += s_cnt[k];
		}
		if (blockIdx.x == 0) {
			const unsigned long long worst = (unsigned long long)s_over * PAIR_SEGS;
			u32 P = s_over ? (worst > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (u32)worst) : acc;
			pair_count[0] = P;
			if (chk.pg) {
				const u32 G = *chk.gcount;
				chk.report[0] = P;
				chk.report[1] = G;
				if (P > chk.cap || G > chk.gbound) {
					atomicOr(chk.status, UGRT_STATUS_PAIR_OVERFLOW);
					P = 0; // nothing is traced: the frame is reported as incomplete
				}
				chk.pg[0] = P;
				chk.pg[1] = G;
			}
		}
	}
	__syncthreads();
	const u32 seg = blockIdx.x % PAIR_SEGS, part = blockIdx.x / PAIR_SEGS, parts = gridDim.x / PAIR_SEGS;
	const u32 n = s_cnt[seg], base = s_base[seg];
	const size_t src = (size_t)seg * segcap;
	for (u32 i0 = part * 256u; i0 < n; i0 += parts * 256u) {
		const u32 i = i0 + threadIdx.x;
		u32 key = 0;
		if (i < n) {
			key = sbeam[src + i];
			pair_beam[base + i] = key;
			pair_tri[base + i] = stri[src + i];
		}
		if (hs.hist)
			d_rs_count(s_rsh, key & 0xFFu, i < n);
	}
	__syncthreads();
	d_rs_flush(s_rsh, hs);
}

// A cull item = (light cell, batch of 64 of its triangles, chunk of GCHUNK of its beams), as the kernel needs it:
// where the batch's ids start, how many there are, the first beam box and the number of boxes.
struct CullItem {
	u32 ref_base, cnt, gfirst, gcount;
};

__device__ __forceinline__ CullItem d_cull_item(const u32 *__restrict__ iincl, const u32 *__restrict__ gincl,
						 const u32 *__restrict__ span, const u32 *__restrict__ offset, u32 C, u32 it)
{
	const u32 c = d_find_cell(iincl, C, it);
	const u32 sp = span[c];
	const u32 nb = (sp + 63u) / 64u;
	const u32 ngrp = gincl[c] - (c ? gincl[c - 1] : 0u);
	const u32 gbase = gincl[c] - ngrp;
	const u32 nq = (ngrp + GCHUNK - 1) / GCHUNK;
	const u32 local = it - (iincl[c] - nb * nq);
	const u32 j = local / nq, q = local % nq;
	const u32 first = 64u * j, g0 = q * GCHUNK;
	CullItem d;
	d.ref_base = offset[c] + first;
	d.cnt = (sp - first) < 64u ? (sp - first) : 64u;
	d.gfirst = gbase + g0;
	d.gcount = ((g0 + GCHUNK) < ngrp ? (g0 + GCHUNK) : ngrp) - g0;
	return d;
}

// The items as a table (the first CULL_TABLE of them; the bench frame has 27 k): the kernel reads an item with one
// scalar load instead of a search and four dependent loads at the head of every item
#define CULL_TABLE (1u << 20)
__device__ void d_cull_items_fill(const u32 *__restrict__ iincl, const u32 *__restrict__ gincl, const u32 *__restrict__ span,
				  const u32 *__restrict__ offset, u32 C, CullItem *__restrict__ items, u32 first, u32 stride)
{
	const u32 total = iincl[C - 1] < CULL_TABLE ? iincl[C - 1] : CULL_TABLE;
	for (u32 it = first; it < total; it += stride)
		items[it] = d_cull_item(iincl, gincl, span, offset, C, it);
}

// CULL pass, lane = triangle.  Same test as d_cull with the box as centre +- half width: f(d) = n.d ranges over
// n.c -+ sum_k |n_k| r_k.  A wave takes its items in a fixed stride, so it knows the ones to come: an item's
// descriptor is requested three items ahead, the ids of its triangles two, their records one -- the head of an item
// was a chain of five dependent loads (25 k cycles, half of the kernel, for 15 beam iterations on average:
// per-wave cycle stamps).
template <bool REC>
__global__ __launch_bounds__(64) void k_shadow_cull(CamBlock cam, const u32 *__restrict__ iincl, const u32 *__restrict__ gincl,
						    u32 C, const u32 *__restrict__ span, const u32 *__restrict__ offset,
						    const u32 *__restrict__ value_list, const float4 *__restrict__ rec,
						    const float *__restrict__ verts, const int *__restrict__ tris,
						    const GBox *__restrict__ boxes, u32 *__restrict__ pair_count, u32 pair_cap,
						    u32 *__restrict__ pair_beam, u32 *__restrict__ pair_tri, u32 sbits,
						    const CullItem *__restrict__ table, u32 *__restrict__ bkt, u32 gbound)
{
#pragma clang fp contract(fast) // cull arithmetic only (conservative by margin); no exact test in this kernel
	// candidate pairs are staged in LDS and flushed PAIR_BUF at a time: one atomic on the shared
	// output cursor per ~450 pairs instead of one per beam iteration
	__shared__ u32 buf_beam[PAIR_BUF], buf_tri[PAIR_BUF];
	u32 nbuf = 0; // wave-uniform
	{ // this wave's segment of the staging arrays (pair_cap = capacity of ONE segment)
		const u32 seg = blockIdx.x % PAIR_SEGS;
		pair_count += seg * PAIR_SEG_STRIDE;
		pair_beam += (size_t)seg * pair_cap;
		pair_tri += (size_t)seg * pair_cap;
	}
	const u32 total = iincl[C - 1];
	const int lane = threadIdx.x;
	const float lx = cam.cc[0], ly = cam.cc[1], lz = cam.cc[2];
	const u32 stride = gridDim.x;
	u32 it = d_xcd_block();
	// An item costs between 1 and GCHUNK beam iterations and the cost changes slowly along the list (cell by
	// cell), so neighbouring waves -- the eight of a SIMD -- would all hold cheap or all hold expensive items,
	// and the SIMDs with the expensive ones set the kernel's time (slowest wave 1.85 x the mean).  The waves'
	// first items are therefore dealt out through a multiplicative permutation of the wave index.
	if ((stride & (stride - 1u)) == 0u)
		it = (it * 40503u) & (stride - 1u);
	if (it >= total)
		return;
	// (items past the end read as empty; their loads go to the first id and its record)
	auto item_at = [&](u32 i) -> CullItem {
		CullItem d = { 0u, 0u, 0u, 0u };
		if (i < total)
			d = i < CULL_TABLE ? table[i] : d_cull_item(iincl, gincl, span, offset, C, i);
		return d;
	};
	auto id_of = [&](const CullItem &d) -> u32 {
		const u32 l = (u32)lane < d.cnt ? (u32)lane : (d.cnt ? d.cnt - 1u : 0u);
		return value_list[d.ref_base + l];
	};
	CullItem d_cur = item_at(it), d_1 = item_at(it + stride), d_2 = item_at(it + 2u * stride);
	u32 id_cur = id_of(d_cur), id_1 = id_of(d_1);
	float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
	float rcx = 0.f;
	if (REC) {
		ra = rec[id_cur * 3u + 0u];
		rb = rec[id_cur * 3u + 1u];
		rcx = reinterpret_cast<const float *>(rec)[id_cur * 12u + 8u];
	}
	for (;;) {
		const bool have = (u32)lane < d_cur.cnt;
		const u32 face = id_cur;
		float t9[9];
		if (REC) {
			t9[0] = lx - ra.x, t9[1] = ly - ra.y, t9[2] = lz - ra.z;
			t9[3] = ra.w, t9[4] = rb.x, t9[5] = rb.y, t9[6] = rb.z, t9[7] = rb.w, t9[8] = rcx;
			// the loads of the items to come
			ra = rec[id_1 * 3u + 0u];
			rb = rec[id_1 * 3u + 1u];
			rcx = reinterpret_cast<const float *>(rec)[id_1 * 12u + 8u];
		} else {
			d_load_triangle<REC>(rec, verts, tris, face, lx, ly, lz, t9);
		}
		id_cur = id_1;
		id_1 = id_of(d_2);
		const CullItem d_3 = item_at(it + 3u * stride);
		float nA[3], nB[3], nD[3], nC[3];
		float mA, mB, mD;
		u32 code;
		{
			const float *tv = &t9[0], *e1 = &t9[3], *e2 = &t9[6];
			D_CROSS(nA, e2, tv);
			D_CROSS(nB, tv, e1);
			D_CROSS(nD, e2, e1);
#pragma unroll
			for (int k = 0; k < 3; k++)
				nC[k] = nA[k] + nB[k] - nD[k];
			const float a = fmaxf(fmaxf(fabsf(tv[0]), fabsf(tv[1])), fabsf(tv[2]));
			const float b = fmaxf(fmaxf(fabsf(e1[0]), fabsf(e1[1])), fabsf(e1[2]));
			const float cc = fmaxf(fmaxf(fabsf(e2[0]), fabsf(e2[1])), fabsf(e2[2]));
			const float K = 6.0f / 65536.0f;
			mA = fmaxf(K * a * cc, 1e-25f);
			mB = fmaxf(K * a * b, 1e-25f);
			mD = fmaxf(K * b * cc, 1e-25f);
			// apparent size from the light, large first: the exact pass stops a ray at its first occluder
			const float sa = __builtin_sqrtf(D_DOT(nD, nD)) / (D_DOT(tv, tv) + 1e-30f);
			float lc = (__log2f(sa + 1e-30f) + 30.0f) * 5.0f;
			lc = lc < 0.0f ? 0.0f : (lc > 255.0f ? 255.0f : lc);
			code = (255u - (u32)lc) >> (8u - sbits);
		}
		const float mC = mA + mB + mD;
		const u32 g0 = d_cur.gfirst, g1 = d_cur.gfirst + d_cur.gcount;
		GBox nxt = boxes[g0]; // wave-uniform address: scalar loads
		unsigned long long cls = 0ull; // counted buckets: the lanes of this lane's size class, and whether it is their first
		bool cls_first = false, cls_ready = false;
		for (u32 g = g0; g < g1; g++) {
			const GBox bx = nxt;
			// the next beam's box is requested before this one is used: its latency hides behind the test
			nxt = boxes[(g + 1 < g1) ? g + 1 : g];
			bool keep = false;
			if (have) {
				const float Dm = nD[0] * bx.cx + nD[1] * bx.cy + nD[2] * bx.cz;
				const float Dr = fabsf(nD[0]) * bx.rx + fabsf(nD[1]) * bx.ry + fabsf(nD[2]) * bx.rz;
				const float Am = nA[0] * bx.cx + nA[1] * bx.cy + nA[2] * bx.cz;
				const float Ar = fabsf(nA[0]) * bx.rx + fabsf(nA[1]) * bx.ry + fabsf(nA[2]) * bx.rz;
				const float Bm = nB[0] * bx.cx + nB[1] * bx.cy + nB[2] * bx.cz;
				const float Br = fabsf(nB[0]) * bx.rx + fabsf(nB[1]) * bx.ry + fabsf(nB[2]) * bx.rz;
				const float Cm = nC[0] * bx.cx + nC[1] * bx.cy + nC[2] * bx.cz;
				const float Cr = fabsf(nC[0]) * bx.rx + fabsf(nC[1]) * bx.ry + fabsf(nC[2]) * bx.rz;
				keep = !d_cull_decide(Dm, Dr, Am, Ar, Bm, Br, Cm, Cr, mA, mB, mD, mC);
			}
			const unsigned long long mask = __ballot(keep);
			if (mask != 0ull) {
				if (keep) {
					const u32 pos = nbuf + d_rank_in_mask(mask);
					buf_beam[pos] = (g << sbits) | code;
					buf_tri[pos] = face;
				}
				nbuf += (u32)__popcll(mask);
				// counted buckets (bkt): the kept lanes of each size class present, added to the beam's counter of that class
				// by the class's first lane -- nothing comes back, the wave does not wait.  (beams past the bound the table
				// was made for, asynchronous form: the pass is reported as overflowed and nothing is placed)
				if (bkt && g < gbound) {
					// (a lane's class is the same for every beam of the item: the lanes are sorted into their classes once
					// per item, at its first kept pair -- a scalar loop of 1-3 rounds -- and a beam then costs the classes'
					// first lanes a population count and an add)
					if (!cls_ready) {
						cls_ready = true;
						unsigned long long left = __ballot(have);
						while (left != 0ull) {
							const u32 lc = (u32)__builtin_amdgcn_readlane((int)code, (int)__builtin_ctzll(left));
							const unsigned long long same = __ballot(have && code == lc);
							if (have && code == lc) {
								cls = same;
								cls_first = lane == (int)__builtin_ctzll(same);
							}
							left &= ~same;
						}
					}
					if (cls_first) {
						const u32 kept = (u32)__popcll(mask & cls);
						if (kept)
							atomicAdd(&bkt[(g << sbits) | code], kept);
					}
				}
				if (nbuf > PAIR_BUF - 64u) {
					d_flush_pairs(buf_beam, buf_tri, nbuf, lane, pair_count, pair_cap, pair_beam, pair_tri);
					nbuf = 0;
				}
			}
		}
		it += stride;
		if (it >= total)
			break;
		d_cur = d_1;
		d_1 = d_2;
		d_2 = d_3;
	}
	if (nbuf)
		d_flush_pairs(buf_beam, buf_tri, nbuf, lane, pair_count, pair_cap, pair_beam, pair_tri);
}

// (pg: {candidate pairs, beams} on the device when the host does not know them - the asynchronous form; the launch
// is then sized by an estimate and strides)
__global__ __launch_bounds__(WL_THREADS) void k_pair_runs(const u32 *__restrict__ beam, u32 P, u32 sbits,
							   u32 *__restrict__ pstart, u32 *__restrict__ pend,
							   const u32 *__restrict__ pg)
{
	if (pg)
		P = pg[0];
	for (u32 i = blockIdx.x * WL_THREADS + threadIdx.x; i < P; i += gridDim.x * WL_THREADS) {
		u32 b = beam[i] >> sbits;
		if (i == 0 || (beam[i - 1] >> sbits) != b)
			pstart[b] = i;
		if (i == P - 1 || (beam[i + 1] >> sbits) != b)
			pend[b] = i + 1;
	}
}


// an item with segment number XSEG_LAST takes all the remaining candidates of its beam (the segment is
// the 8-bit sort key of the item list; XSEG_LAST + 1 marks the padding behind the last item)
#define XSEG_LAST 254u
// items per beam, formed where the scan of the counts loads them (ugrt_scan.h; it runs over the capacity Gcap)
struct PairItemLoad {
	const u32 *pstart, *pend;
	const GBox *boxes;
	u32 G;
	unsigned long long *staged;
	u32 XSEG;
	const u32 *pg;
	__device__ __forceinline__ void operator()(u32 base, u32 Gcap, u32 (&v)[SC_ITEMS]) const
	{
		const u32 Gn = pg ? (pg[0] ? pg[1] : 0u) : G; // (no pairs: no items)
		unsigned long long mine = 0;
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++) {
			const u32 g = base + (u32)k;
			u32 x = 0;
			if (g < Gn && g < Gcap) {
				const u32 cand = pend[g] - pstart[g], nsub = (boxes[g].ray_count + 63u) / 64u;
				const u32 nseg = (cand + XSEG - 1) / XSEG;
				x = (nseg < XSEG_LAST + 1u ? nseg : XSEG_LAST + 1u) * nsub;
				mine += (unsigned long long)cand * nsub;
			}
			v[k] = x;
		}
		// candidates staged by the exact pass (work accounting): one atomic per wave
#pragma unroll
		for (int m = 32; m >= 1; m >>= 1)
			mine += __shfl_xor(mine, m);
		if ((threadIdx.x & 63) == 0 && mine)
			atomicAdd(staged, mine);
	}
};

// The exact-pass items, listed once (the tracer then starts with two loads instead of a 12-step search)
// and ordered by SEGMENT first: all beams' first segments run before any second segment, so by the time a
// later segment of a beam is picked up its rays have mostly been flagged by the earlier ones and the item
// ends at its first ballot.  key = segment, value = beam << 7 | sub-group.
// (runs as k_pair_items behind the pair sort, or as the workgroups [first, first + blocks) of k_pair_place: there the
// beams' candidate runs are not written yet and are taken from the buckets' inclusive sums `bincl`)
__device__ __forceinline__ void d_pair_items(u32 block, u32 blocks, const u32 *__restrict__ xincl, u32 G, u32 cap,
					     const u32 *__restrict__ pstart, const u32 *__restrict__ pend,
					     const u32 *__restrict__ bincl, u32 sbits, const GBox *__restrict__ boxes, u32 XSEG,
					     u32 *__restrict__ item_seg, u32 *__restrict__ item_sub, u32 *__restrict__ status,
					     RsFirst hs)
{
	// (grid-stride; the workgroups also count the items' 8-bit keys for the sort that follows -- ugrt_rs_hist.h)
	__shared__ u32 s_rsh[RS_BINS * RS_PRIV];
	d_rs_zero(s_rsh, hs);
	__syncthreads();
	const u32 nitems = xincl[G - 1];
	if (status && block == 0 && threadIdx.x == 0 && nitems > cap)
		atomicOr(status, UGRT_STATUS_ITEM_OVERFLOW); // asynchronous form: the list was sized by an estimate
	for (u32 i0 = block * WL_THREADS; i0 < cap; i0 += blocks * WL_THREADS) {
		const u32 it = i0 + threadIdx.x;
		const bool ok = it < cap;
		u32 seg = XSEG_LAST + 1u, sub = 0u; // the list is sorted at its capacity: padding goes last
		if (ok && it < nitems) {
			const u32 g = d_find_cell(xincl, G, it);
			const u32 cand = bincl ? bincl[((g + 1u) << sbits) - 1u] - (g ? bincl[(g << sbits) - 1u] : 0u) : pend[g] - pstart[g];
			u32 nseg = (cand + XSEG - 1) / XSEG;
			nseg = nseg < XSEG_LAST + 1u ? nseg : XSEG_LAST + 1u;
			const u32 nsub = (boxes[g].ray_count + 63u) / 64u;
			const u32 local = it - (xincl[g] - nseg * nsub);
			seg = local / nsub;
			sub = (g << 7) | (local % nsub);
		}
		if (ok) {
			item_seg[it] = seg;
			item_sub[it] = sub;
		}
		if (hs.hist)
			d_rs_count(s_rsh, seg & 0xFFu, ok);
	}
	__syncthreads();
	d_rs_flush(s_rsh, hs);
}

__global__ __launch_bounds__(WL_THREADS) void k_pair_items(const u32 *__restrict__ xincl, u32 G, u32 cap,
							    const u32 *__restrict__ pstart, const u32 *__restrict__ pend,
							    const GBox *__restrict__ boxes, u32 XSEG,
							    u32 *__restrict__ item_seg, u32 *__restrict__ item_sub,
							    u32 *__restrict__ status, RsFirst hs)
{
	d_pair_items(blockIdx.x, gridDim.x, xincl, G, cap, pstart, pend, nullptr, 0u, boxes, XSEG, item_seg, item_sub, status, hs);
}

// COUNTED BUCKETS (option "shadow_pairs", the default).  A ray's flag is 1 iff any triangle of its cell occludes it, and
// the exact pass wants a beam's candidates next to each other, large apparent size first: a bucketing by (beam, size
// class), in which the order inside a bucket is free -- no sort.  The cull pass counts its kept pairs per bucket
// (`bkt`, cleared by k_shadow_boxes), one launch scans the counts (`bincl`, inclusive: bucket k's run ends at bincl[k])
// beside the exact pass's items per beam, and k_pair_place moves every staged triangle id to its bucket's run, taking
// its place from the bucket's counter, which it counts down to zero again.  What k_pair_compact checked is checked
// where the scan loads its input: every wave of the scan forms the pass's {pairs, beams} from the 64 staging cursors
// and the beam count itself (no workgroup waits for another), the launch's first workgroup reports them.
static_assert(PAIR_SEGS == 64u, "a wave sums the staging cursors, one per lane");
#define SHADOW_BUCKET_WORDS (1u << 22) // (beam bound << size bits) up to which the pairs are counted: 16 MB of counters, as much of sums

// {pairs, beams} of the pass and whether they fit what the launches behind the cull pass were made for (cap pairs,
// gbound beams).  A staging segment that ran over makes a total that no buffer holds.  (whole waves only)
__device__ __forceinline__ bool d_pair_totals(const u32 *__restrict__ segcnt, u32 segcap, const u32 *__restrict__ gcount,
					      u32 cap, u32 gbound, u32 *P, u32 *G)
{
	const u32 c = segcnt[(threadIdx.x & 63u) * PAIR_SEG_STRIDE];
	u32 sum = c < segcap ? c : segcap, over = c > segcap ? c : 0u;
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) {
		sum += (u32)__shfl_xor((int)sum, m);
		const u32 o = (u32)__shfl_xor((int)over, m);
		over = o > over ? o : over;
	}
	const unsigned long long worst = (unsigned long long)over * PAIR_SEGS;
	*P = over ? (worst > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (u32)worst) : sum;
	*G = *gcount;
	return *P <= cap && *G <= gbound;
}

// input of the two scans behind the cull pass (ugrt_scan.h): ITEMS = false the buckets' counts (n = the table's words),
// ITEMS = true the exact-pass items per beam as PairItemLoad forms them, from the counts of the beam's buckets
struct PairBucketLoad {
	const u32 *bkt, *segcnt;
	u32 segcap;
	const u32 *gcount;
	u32 cap, gbound, sbits;
	const GBox *boxes;
	unsigned long long *staged;
	u32 XSEG;
	u32 *pair_count; // the pass's pairs, for the waiting form's read-back
	PairCheck chk;   // asynchronous form (pg != nullptr): where the checked counts and the report go
	bool ITEMS;
	__device__ __forceinline__ void operator()(u32 base, u32 n, u32 (&v)[SC_ITEMS]) const
	{
		// (the counts are requested before the pass's totals are formed, for every bucket and beam the table has: what the
		// totals rule out is dropped afterwards -- one round trip instead of two in front of the look-back)
		u32 P, G;
		if (!ITEMS) {
			if (base + SC_ITEMS <= n) { // (the table is 16-byte aligned, base a multiple of 16)
#pragma unroll
				for (int q = 0; q < SC_ITEMS / 4; q++) {
					const uint4 x = reinterpret_cast<const uint4 *>(bkt + base)[q];
					v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
				}
			} else {
#pragma unroll
				for (int k = 0; k < SC_ITEMS; k++)
					v[k] = base + (u32)k < n ? bkt[base + k] : 0u;
			}
			const bool fits = d_pair_totals(segcnt, segcap, gcount, cap, gbound, &P, &G);
			if (blockIdx.x == 0 && threadIdx.x == 0) { // (what k_pair_compact's first workgroup did)
				pair_count[0] = P;
				if (chk.pg) {
					chk.report[0] = P;
					chk.report[1] = G;
					if (!fits)
						atomicOr(chk.status, UGRT_STATUS_PAIR_OVERFLOW);
					chk.pg[0] = fits ? P : 0u; // nothing is traced: the frame is reported as incomplete
					chk.pg[1] = G;
				}
			}
			const unsigned long long used = fits ? (unsigned long long)G << sbits : 0ull;
#pragma unroll
			for (int k = 0; k < SC_ITEMS; k++)
				v[k] = base + (u32)k < used ? v[k] : 0u; // (beyond the pass's beams the table is not cleared)
			return;
		}
		// a beam's candidates: the sum of its buckets.  The thread's 16 beams are loaded side by side, 16 bytes of each
		// per round (the sums of 16 beams x 16 classes one after the other were 256 dependent round trips: 56 us)
		u32 cands[SC_ITEMS], nsubs[SC_ITEMS];
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++)
			cands[k] = nsubs[k] = 0u;
		const u32 have = gbound < n ? gbound : n; // beams the table has
		if (base < have) {
#pragma unroll
			for (int k = 0; k < SC_ITEMS; k++)
				nsubs[k] = (boxes[base + (u32)k < have ? base + (u32)k : have - 1u].ray_count + 63u) / 64u;
			if (sbits >= 2u) {
				for (u32 q = 0; q < (1u << (sbits - 2u)); q++) {
#pragma unroll
					for (int k = 0; k < SC_ITEMS; k++) {
						const u32 g = base + (u32)k < have ? base + (u32)k : have - 1u; // (clamped: no branch around the loads)
						const uint4 x = reinterpret_cast<const uint4 *>(bkt + ((size_t)g << sbits))[q];
						cands[k] += x.x + x.y + x.z + x.w;
					}
				}
			} else {
				for (u32 c = 0; c < (1u << sbits); c++) {
#pragma unroll
					for (int k = 0; k < SC_ITEMS; k++) {
						const u32 g = base + (u32)k < have ? base + (u32)k : have - 1u;
						cands[k] += bkt[(g << sbits) + c];
					}
				}
			}
		}
		const bool fits = d_pair_totals(segcnt, segcap, gcount, cap, gbound, &P, &G);
		const u32 Gn = fits && P ? G : 0u; // (no pairs: no items)
		const u32 lim = Gn < n ? Gn : n;
		unsigned long long mine = 0;
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++) {
			const u32 g = base + (u32)k;
			u32 x = 0;
			if (g < lim) {
				const u32 cand = cands[k], nsub = nsubs[k];
				const u32 nseg = (cand + XSEG - 1) / XSEG;
				x = (nseg < XSEG_LAST + 1u ? nseg : XSEG_LAST + 1u) * nsub;
				mine += (unsigned long long)cand * nsub;
			}
			v[k] = x;
		}
		// candidates staged by the exact pass (work accounting): one atomic per wave
#pragma unroll
		for (int m = 32; m >= 1; m >>= 1)
			mine += __shfl_xor(mine, m);
		if ((threadIdx.x & 63) == 0 && mine)
			atomicAdd(staged, mine);
	}
};

// PLACE: the workgroups behind the first `nitemb` (a multiple of PAIR_SEGS of them) read the staging segments as the
// cull pass left them and write each pair's triangle id to bincl[key] - (what is left of the bucket's counter) + (rank
// among the wave's pairs of that key): the lanes of a wave are sorted into groups of equal keys first (scalar loop, no
// memory), then the groups' first lanes take their places with ONE returning atomic each, all in flight together.  The
// same workgroups write the beams' candidate runs for the exact pass.  The first `nitemb` workgroups list the exact
// pass's items (d_pair_items), which depend on the scan alone: chains of dependent loads, started first so that they
// run beside the placement, not behind it.
__global__ __launch_bounds__(WL_THREADS) void k_pair_place(const u32 *__restrict__ segcnt, u32 segcap,
							    const u32 *__restrict__ sbeam, const u32 *__restrict__ stri,
							    u32 *__restrict__ pair_tri, u32 out_cap, u32 *__restrict__ bkt,
							    const u32 *__restrict__ bincl, u32 bkt_words, u32 sbits,
							    const u32 *__restrict__ pg, const u32 *__restrict__ gcount,
							    u32 *__restrict__ pstart, u32 *__restrict__ pend, u32 nitemb,
							    const u32 *__restrict__ xincl, u32 Gcap, u32 xcap,
							    const GBox *__restrict__ boxes, u32 XSEG, u32 *__restrict__ item_seg,
							    u32 *__restrict__ item_sub, u32 *__restrict__ status, RsFirst hs)
{
	if (blockIdx.x < nitemb) {
		d_pair_items(blockIdx.x, nitemb, xincl, Gcap, xcap, nullptr, nullptr, bincl, sbits, boxes, XSEG, item_seg, item_sub, status, hs);
		return;
	}
	const u32 block = blockIdx.x - nitemb, nplace = gridDim.x - nitemb;
	if (pg && pg[0] == 0u) // asynchronous form: no pairs, or counts beyond what the pass was made for
		return;
	const u32 G = *gcount; // (<= the bound the table was made for: checked by the scan)
	for (u32 g = block * WL_THREADS + threadIdx.x; g < G && ((g + 1u) << sbits) <= bkt_words; g += nplace * WL_THREADS) {
		pstart[g] = g ? bincl[(g << sbits) - 1u] : 0u;
		pend[g] = bincl[((g + 1u) << sbits) - 1u];
	}
	const int lane = threadIdx.x & 63;
	const u32 seg = block % PAIR_SEGS, part = block / PAIR_SEGS, parts = nplace / PAIR_SEGS;
	const u32 c = segcnt[seg * PAIR_SEG_STRIDE], n = c < segcap ? c : segcap;
	const size_t src = (size_t)seg * segcap;
	// (a round is three dependent round trips -- pair, place, store -- so the next round's pair is requested first)
	u32 key_n = 0xFFFFFFFFu, tri_n = 0u;
	if (part * WL_THREADS + threadIdx.x < n) {
		key_n = sbeam[src + part * WL_THREADS + threadIdx.x];
		tri_n = stri[src + part * WL_THREADS + threadIdx.x];
	}
	for (u32 i0 = part * WL_THREADS; i0 < n; i0 += parts * WL_THREADS) {
		const u32 key = key_n, tri = tri_n, in = i0 + parts * WL_THREADS + threadIdx.x;
		key_n = 0xFFFFFFFFu;
		if (in < n) {
			key_n = sbeam[src + in];
			tri_n = stri[src + in];
		}
		const bool ok = key < bkt_words;
		const u32 end = bincl[ok ? key : 0u]; // (requested beside the place, not behind it)
		u32 leader = 0u, rank = 0u, cnt = 0u;
		unsigned long long left = __ballot(ok);
		while (left != 0ull) {
			const int l = (int)__builtin_ctzll(left);
			const u32 lk = (u32)__builtin_amdgcn_readlane((int)key, l);
			const unsigned long long same = __ballot(ok && key == lk);
			if (ok && key == lk) {
				leader = (u32)l;
				rank = d_rank_in_mask(same);
				cnt = (u32)__popcll(same);
			}
			left &= ~same;
		}
		u32 old = 0u;
		if (ok && (u32)lane == leader)
			old = atomicSub(&bkt[key], cnt);
		old = (u32)__shfl((int)old, (int)leader);
		if (ok) {
			const u32 pos = end - old + rank;
			if (pos < out_cap)
				pair_tri[pos] = tri;
		}
	}
}

// EXACT pass: item -> (beam, segment of its candidate list, 64-ray sub-group); lane = ray, the reference's test
#ifdef UGRT_SHADOW_TIMELINE
// Instrumented builds only (make EXTRA=-DUGRT_SHADOW_TIMELINE; tools/shadow_timeline.py): every wave of the exact pass
// leaves its start and end time (s_memrealtime, 100 MHz) and the number of items it worked on.
__device__ unsigned long long *g_shadow_tl;
#endif
template <bool REC>
__global__ __launch_bounds__(64) void k_trace_shadow(CamBlock cam, const u32 *__restrict__ xincl, u32 G,
						      const u32 *__restrict__ item_seg, const u32 *__restrict__ item_sub,
						      const GBox *__restrict__ boxes, const u32 *__restrict__ pstart,
						      const u32 *__restrict__ pend, const u32 *__restrict__ pair_tri,
						      const float *__restrict__ verts, const int *__restrict__ tris,
						      const float4 *__restrict__ rec, const float *__restrict__ t_value_list,
						      const float *__restrict__ ray_direction_list,
						      int *__restrict__ is_shadowed, const u32 *__restrict__ ray_pixels,
						      const float *__restrict__ cmPt, u32 XSEG, u32 *__restrict__ sub_done,
						      u32 nsubmax, const float4 *__restrict__ sray, u32 item_cap,
						      u32 *__restrict__ report, const u32 *__restrict__ status,
						      const unsigned long long *__restrict__ work, u32 SLICES, u32 W0, u32 SIEVE, u32 NSIEVE)
{
	__shared__ __attribute__((aligned(16))) float lds[64 * 16]; // per survivor: tvec, e1, e2, then the part all rays share: qvec, T
	const int lane = threadIdx.x;
#ifdef UGRT_SHADOW_TIMELINE
	const unsigned long long tl0 = __builtin_amdgcn_s_memrealtime();
	u32 tl_n = 0;
#endif
	// every kernel that raises a status bit or counts work has finished: complete the pass's report
	if (blockIdx.x == 0 && lane == 0) {
		report[2] = *status;
		reinterpret_cast<unsigned long long *>(report + 4)[0] = work[0];
		reinterpret_cast<unsigned long long *>(report + 4)[1] = work[1];
	}
	// (the list is written, and sorted, at its capacity: behind the last item come entries of segment XSEG_LAST + 1.  A
	// wave tells by its entry that there is nothing to do - not by the number of items, a load every one of the 400 k
	// single-item waves would have to wait for first.  Asynchronous form: a list cut at its estimated capacity is
	// flagged by k_pair_items.)
	const u32 total = item_cap;
	const float lx = cam.cc[0], ly = cam.cc[1], lz = cam.cc[2];
	// SLICES 1: persistent waves, a contiguous slice of the list per XCD; otherwise one wave per item, runs of
	// 2^((SLICES >> 1) - 1) items per XCD in turn (as the primary tracer)
	u32 first = blockIdx.x;
	if (SLICES == 1u) {
		first = d_xcd_block();
	} else if (SLICES > 1u) {
		const u32 rl = (SLICES >> 1) - 1u, j = blockIdx.x >> 3;
		first = ((((j >> rl) << 3) + (blockIdx.x & 7u)) << rl) + (j & ((1u << rl) - 1u));
	}
	// Which items a wave takes.  The list is sorted by segment, the first segments of all sub-groups come first and are
	// where the work is: of the 325 k items of the bench frame 42 k do anything, 33 k of them among the first 40 k; the
	// other 283 k find their sub-group flagged - 0.9 us each, but the chip starts fewer than four waves per ns, so they
	// were 77 of the pass's 178 us, and the long items behind them (up to 80 us: lit rays meet every candidate) started
	// late and were its tail (per-wave time stamps, profiles/r04_shadow_exact_timeline.txt).  So only the first W0 items
	// (>= the number of sub-groups: rays / 64 + beams) get a wave each; behind them a SIEVE wave looks at SIEVE items at
	// once, lane = item, and works off the few that have anything to do.  Its items lie NSIEVE apart: the working ones
	// cluster (neighbouring sub-groups of a beam with lit rays) and must not meet in one wave.
	// (persistent form: every wave takes single items, in a stride)
	const bool persistent = SLICES == 1u;
	for (u32 base = first; base < (persistent ? total : W0 + NSIEVE); base += gridDim.x) {
		const bool sieve = !persistent && base >= W0; // (base = W0 + v: the sieve wave's first item)
		const u32 n_v = sieve ? SIEVE : 1u, stride_v = sieve ? NSIEVE : 0u;
		u32 sgm_v = XSEG_LAST + 1u, gs_v = 0u;
		const u32 my_it = base + (u32)lane * stride_v;
		if ((u32)lane < n_v && my_it < total) {
			sgm_v = item_seg[my_it];
			gs_v = item_sub[my_it];
		}
		// Three quarters of the items find every ray of their sub-group flagged by an earlier segment (the
		// point of the segment-major order).  The sub-group says so in one word, and the flags are looked
		// at before the rays are rebuilt.  (a padding entry reads beam 0's word)
		const u32 flagged_v = __hip_atomic_load(sub_done + (size_t)(gs_v >> 7) * nsubmax + (gs_v & 127u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		unsigned long long todo = __ballot(sgm_v <= XSEG_LAST && flagged_v == 0u);
	while (todo != 0ull) {
#ifdef UGRT_SHADOW_TIMELINE
		tl_n++;
#endif
		const int tl = (int)__builtin_ctzll(todo);
		todo &= todo - 1ull;
		// The head of an item is a chain of loads that depend on each other, and the pass is as long as its
		// chains: what does not depend on a load is requested with it.  {entry} -> {the sub-group's "all flagged"
		// word} -> {beam, candidate run} -> {pixel, rebuilt ray, ids of the first candidates} -> {flag of the pixel, the
		// candidates' records}: five round trips where the straightforward order made ten.  Indices are clamped, not
		// masked: loads under a divergent branch are waited for at the join.
		const u32 sgm = (u32)__builtin_amdgcn_readlane((int)sgm_v, tl), gs = (u32)__builtin_amdgcn_readlane((int)gs_v, tl);
		const u32 g = gs >> 7, sub = gs & 127u; // the sub-groups of a beam share its candidate list (a padding entry reads beam 0's word)
		u32 *my_done = sub_done + (size_t)g * nsubmax + sub;
		const GBox bx = boxes[g];
		const u32 ps = pstart[g], pe = pend[g];
		const u32 p0 = ps + sgm * XSEG;
		const u32 p1 = (sgm != XSEG_LAST && (p0 + XSEG) < pe) ? (p0 + XSEG) : pe;
		const u32 rl0 = 64u * sub + (u32)lane;
		const bool have_ray = rl0 < bx.ray_count;
		const u32 ri = bx.ray_start + (have_ray ? rl0 : bx.ray_count - 1u); // (a listed sub-group has a ray)
		const int pixel = (int)ray_pixels[ri];
		const float4 q = sray[ri]; // = d_shadow_ray(pixel), stored by k_shadow_boxes
		const u32 id_first = pair_tri[min(p0 + (u32)lane, p1 - 1u)]; // (a listed segment has a candidate)
		u32 id_next = pair_tri[min(p0 + 64u + (u32)lane, p1 - 1u)];   // (beyond the run: its last candidate again)
		// a ray already flagged by another segment of its beam needs no more tests
		float qx = q.x, qy = q.y, qz = q.z, qw = q.w;
		// (all four requests go out together; the compiler would move the ones the early exit below does not need behind it)
		asm volatile("" : "+v"(id_next), "+v"(qx), "+v"(qy), "+v"(qz), "+v"(qw));
		const int flag = is_shadowed[pixel];
		float t9n[9];
		d_load_triangle<REC>(rec, verts, tris, id_first, lx, ly, lz, t9n);
		// (the records are requested beside the flag, not behind the test of it)
		asm volatile("" : "+v"(t9n[0]), "+v"(t9n[3]), "+v"(t9n[4]), "+v"(t9n[8]));
		bool done = !have_ray | (flag == 1); // rayDoneMap == 2
		if (__ballot(!done) == 0ull) {
			if (lane == 0)
				__hip_atomic_store(my_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			continue;
		}
		ShadowRay r;
		r.rd[0] = qx;
		r.rd[1] = qy;
		r.rd[2] = qz;
		r.distance_b = qw;
		r.pixel = pixel;
		// the candidates were found for the whole beam; this wave's 64 (still undecided) rays are a
		// narrower packet, so each staged candidate is culled once more against their own box
		DirBox box = d_dir_box(r.rd, !done);
		unsigned long long boxed = __ballot(!done); // the rays the box was formed for
		bool hit = false;
		for (u32 b = p0; b < p1; b += 64) {
			const u32 ncand = (p1 - b) < 64u ? (p1 - b) : 64u;
			// rays flagged by the batches before need no more tests: once an eighth of the box's rays are gone the box is
			// formed again for the rest (six wave reductions against ~35 instructions for every candidate it then culls)
			{
				const unsigned long long open = __ballot(!done);
				if (8u * (u32)__popcll(open) <= 7u * (u32)__popcll(boxed)) {
					box = d_dir_box(r.rd, !done);
					boxed = open;
				}
			}
			// (this batch's records were requested a batch ago, the ids of the next one with them: now that batch's records
			// are requested, and the ids of the one after)
			float t9[9];
#pragma unroll
			for (int k = 0; k < 9; k++)
				t9[k] = t9n[k];
			d_load_triangle<REC>(rec, verts, tris, id_next, lx, ly, lz, t9n);
			id_next = pair_tri[min(b + 128u + (u32)lane, p1 - 1u)];
			const bool keep = (u32)lane < ncand && !d_cull(&t9[0], &t9[3], &t9[6], box);
			const unsigned long long mask = __ballot(keep);
			const u32 cnt = (u32)__popcll(mask);
			__syncthreads();
			if (keep) {
				// (all rays start at the light: tvec x e1 and e2 . (tvec x e1) are the triangle's, formed here once)
				float qv[3], T;
				d_mt_shared(&t9[0], &t9[3], &t9[6], qv, &T);
				float4 *dst = reinterpret_cast<float4 *>(&lds[d_rank_in_mask(mask) * 16u]);
				dst[0] = make_float4(t9[0], t9[1], t9[2], t9[3]);
				dst[1] = make_float4(t9[4], t9[5], t9[6], t9[7]);
				dst[2] = make_float4(t9[8], qv[0], qv[1], qv[2]);
				dst[3] = make_float4(T, 0.0f, 0.0f, 0.0f);
			}
			__syncthreads();
			if (!done) {
				for (u32 k = 0; k < cnt; k++) {
					const float4 *src = reinterpret_cast<const float4 *>(&lds[k * 16u]);
					const float4 a = src[0], c = src[1], e = src[2];
					const float T = lds[k * 16u + 12u];
					const float tv[3] = { a.x, a.y, a.z }, e1[3] = { a.w, c.x, c.y }, e2[3] = { c.z, c.w, e.x }, qv[3] = { e.y, e.z, e.w };
					const float value = d_intersect_tri_shared(tv, e1, e2, qv, T, r.rd, 999999.9f);
					if (value != 0.0f) {
						// light_kernel.cu:193-202 with isSmaller (:1-11)
						float pt[3];
						pt[0] = lx + value * r.rd[0];
						pt[1] = ly + value * r.rd[1];
						pt[2] = lz + value * r.rd[2];
						float distance_a = __builtin_sqrtf((pt[0] - lx) * (pt[0] - lx) + (pt[1] - ly) * (pt[1] - ly) +
										   (pt[2] - lz) * (pt[2] - lz));
						if (distance_a + 1e-03f < r.distance_b) {
							hit = true;
							done = true;
							break;
						}
					}
				}
			}
			// the whole beam is decided: skip the remaining candidates
			if (__ballot(!done) == 0ull)
				break;
		}
		if (hit)
			is_shadowed[r.pixel] = 1;
		if (__ballot(!done) == 0ull && lane == 0)
			__hip_atomic_store(my_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
		if (!persistent)
			break;
	}
#ifdef UGRT_SHADOW_TIMELINE
	if (g_shadow_tl && lane == 0) {
		g_shadow_tl[2 * (size_t)blockIdx.x] = tl0;
		g_shadow_tl[2 * (size_t)blockIdx.x + 1] = (__builtin_amdgcn_s_memrealtime() << 8) | (tl_n & 255u);
	}
#endif
}

static int bits_of(u32 v)
{
	int b = 1;
	while (b < 32 && (1ull << b) < (unsigned long long)v)
		b++;
	return b;
}

// One ugrt_trace_shadow: what its stages share, and the stages in the order they run
struct ShadowPass {
	ugrt_ctx *ctx;
	hipStream_t st;
	u32 C, n; // light cells, rays
	// the caller's arrays (d_span / d_offset: over the union of a cell's slabs where NUM_SLABS > 1)
	const unsigned *d_value_list, *d_span, *d_offset, *d_map, *d_prefix_map;
	const float *d_vertlist, *d_t_value, *d_ray_dir, *d_cam_position;
	const int *d_trilist;
	int *d_is_shadowed;
	u32 ncellk;  // C + sentinel + "not traced"
	size_t maxg; // beams
	u32 traced, launch_cap, nchunks_arg; // which chunks get traced
	const u32 *nchunks_dev; // (stays null unless the chunk count lives on the device)
	bool use_rec;
	const float4 *rec;
	void *k0, *k1; // the carved-up buffers
	u32 *v0, *v1, *rstart, *rend, *gincl, *iincl, *pstart, *pend;
	GBox *boxes;
	unsigned long long *wcnt; // [0] cull tests, [1] staged candidates
	bool own_sort, async;
	u32 beam, XSEG, sbits; // launch shape
	u32 P, G, Gcap, xcap;  // candidate pairs and beams, as read back or (asynchronous form) as estimated; exact-pass items
	const u32 *pgp;        // device counts (asynchronous form; null otherwise)
	u32 *status, *report;  // the status word on the device; the pinned host words of the pass's report
	u32 *xincl, *iseg1, *isub1; // the exact pass's item list
	// candidate pairs bucketed by counting (option "shadow_pairs") instead of sorted: the beam bound the bucket table is
	// made for, its words, the counts and their inclusive sums; the cursors of the staging segments and a segment's room
	bool deferred; // the ray sort was put off: d_map is the map as ugrt_map_rays_to_light left it and every ray is traced
	bool counted;
	u32 gbound, bkt_words, *bkt, *bincl, *segcnt, segcap;
	const u32 *pair_tri; // the candidates' triangle ids in beam order, as the exact pass reads them
	int traced_chunks(unsigned num_chunks);
	int reserve();
	int plan();       // 0. waiting or asynchronous, candidate pairs sorted or counted
	int beams();      // 1. rays in (cell, direction code) order, runs per cell, beams and their boxes
	int cull();       // 2. cull pass -> (beam, triangle) candidate pairs
	int candidates(); // 3. candidates by beam, cut into the exact pass's items
	int exact();      // 4. exact pass
};

// which chunks get traced: the reference launches nbx*nby blocks, block b
// takes chunk b-1 and only blocks b < num_chunks work (light_kernel.cu:76-85)
int ShadowPass::traced_chunks(unsigned num_chunks)
{
	const bool on_device = num_chunks == UGRT_CHUNKS_ON_DEVICE; // ugrt_sort_rays(..., NULL) left the count there
	launch_cap = (ctx->cfg.flags & UGRT_FLAG_SHADOW_ALL_CHUNKS) ? 0xFFFFFFFFu : (u32)ctx->nbx * (u32)ctx->nby;
	nchunks_arg = num_chunks;
	if (on_device) {
		if (!ctx->ray_sort_pending && !ctx->cbase.p)
			return ugrt_fail(UGRT_EINVAL, "trace_shadow: UGRT_CHUNKS_ON_DEVICE without a ugrt_sort_rays before");
		if (ctx->chunk_prefix != d_prefix_map || ctx->chunk_map != d_map)
			return ugrt_fail(UGRT_EINVAL, "trace_shadow: UGRT_CHUNKS_ON_DEVICE refers to the last ugrt_sort_rays, which "
						      "sorted other arrays");
		traced = num_chunks; // the keys kernel applies the launch rule itself
		deferred = ctx->ray_sort_pending;
		if (ctx->ray_sort_pending)
			nchunks_arg = 0u; // every chunk is traced and none was formed: d_map is the unsorted map, all n rays count
		else
			nchunks_dev = (const u32 *)ctx->cbase.p + C; // inclusive scan of the chunks per light cell, last entry
	} else if (launch_cap == 0xFFFFFFFFu) {
		traced = num_chunks;
	} else {
		u32 lim = num_chunks < launch_cap ? num_chunks : launch_cap;
		traced = lim ? lim - 1 : 0;
	}
	ctx->stats[2] = traced;
	ctx->stats[1] = ctx->stats[6] = ctx->stats[7] = 0;
	return UGRT_OK;
}

// the pass's buffers, all but the candidate pairs' (cull) and the two that later stages size
int ShadowPass::reserve()
{
	int rc;
	// NUM_SLABS > 1: span/offset hold C * slabs entries; the block of a chunk walks all slabs of its cell
	// (light_kernel.cu:105-113) and a ray is shadowed by an occluder in any of them: the cell's list is the
	// union of its slabs' runs, which lie next to each other
	if (ctx->cfg.slabs > 1 && (rc = ugrt_slab_union(ctx, d_span, d_offset, C, (u32)ctx->cfg.slabs, &d_span, &d_offset)))
		return rc;
	ncellk = C + 2; // + sentinel + "not traced"
	maxg = (size_t)n / 64 + C + 1; // beams
	const struct { DevBuf &b; size_t bytes; } need[] = {
		{ ctx->skey[0], (size_t)n * 8 }, { ctx->sval[0], (size_t)n * 4 }, { ctx->skey[1], (size_t)n * 8 }, { ctx->sval[1], (size_t)n * 4 },
		{ ctx->sstart, (size_t)ncellk * 8 }, // run starts, then run ends
		{ ctx->sbase, (size_t)C * 8 },
		{ ctx->sdesc, maxg * sizeof(GBox) },
		// candidate run starts, then ends, per beam; then one "all rays flagged" word per 64-ray sub-group
		{ ctx->tbcnt, maxg * 8 + maxg * 128 * 4 },
		{ ctx->witems, maxg * 8 },
		{ ctx->sray, (size_t)n * 16 }, // rebuilt shadow rays in beam order
		{ ctx->pseg, (size_t)PAIR_SEGS * PAIR_SEG_STRIDE * 4 },
	};
	for (const auto &r : need)
		if ((rc = ugrt_buf_reserve(ctx, r.b, r.bytes)))
			return rc;
	k0 = ctx->skey[0].p, k1 = ctx->skey[1].p;
	v0 = (u32 *)ctx->sval[0].p, v1 = (u32 *)ctx->sval[1].p;
	rstart = (u32 *)ctx->sstart.p, rend = rstart + ncellk;
	gincl = (u32 *)ctx->sbase.p, iincl = gincl + C;
	pstart = (u32 *)ctx->tbcnt.p, pend = pstart + maxg;
	boxes = (GBox *)ctx->sdesc.p;
	wcnt = (unsigned long long *)(ctx->d_small + UGRT_DSMALL_SHADOW_WORK); // [0] cull tests, [1] staged candidates
	// (the two work counters + the candidate-pair cursor behind them, and the cull pass's output cursors, are cleared by
	// the keys kernel: two fills less per pass)
	return UGRT_OK;
}

// 0. The form of the pass.  Synchronous form: the pair count is read back behind the cull pass (it sizes the
// launches that follow), and the pass is repeated with a larger buffer if it was too small.  Asynchronous form
// (option "async_build", once a synchronous pass has left estimates): no read-back; the launches are sized by
// the previous pass's counts plus a quarter, the kernels take the real counts from the device, and counts
// beyond the capacities raise a status bit instead (UGRT_EOVERFLOW at the next synchronisation).
// The candidate pairs are counted into their (beam, size class) buckets unless "shadow_pairs" is 0, the library sorts,
// or the table -- beam bound << size bits words, where the bound is every beam the rays could form in the waiting form
// (the cull pass runs before the count is read back) and the power of two above the estimate in the asynchronous one --
// would exceed SHADOW_BUCKET_WORDS: "shadow_sizebits" 8 on a huge light grid cannot ask for an unbounded table.
int ShadowPass::plan()
{
	int rc;
	own_sort = ctx->opt[UGRT_OPT_SORT_LIBRARY] != 1;
	sbits = ctx->opt[UGRT_OPT_SHADOW_SIZEBITS] >= 0 ? (u32)ctx->opt[UGRT_OPT_SHADOW_SIZEBITS] : 4u;
	sbits = sbits > 8u ? 8u : sbits;
	if (ctx->shadow_async_pending) { // what the last asynchronous pass needed (possibly a frame old)
		ctx->est_pairs = ctx->h_pinned[UGRT_PIN_SHADOW];
		ctx->est_beams = ctx->h_pinned[UGRT_PIN_SHADOW + 1];
	}
	async = ctx->opt[UGRT_OPT_ASYNC_BUILD] == 1 && ctx->have_shadow_est && ugrt_reported_status(ctx) == 0u && !ctx->overflow_seen &&
		!ctx->overflow_repair;
	if (!async && ugrt_reported_status(ctx) != 0u)
		ctx->overflow_seen = true;
	gbound = (u32)maxg;
	if (async) {
		// beams: a power of two above the estimate keeps the sort at the key width the real count needs
		u32 gb = 1;
		while (gb < ctx->est_beams + ctx->est_beams / 4u + 1u)
			gb <<= 1;
		gbound = gb < gbound ? gb : gbound;
	}
	counted = ctx->opt[UGRT_OPT_SHADOW_PAIRS] != 0 && own_sort && ((unsigned long long)gbound << sbits) <= SHADOW_BUCKET_WORDS;
	ctx->shadow_pairs_counted = counted;
	if (counted) {
		bkt_words = gbound << sbits;
		const size_t half = ((size_t)bkt_words + 3u) / 4u * 4u; // (both halves 16-byte aligned)
		if ((rc = ugrt_buf_reserve(ctx, ctx->pbkt, 2 * half * 4)))
			return rc;
		bkt = (u32 *)ctx->pbkt.p, bincl = bkt + half;
	}
	return UGRT_OK;
}

// 1. rays: (cell, direction code) order, runs per cell, beams
int ShadowPass::beams()
{
	int rc;
	ugrt_prof_begin(ctx, UGRT_ST_SHADOW_PREP);
	// key = (light cell, direction code).  The cell field also holds the two values behind the last cell (C = nothing can
	// shadow the ray, C + 1 = not traced), so it is as wide as C + 1 needs: 32-bit keys while that leaves >= 12 bits for
	// the code (C + 2 <= 2^20: a 1024 x 512 light grid still, 1024 x 1024 no longer), 64-bit keys above
	const u32 cellbits = (u32)bits_of(ncellk);
	const bool key64 = cellbits > 20u || ctx->opt[UGRT_OPT_SHADOW_KEY64] == 1;
	u32 mbits = 32u - cellbits;
	if (ctx->opt[UGRT_OPT_SHADOW_MBITS] > 0 && (u32)ctx->opt[UGRT_OPT_SHADOW_MBITS] < mbits)
		mbits = (u32)ctx->opt[UGRT_OPT_SHADOW_MBITS];
	mbits = mbits > 24u ? 24u : mbits;
	ctx->shadow_key_bits = (key64 ? 30u : mbits) + cellbits;
	const u32 kblocks = (u32)((n + WL_THREADS - 1) / WL_THREADS) < 768u ? (u32)((n + WL_THREADS - 1) / WL_THREADS) : 768u;
	// (the kernels that write this pass's sort keys count their first digit: no histogram kernel before the sorts;
	// 64-bit keys go to the library's sort and are not counted)
	RsFirst hs = { nullptr };
	if (!key64 && own_sort && (rc = ugrt_sort_first_digit(ctx, &hs)))
		return rc;
	// by fragments (FRAGMENTS above) where the map is the unsorted one of whole 8x8 tiles and every ray is traced
	const u32 W = (u32)ctx->cam.W;
	const bool frags = deferred && !key64 && own_sort && ctx->opt[UGRT_OPT_SHADOW_FRAGS] != 0 && W != 0u && W % 8u == 0u &&
			   n % (8u * W) == 0u;
	ctx->shadow_frag_ran = frags;
	if (frags) {
		// the launches behind the fragment kernel are made for `fcap` fragments: all there can be (a fragment holds a ray),
		// or, asynchronous form, the last fragment pass's count plus a quarter, against which the count is checked on the
		// device by the fragment kernel.  The count travels in the pass's report (word 3 of the pinned words).
		u32 *fw = ctx->d_small + UGRT_DSMALL_FRAGS; // {cursor, finished workgroups, checked count}
		u32 fcap = n;
		if (async) {
			if (ctx->have_frag_est) {
				ctx->est_frags = ctx->h_pinned[UGRT_PIN_SHADOW + 3];
				const unsigned long long want = (unsigned long long)ctx->est_frags + ctx->est_frags / 4u + 1024u;
				fcap = want < n ? (u32)want : n;
			} else {
				// (no fragment pass has reported yet and none is under way: until this one has, the estimate is all there can be)
				ctx->h_pinned[UGRT_PIN_SHADOW + 3] = n;
				ctx->have_frag_est = true;
			}
		}
		u32 *fkeys = (u32 *)k0, *fincl = fkeys + n, *skeys = (u32 *)k1, *sslots = skeys + n;
		FragRec *recs = (FragRec *)ctx->sray.p; // (the rebuilt rays are written behind the expansion, by k_shadow_boxes)
		const u32 fb = (n / 64u + FRAG_ROUND - 1u) / FRAG_ROUND, fblocks = fb < 768u ? (fb ? fb : 1u) : 768u;
		hipLaunchKernelGGL(k_shadow_frags, dim3(fblocks), dim3(WL_THREADS), 0, st, ctx->cam, d_t_value, d_ray_dir, d_map, n, W, C, d_span,
				   d_cam_position, mbits, fkeys, v0, recs, fw, fcap, ctx->d_small + UGRT_DSMALL_STATUS,
				   ctx->h_pinned + UGRT_PIN_SHADOW, rstart, 2u * ncellk, (u32 *)wcnt, 5u, (u32 *)ctx->pseg.p,
				   PAIR_SEGS * PAIR_SEG_STRIDE, hs);
		UGRT_HIP(hipGetLastError());
		if ((rc = ugrt_sort_pairs_u32(ctx, fkeys, skeys, v0, sslots, fcap, (int)(mbits + cellbits), fw + 2, true)))
			return rc;
		const FragCountLoad nrays = { sslots, recs, fw + 2 };
		if ((rc = ugrt_scan_launch<true>(ctx, nrays, fincl, fcap, ScanTailNone())))
			return rc;
		const u32 eb = (fcap + FRAG_PER_WAVE * (WL_THREADS / 64u) - 1u) / (FRAG_PER_WAVE * (WL_THREADS / 64u));
		hipLaunchKernelGGL(k_shadow_expand, dim3(eb < 8192u ? (eb ? eb : 1u) : 8192u), dim3(WL_THREADS), 0, st, (const u32 *)skeys,
				   (const u32 *)sslots, (const FragRec *)recs, (const u32 *)fincl, (const u32 *)(fw + 2), mbits, d_map, n, W, v1, rstart, rend);
		UGRT_HIP(hipGetLastError());
	} else {
	hipLaunchKernelGGL(key64 ? k_shadow_keys<true> : k_shadow_keys<false>, dim3(kblocks), dim3(WL_THREADS), 0, st,
			   ctx->cam, d_t_value, d_ray_dir, d_map, d_prefix_map, nchunks_arg, nchunks_arg ? traced : 0u, n, C, d_span,
			   d_cam_position, key64 ? 30u : mbits, k0, v0, rstart, 2u * ncellk, nchunks_dev, launch_cap, ctx->chunk_capacity,
			   (u32 *)wcnt, 5u, (u32 *)ctx->pseg.p, PAIR_SEGS * PAIR_SEG_STRIDE, hs);
	UGRT_HIP(hipGetLastError());
	if (key64)
		rc = ugrt_prim_sort_pairs64(ctx, (const u64 *)k0, (u64 *)k1, v0, v1, n, 30 + (int)cellbits);
	else
		rc = own_sort ? ugrt_sort_pairs_u32(ctx, (const u32 *)k0, (u32 *)k1, v0, v1, n, (int)(mbits + cellbits), nullptr, true)
			      : ugrt_prim_sort_pairs(ctx, (const u32 *)k0, (u32 *)k1, v0, v1, n, (int)(mbits + cellbits));
	if (rc)
		return rc;
	if (key64)
		hipLaunchKernelGGL(k_shadow_runs<u64>, dim3((n + WL_THREADS - 1) / WL_THREADS), dim3(WL_THREADS), 0, st,
				   (const u64 *)k1, n, 30u, rstart, rend);
	else
		hipLaunchKernelGGL(k_shadow_runs<u32>, dim3((n + WL_THREADS - 1) / WL_THREADS), dim3(WL_THREADS), 0, st,
				   (const u32 *)k1, n, mbits, rstart, rend);
	UGRT_HIP(hipGetLastError());
	} // every ray
	// rays per beam: the cull pass costs (triangles of the cell) x (beams of the cell); the exact pass
	// re-culls the beam's candidates against each 64-ray sub-group, so its cost barely depends on the
	// beam size.  ~1000 rays per beam is the measured optimum on the 1 M-triangle scene (tools/beam_sweep.py)
	beam = ctx->opt[UGRT_OPT_SHADOW_BEAM] > 0 ? (u32)ctx->opt[UGRT_OPT_SHADOW_BEAM] : 2048u;
	beam = beam < 64u ? 64u : (beam > 8192u ? 8192u : (beam + 63u) / 64u * 64u);
	// candidates per exact-pass work item: a 64-ray sub-group stops at the first batch after which all its
	// rays are flagged, so long items cost little where everything is in shadow; short items bound the
	// work of a sub-group that stays lit (128 since the later segments' items go through sieve waves: twice the items
	// were twice the waves to start before - 256 then; profiles/r04_shadow_sieve_sweep.txt)
	XSEG = ctx->opt[UGRT_OPT_SHADOW_XSEG] > 0 ? (u32)ctx->opt[UGRT_OPT_SHADOW_XSEG] : 128u;
	XSEG = XSEG < 64u ? 64u : (XSEG + 63u) / 64u * 64u;
	// (the beams and the cull items per cell: two scans over the light cells in one launch)
	const ShadowCountLoad nbeams = { d_span, rstart, rend, beam, wcnt, false }, nitems = { d_span, rstart, rend, beam, wcnt, true };
	if ((rc = ugrt_scan_launch_pair<true>(ctx, nbeams, gincl, nitems, iincl, C)))
		return rc;
	if ((rc = ugrt_buf_reserve(ctx, ctx->citem, (size_t)CULL_TABLE * sizeof(CullItem))))
		return rc;
	hipLaunchKernelGGL(k_shadow_boxes, dim3(launch_blocks_for((u32)maxg)), dim3(64 * BOX_WAVES), 0, st, ctx->cam,
			   (const u32 *)gincl, C, (const u32 *)rstart, (const u32 *)rend, (const u32 *)v1, d_t_value,
			   d_ray_dir, d_cam_position, boxes, beam, pstart, (u32)(2 * maxg + maxg * (beam / 64u)),
			   (float4 *)ctx->sray.p, (const u32 *)iincl, d_span, d_offset, (CullItem *)ctx->citem.p,
			   counted ? bkt : (u32 *)nullptr, bkt_words, sbits);
	UGRT_HIP(hipGetLastError());
	ugrt_prof_end(ctx, UGRT_ST_SHADOW_PREP);
	return UGRT_OK;
}

// 2. cull pass -> (beam, triangle) candidate pairs in the staging segments, and either their compaction (with the first
// digit of the pair sort counted) or, counted buckets, the scan of the buckets' counts and of the exact pass's items per
// beam.  The launch behind the cull pass makes the pass's checks and leaves the pair count for the waiting form.
int ShadowPass::cull()
{
	int rc;
	u32 *pcount = ctx->d_small + UGRT_DSMALL_PAIRS; // right behind the work counters: cleared with them
	// (the report is written by the kernels straight into the pinned host words: no copy behind the pass)
	u32 *pg = ctx->d_small + UGRT_DSMALL_SHADOW;
	status = ctx->d_small + UGRT_DSMALL_STATUS, report = ctx->h_pinned + UGRT_PIN_SHADOW;
	xincl = (u32 *)ctx->witems.p;
	size_t cap, want = (size_t)4 << 22; // bytes per candidate buffer
	if (async && ((size_t)ctx->est_pairs + ctx->est_pairs / 2 + 65536) * 4 > want)
		want = ((size_t)ctx->est_pairs + ctx->est_pairs / 2 + 65536) * 4;
	for (int attempt = 0; attempt < 3; attempt++) {
		if (ctx->tkey[0].cap / 4 * 4 < want &&
		    ((rc = ugrt_buf_reserve(ctx, ctx->tkey[0], want)) || (rc = ugrt_buf_reserve(ctx, ctx->tkey[1], want)) ||
		     (rc = ugrt_buf_reserve(ctx, ctx->tval[0], want)) || (rc = ugrt_buf_reserve(ctx, ctx->tval[1], want))))
			return rc;
		cap = std::min(std::min(ctx->tkey[0].cap, ctx->tkey[1].cap), std::min(ctx->tval[0].cap, ctx->tval[1].cap)) / 4;
		cap = cap > 0xFFFFFFF0u ? 0xFFFFFFF0u : cap; // pairs that fit each of the four buffers
		segcnt = (u32 *)ctx->pseg.p;
		segcap = (u32)(cap / PAIR_SEGS);
		if (attempt > 0) { // (the first attempt's cursors were cleared by the keys kernel, its buckets by the box kernel)
			UGRT_HIP(hipMemsetAsync(segcnt, 0, (size_t)PAIR_SEGS * PAIR_SEG_STRIDE * 4, st));
			if (counted)
				UGRT_HIP(hipMemsetAsync(bkt, 0, (size_t)bkt_words * 4, st));
		}
		PairCheck chk = { nullptr, 0u, 0u, nullptr, nullptr, nullptr };
		if (async) {
			// (counted buckets: no beam beyond the bound has items, the items' scan and the searches in it end there)
			Gcap = counted ? gbound : (u32)maxg;
			G = gbound; // only its bit width is used below
			// launch size of the per-pair kernels; the check is made against it, not against the (larger) buffers:
			// the sort and the run kernel work on P pairs, so a count between the two would lose candidates
			const size_t lp = (size_t)ctx->est_pairs + ctx->est_pairs / 4 + 65536;
			P = (u32)(lp < cap ? lp : cap);
			chk = PairCheck{ (const u32 *)(gincl + (C - 1)), P, G, pg, status, report }; // (made by the first workgroup behind the cull pass)
		}
		RsFirst hsp = { nullptr };
		if (!counted && own_sort && (rc = ugrt_sort_first_digit(ctx, &hsp)))
			return rc;
		ugrt_prof_begin(ctx, UGRT_ST_SHADOW_CULL);
		hipLaunchKernelGGL(use_rec ? k_shadow_cull<true> : k_shadow_cull<false>,
				   dim3(launch_blocks_for(0xFFFFFFFFu, ctx->opt[UGRT_OPT_SHADOW_WAVES])), dim3(64), 0, st, ctx->cam, (const u32 *)iincl,
				   (const u32 *)gincl, C, d_span, d_offset, d_value_list, rec, d_vertlist, d_trilist,
				   (const GBox *)boxes, segcnt, segcap, (u32 *)ctx->tkey[1].p, (u32 *)ctx->tval[1].p, sbits,
				   (const CullItem *)ctx->citem.p, counted ? bkt : (u32 *)nullptr, gbound);
		if (!counted)
			hipLaunchKernelGGL(k_pair_compact, dim3(PAIR_SEGS * 16u), dim3(256), 0, st, (const u32 *)segcnt, segcap,
					   (const u32 *)ctx->tkey[1].p, (const u32 *)ctx->tval[1].p, (u32 *)ctx->tkey[0].p,
					   (u32 *)ctx->tval[0].p, pcount, chk, hsp);
		ugrt_prof_end(ctx, UGRT_ST_SHADOW_CULL);
		UGRT_HIP(hipGetLastError());
		if (counted) {
			// (the pairs a segment holds, the beams the table was made for: what the waiting form's launches can take)
			PairBucketLoad la = { bkt, segcnt, segcap, (const u32 *)(gincl + (C - 1)), async ? P : segcap * PAIR_SEGS, gbound, sbits, boxes,
					      wcnt + 1, XSEG, pcount, chk, false };
			PairBucketLoad lb = la;
			lb.ITEMS = true;
			ugrt_prof_begin(ctx, UGRT_ST_SHADOW_PREP);
			rc = ugrt_scan_launch_pair<true>(ctx, la, bincl, lb, xincl, bkt_words, async ? (size_t)gbound : maxg);
			ugrt_prof_end(ctx, UGRT_ST_SHADOW_PREP);
			if (rc)
				return rc;
		}
		if (async) {
			pgp = pg; // (the report travels to the host with the copy behind the exact pass)
			xcap = (ctx->est_beams + ctx->est_beams / 4u + 64u + P / XSEG) * (beam / 64u);
			ctx->shadow_async_pending = true;
			break;
		}
		UGRT_HIP(hipMemcpyAsync(ctx->h_pinned + UGRT_PIN_PAIRS, pcount, 4, hipMemcpyDeviceToHost, st));
		UGRT_HIP(hipMemcpyAsync(ctx->h_pinned + UGRT_PIN_BEAMS, gincl + (C - 1), 4, hipMemcpyDeviceToHost, st));
		UGRT_HIP(hipStreamSynchronize(st));
		P = ctx->h_pinned[UGRT_PIN_PAIRS];
		if ((size_t)P <= cap)
			break;
		if (attempt == 2)
			return ugrt_fail(UGRT_ENOMEM, "trace_shadow: %u candidate pairs do not fit", P);
		want = (size_t)P * 4 + ((size_t)P * 4) / 4; // (P > cap: the next attempt's buffers grow to this)
	}
	if (!async) {
		G = Gcap = ctx->h_pinned[UGRT_PIN_BEAMS];
		ctx->stats[1] = G;
		ctx->est_pairs = P;
		ctx->est_beams = G;
		ctx->have_shadow_est = true;
		if (ctx->shadow_frag_ran) // (the fragment kernel's report is in its pinned word)
			ctx->have_frag_est = true;
		// (the slots the asynchronous form reports into: never older than this pass)
		ctx->h_pinned[UGRT_PIN_SHADOW] = P;
		ctx->h_pinned[UGRT_PIN_SHADOW + 1] = G;
		ctx->shadow_async_pending = false;
		xcap = (G + P / XSEG) * (beam / 64u); // >= number of exact-pass items
	}
	return UGRT_OK;
}

// 3. candidates by beam, cut into the exact pass's items
int ShadowPass::candidates()
{
	int rc;
	ugrt_prof_begin(ctx, UGRT_ST_SHADOW_PREP);
	if (!counted) {
		if ((rc = own_sort ? ugrt_sort_pairs_u32(ctx, (const u32 *)ctx->tkey[0].p, (u32 *)ctx->tkey[1].p, (const u32 *)ctx->tval[0].p,
							 (u32 *)ctx->tval[1].p, P, bits_of(G) + (int)sbits, pgp, true)
				   : ugrt_prim_sort_pairs(ctx, (const u32 *)ctx->tkey[0].p, (u32 *)ctx->tkey[1].p, (const u32 *)ctx->tval[0].p,
							  (u32 *)ctx->tval[1].p, P, bits_of(G) + (int)sbits, pgp)))
			return rc;
		pair_tri = (const u32 *)ctx->tval[1].p;
		{
			u32 pb = (P + WL_THREADS - 1) / WL_THREADS;
			hipLaunchKernelGGL(k_pair_runs, dim3(pb ? pb : 1u), dim3(WL_THREADS), 0, st, (const u32 *)ctx->tkey[1].p, P, sbits,
					   pstart, pend, pgp);
		}
		UGRT_HIP(hipGetLastError());
		const PairItemLoad load = { pstart, pend, boxes, G, wcnt + 1, XSEG, pgp };
		if ((rc = ugrt_scan_launch<true>(ctx, load, xincl, Gcap, ScanTailNone())))
			return rc;
	}
	if ((rc = ugrt_buf_reserve(ctx, ctx->sitem, (size_t)xcap * 16)))
		return rc;
	u32 *iseg0 = (u32 *)ctx->sitem.p, *isub0 = iseg0 + xcap;
	iseg1 = isub0 + xcap, isub1 = iseg1 + xcap;
	const bool item_sort = ctx->opt[UGRT_OPT_SHADOW_ITEMSORT] != 0;
	RsFirst hsi = { nullptr };
	if (item_sort && own_sort && (rc = ugrt_sort_first_digit(ctx, &hsi)))
		return rc;
	const u32 ib = (xcap + WL_THREADS - 1) / WL_THREADS, iblocks = ib < 512u ? (ib ? ib : 1u) : 512u;
	if (counted) {
		// the staged ids (tval[1], keys tkey[1]) go to their buckets' runs in tval[0]; the items are listed by the same launch
		const u32 nplace = PAIR_SEGS * 32u; // (8192 waves: what the device holds at once)
		pair_tri = (const u32 *)ctx->tval[0].p;
		hipLaunchKernelGGL(k_pair_place, dim3(nplace + iblocks), dim3(WL_THREADS), 0, st, (const u32 *)segcnt, segcap,
				   (const u32 *)ctx->tkey[1].p, (const u32 *)ctx->tval[1].p, (u32 *)ctx->tval[0].p,
				   (u32)std::min(ctx->tval[0].cap / 4, (size_t)0xFFFFFFF0u), bkt, (const u32 *)bincl, bkt_words, sbits, pgp,
				   (const u32 *)(gincl + (C - 1)), pstart, pend, iblocks, (const u32 *)xincl, Gcap, xcap, (const GBox *)boxes,
				   XSEG, iseg0, isub0, async ? status : (u32 *)nullptr, hsi);
	} else {
		hipLaunchKernelGGL(k_pair_items, dim3(iblocks), dim3(WL_THREADS), 0, st,
				   (const u32 *)xincl, Gcap, xcap, (const u32 *)pstart, (const u32 *)pend, (const GBox *)boxes, XSEG,
				   iseg0, isub0, async ? status : (u32 *)nullptr, hsi);
	}
	UGRT_HIP(hipGetLastError());
	if (item_sort) {
		if ((rc = own_sort ? ugrt_sort_pairs_u32(ctx, iseg0, iseg1, isub0, isub1, xcap, 8, nullptr, true)
				   : ugrt_prim_sort_pairs(ctx, iseg0, iseg1, isub0, isub1, xcap, 8)))
			return rc;
	} else {
		iseg1 = iseg0;
		isub1 = isub0;
	}
	ugrt_prof_end(ctx, UGRT_ST_SHADOW_PREP);
	return UGRT_OK;
}

#ifdef UGRT_SHADOW_TIMELINE
// waits for the exact pass; hdr = { waves, single-item waves, sieve waves, log2 of the XCD run } and two time stamps
// per wave go to the file (tools/shadow_timeline.py)
static int shadow_timeline_dump(hipStream_t st, const unsigned long long *hdr, unsigned long long *tlbuf)
{
	const size_t xwaves = (size_t)hdr[0];
	UGRT_HIP(hipStreamSynchronize(st));
	unsigned long long *h = (unsigned long long *)malloc(xwaves * 16), *none = nullptr;
	UGRT_HIP(hipMemcpy(h, tlbuf, xwaves * 16, hipMemcpyDeviceToHost));
	UGRT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_shadow_tl), &none, sizeof none));
	FILE *f = fopen(getenv("UGRT_SHADOW_TIMELINE_FILE"), "wb");
	if (f) {
		fwrite(hdr, 8, 4, f);
		fwrite(h, 16, xwaves, f);
		fclose(f);
	}
	free(h);
	(void)hipFree(tlbuf);
	return UGRT_OK;
}
#endif

// 4. exact pass
int ShadowPass::exact()
{
	ugrt_prof_begin(ctx, UGRT_ST_TRACE_SHADOW);
	// One wave per item, runs of `x_run` neighbouring items per XCD in turn (as the primary tracer; alone 0.254 -> 0.216
	// ms, profiles/r03_shadow_waves.txt); "shadow_xcd_run" 0 restores round 2's persistent waves ("shadow_waves" of
	// them, which the cull pass always runs on) with a contiguous slice of the list per XCD
	const int x_opt = ctx->opt[UGRT_OPT_SHADOW_XCD_RUN];
	const bool x_persistent = x_opt == 0;
	u32 x_run = x_opt > 0 ? (u32)x_opt : 128u, x_run_log2 = 0;
	while (x_run >> (x_run_log2 + 1u))
		x_run_log2++;
	x_run = 1u << x_run_log2; // (a power of two: rounded down)
	// (the first W0 items - at least the first segments of all sub-groups, of which there are at most rays / 64 + beams -
	// get a wave each, the rest go through sieve waves of `x_sieve` items: see the kernel)
	const u32 x_sieve = ctx->opt[UGRT_OPT_SHADOW_SIEVE] >= 0 ? (u32)ctx->opt[UGRT_OPT_SHADOW_SIEVE] : 8u;
	u32 xw0 = xcap, xnsieve = 0u;
	if (!x_persistent && x_sieve > 1u) {
		const unsigned long long firsts = (unsigned long long)n / 64u + G + 1u; // (asynchronous form: G is the bound the beams were checked against)
		xw0 = firsts < xcap ? (u32)firsts : xcap;
		xnsieve = (xcap - xw0 + x_sieve - 1u) / x_sieve;
	}
	const u32 xwaves = x_persistent ? (u32)launch_blocks_for(xcap, ctx->opt[UGRT_OPT_SHADOW_WAVES])
					: (u32)(((size_t)xw0 + xnsieve + 8u * x_run - 1) / (8u * x_run) * (8u * x_run));
	const u32 xslices = x_persistent ? 1u : (x_run_log2 + 1u) << 1;
#ifdef UGRT_SHADOW_TIMELINE
	const unsigned long long tlhdr[4] = { xwaves, xw0, xnsieve, x_run_log2 };
	unsigned long long *tlbuf = nullptr;
	if (getenv("UGRT_SHADOW_TIMELINE_FILE")) {
		UGRT_HIP(hipMalloc((void **)&tlbuf, (size_t)xwaves * 16));
		UGRT_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_shadow_tl), &tlbuf, sizeof tlbuf, 0, hipMemcpyHostToDevice, st));
		fprintf(stderr, "[shadow timeline] waves %u single-item waves %u sieve waves %u of %u items, %u item slots\n", xwaves, xw0, xnsieve, x_sieve, xcap);
	}
#endif
	hipLaunchKernelGGL(use_rec ? k_trace_shadow<true> : k_trace_shadow<false>, dim3(xwaves), dim3(64), 0, st, ctx->cam,
			   (const u32 *)xincl, Gcap, (const u32 *)iseg1, (const u32 *)isub1, (const GBox *)boxes, (const u32 *)pstart, (const u32 *)pend,
			   pair_tri, d_vertlist, d_trilist, rec, d_t_value, d_ray_dir, d_is_shadowed,
			   (const u32 *)v1, d_cam_position, XSEG, pend + maxg, beam / 64u,
			   (const float4 *)ctx->sray.p, xcap, report, (const u32 *)status, (const unsigned long long *)wcnt, xslices, xw0,
			   x_sieve > 64u ? 64u : x_sieve, xnsieve);
	ugrt_prof_end(ctx, UGRT_ST_TRACE_SHADOW);
	UGRT_HIP(hipGetLastError());
#ifdef UGRT_SHADOW_TIMELINE
	if (tlbuf)
		return shadow_timeline_dump(st, tlhdr, tlbuf);
#endif
	// (the pass's report -- {pairs, beams} as found in the asynchronous form: what the next pass is sized by; the status
	// word; the work counters of ugrt_stats_get -- is in the pinned host words when the stream has got this far: the
	// compaction and the exact pass write it there themselves)
	return UGRT_OK;
}

// check_for_shadows, per_frame_funcs.h:139-159
extern "C" int ugrt_trace_shadow(ugrt_ctx *ctx, const unsigned *d_value_list, const float *d_vertlist,
				 const int *d_trilist, const unsigned *d_span, const unsigned *d_offset,
				 const float *d_t_value, const float *d_ray_dir, int *d_is_shadowed,
				 const unsigned *d_map, const unsigned *d_prefix_map, const float *d_cam_position,
				 unsigned num_chunks)
{
	if (!ctx || !d_value_list || !d_vertlist || !d_trilist || !d_span || !d_offset || !d_t_value || !d_ray_dir ||
	    !d_is_shadowed || !d_map || !d_prefix_map || !d_cam_position)
		return ugrt_fail(UGRT_EINVAL, "trace_shadow: null argument");
	UGRT_HIP(hipSetDevice(ctx->device));
	ShadowPass s = { ctx, ctx->stream, (u32)ctx->cfg.light_nbx * (u32)ctx->cfg.light_nby, (u32)ctx->npix }; // (the rest: zero)
	s.d_value_list = d_value_list, s.d_vertlist = d_vertlist, s.d_trilist = d_trilist;
	s.d_span = d_span, s.d_offset = d_offset, s.d_map = d_map, s.d_prefix_map = d_prefix_map;
	s.d_t_value = d_t_value, s.d_ray_dir = d_ray_dir, s.d_is_shadowed = d_is_shadowed, s.d_cam_position = d_cam_position;
	int rc;
	if ((rc = s.traced_chunks(num_chunks)))
		return rc;
	if (s.traced == 0 || s.n == 0)
		return UGRT_OK;
	s.rec = ugrt_trirec_of(ctx, d_vertlist, d_trilist);
	s.use_rec = s.rec != nullptr;
	if ((rc = s.reserve()) || (rc = s.plan()) || (rc = s.beams()) || (rc = s.cull()))
		return rc;
	if (!s.async && (s.P == 0 || s.G == 0))
		return UGRT_OK;
	if ((rc = s.candidates()))
		return rc;
	return s.exact();
}
