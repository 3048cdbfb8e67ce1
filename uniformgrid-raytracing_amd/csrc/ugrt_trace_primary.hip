// ugrt_trace_primary.hip -- the primary tracer (perspective grid) and its work list.  (The shadow tracer is
// ugrt_trace_shadow.hip, the reflection tracer ugrt_dda.hip / ugrt_dda_walk.hip.)
//
// Mapping to CDNA4: the reference's 8x8-thread CUDA block per grid tile
// (trace_kernel.cu:84, light_kernel.cu:52) is exactly one 64-lane wavefront,
// so "block per cell" becomes "wave per work item" with no multi-wave
// barriers.  A work item is (cell, one segment of that cell's triangles): the
// reference gives a whole cell to one block, and border cells that collect
// every clamped off-screen triangle then serialise the frame;
// here long cells are cut into segments that run on different waves and are
// merged with a 64-bit atomicMin on (t bits << 32 | ref index), which keeps the
// reference's tie-break (strict `<`, first ref in the sorted list wins,
// trace_kernel.cu:38).  Triangles are staged through LDS 64 at a time by the
// wave itself (trace_kernel.cu:151-175) and read back as LDS broadcasts.
// One wave per item is the default: the launch is as long as the work list's upper bound, whose real
// length stays on the device; option "primary_waves" restores the persistent waves of round 2, a launch
// sized to the chip whose waves stride over the list.
#include "ugrt_packet.h"
#include "ugrt_rs_hist.h"
#include "ugrt_scan.h"

struct WItem {
	u32 cell;  // screen cell
	u32 begin; // first ref
	u32 count; // refs in this item (at most one segment)
	u32 multi; // primary: bit 0 = the cell is split across items; bits 1..15 its row, bits 16..31 its column of cells
};

// The context's own screen grid while its merge is put off (ugrt_build.hip: build_defers_merge): the references of a
// cell are its run of the sorted NARROW references followed by the wide triangles, which are the same for every cell
// of the band and are read from their one list.  span[] already counts both.
struct WideSrc {
	const u32 *nvals;  // sorted narrow references
	const u32 *cstart; // per cell: where its run starts in nvals (meaningless for a cell without a run)
	const u32 *span;   // per cell: narrow run + W
	const u32 *wl;     // the W wide triangle ids, in no particular order
	const u32 *rw;     // asynchronous build: {narrow references, wide triangles} on the device; nullptr: W below
	u32 W;
};

// ---------------------------------------------------------------------------
// work lists
// ---------------------------------------------------------------------------
// primary: one entry per cell of the band, x-major like the cell ids.  The list is written by the scan of its
// counts (ugrt_scan.h): the counts are formed where the scan loads them, the items where it has their positions
struct WlPrimaryLoad {
	const u32 *span;
	u32 nby, gy_lo, rows, SEG;
	__device__ __forceinline__ void operator()(u32 base, u32 n, u32 (&v)[SC_ITEMS]) const
	{
#pragma unroll
		for (int k = 0; k < SC_ITEMS; k++) {
			const u32 i = base + (u32)k;
			u32 c = 0;
			if (i < n) {
				const u32 sp = span[(i / rows) * nby + gy_lo + (i % rows)];
				c = sp ? (sp + SEG - 1) / SEG : 1u;
			}
			v[k] = c;
		}
	}
};
// (REL: the context's own grid through a WideSrc -- the items of a cell count from the start of the cell's stream, not
// of the value list)
template <bool REL>
struct WlPrimaryStoreT {
	static constexpr bool active = true;
	const u32 *span, *offset;
	u32 nby, gy_lo, rows, SEG;
	WItem *items;
	u32 *left; // per cell: segment waves of a split cell that have not merged their hits yet (k_trace_primary counts it down)
	__device__ __forceinline__ void operator()(u32 base, u32 n, const u32 (&v)[SC_ITEMS], const u32 (&incl)[SC_ITEMS]) const
	{
		for (int k = 0; k < SC_ITEMS; k++) {
			const u32 i = base + (u32)k;
			if (i >= n)
				break;
			const u32 cx = i / rows, cy = gy_lo + (i % rows);
			const u32 cell = cx * nby + cy;
			const u32 sp = span[cell], off = REL ? 0u : offset[cell], cnt = v[k];
			const u32 first = incl[k] - cnt;
			if (cnt > 1)
				left[cell] = cnt;
			for (u32 s = 0; s < cnt; s++) {
				WItem w;
				w.cell = cell;
				w.begin = off + s * SEG;
				const u32 left = sp - s * SEG;
				w.count = sp ? (left < SEG ? left : SEG) : 0u;
				w.multi = (cnt > 1 ? 1u : 0u) | (cy << 1) | (cx << 16); // (the tracer is spared two integer divisions per item)
				items[first + s] = w;
			}
		}
	}
};

typedef WlPrimaryStoreT<false> WlPrimaryStore;

// ---------------------------------------------------------------------------
// primary rays: rckernel_alpha, trace_kernel.cu:84-270 (NUM_SLABS = 1)
// ---------------------------------------------------------------------------
struct PrimaryOut {
	float *normal;
	float *t_value;
	float *ray_dir;
	int *shadowed;
	int *intersect_id;
};

// trace_kernel.cu:56-82 isWithin + :230-267 epilogue for one pixel.
// `ref` = index into value_list of the nearest accepted triangle (WIDE: the triangle itself), ~0u = none.
template <bool REC, bool WIDE = false>
__device__ __forceinline__ void d_finish_pixel(const CamBlock &cam, const PrimaryOut &o, int pixelID,
					       const float *dir, float oldt, u32 ref,
					       const u32 *__restrict__ value_list, const float *__restrict__ verts,
					       const int *__restrict__ tris, const float4 *__restrict__ rec)
{
	bool ok = false;
	if (ref != 0xFFFFFFFFu) {
		float px = cam.cc[0] + oldt * dir[0];
		float py = cam.cc[1] + oldt * dir[1];
		float pz = cam.cc[2] + oldt * dir[2];
		const float *m = cam.cc;
		float hz = D_MULMV_ROW(m, 48, 2, px, py, pz);
		float hw = D_MULMV_ROW(m, 48, 3, px, py, pz);
		hz /= hw;
		ok = ugrt_floor2i(hz * 1.0f) == 0;
	}
	if (ok) {
		u32 face = WIDE ? ref : value_list[ref];
		float tri[9];
		// the record holds the same two edge subtractions (one 48-B gather instead of three indices + nine floats)
		d_load_triangle<REC>(rec, verts, tris, face, 0.0f, 0.0f, 0.0f, tri);
		float *e1 = &tri[3], *e2 = &tri[6], nrm[3];
		D_NORMALIZE(e1);
		D_NORMALIZE(e2);
		D_CROSS(nrm, e1, e2);
		D_NORMALIZE(nrm);
		nrm[0] = nrm[0] < 0 ? nrm[0] * -1 : nrm[0];
		nrm[1] = nrm[1] < 0 ? nrm[1] * -1 : nrm[1];
		nrm[2] = nrm[2] < 0 ? nrm[2] * -1 : nrm[2];
		o.t_value[pixelID] = oldt;
		o.intersect_id[pixelID] = (int)face;
		o.normal[pixelID * 3 + 0] = nrm[0];
		o.normal[pixelID * 3 + 1] = nrm[1];
		o.normal[pixelID * 3 + 2] = nrm[2];
	} else {
		o.t_value[pixelID] = -1.0f;
		o.intersect_id[pixelID] = -2;
		o.normal[pixelID * 3 + 0] = -1.0f;
		o.normal[pixelID * 3 + 1] = -1.0f;
		o.normal[pixelID * 3 + 2] = -1.0f;
	}
	o.shadowed[pixelID] = 0;
	o.ray_dir[pixelID * 3 + 0] = dir[0];
	o.ray_dir[pixelID * 3 + 1] = dir[1];
	o.ray_dir[pixelID * 3 + 2] = dir[2];
}

#define SURV_CAP 128 // survivors buffered in LDS before the per-lane tests run (flush at >= 64)
#define JOB_CAP (4 * SURV_CAP)
#ifndef JOB_CHUNK
#define JOB_CHUNK 64u // jobs between two looks at the rays' closest hits
#endif

// One wave per item = (8x8-pixel tile, segment of its cell list).  lane = triangle: cull against the
// tile's direction box, then against the boxes of its four 4x4-pixel QUADRANTS; survivors go to LDS once
// and every (survivor, quadrant it may touch) pair becomes a JOB.  lane = (job of the round, ray of that
// job's quadrant): a round runs four jobs of ANY quadrants, so a small triangle costs a quarter of the lanes
// and a tile whose triangles crowd into one quadrant still fills the wave (with one list per quadrant the
// rounds of a flush were those of its longest list: 1.53 M rounds for 2.57 M jobs on the bench frame).
// A ray is then tested by different lanes in different rounds, so its closest hit is merged in LDS as
// min over (t bits << 32 | position in the cell list): the smallest t, and of equal t's the first of the
// list -- what the reference's strict "<" in list order keeps.
// qfar[q] = the largest of the closest-hit distances of quadrant q's 16 rays (lane bits 2 and 5 select the
// quadrant), NaN (bits ~0) while one of them has no hit: positive floats and that sentinel order as unsigned ints
__device__ __forceinline__ void d_quadrant_far(const unsigned long long *s_best, int lane, float *qfar)
{
	// (positive floats and the sentinel ~0 order as unsigned ints; the reduction is made on int images: bit 31 flipped)
	const u32 tb = (u32)d_quadrant_reduce<DOpMax>((int)((u32)(s_best[lane] >> 32) ^ 0x80000000u)) ^ 0x80000000u;
#pragma unroll
	for (int q = 0; q < 4; q++)
		qfar[q] = __uint_as_float((u32)__builtin_amdgcn_readlane((int)tb, ((q & 1) << 2) | ((q & 2) << 4)));
}

// work counters of the COUNT variant (ugrt_stats_primary)
enum { PS_ITEMS, PS_BATCHES, PS_BATCHES_KEPT, PS_REFS, PS_TILE_SURVIVORS, PS_SURVIVORS, PS_JOBS, PS_FLUSHES, PS_ROUNDS,
       PS_ROUNDS_DIV, PS_ROUNDS_V, PS_ROUNDS_T, PS_LANE_TESTS, PS_HITS, PS_PRUNABLE, PS_PRUNED, PS_END };
static_assert(PS_END <= UGRT_PRIMARY_STATS, "primary work counters");

// WIDE: the references come from a WideSrc, and the word that breaks ties between equal t's is the TRIANGLE ID instead
// of the position in the cell's list.  Inside one cell of a grid built here the ids are unique and strictly ascending
// (the fill writes a cell's references in id order, the sort is stable, duplicates are dropped, the merge keeps the
// order), so "the first of the list wins" and "the smaller id wins" are the same rule -- and a minimum over ids does
// not care in which order the stream delivers them, which is what lets the wide triangles come last and unordered.
// The position-keyed instantiations stay for lists a caller supplies, which need not be ascending.
// Registers: launch bounds of FIVE waves per SIMD, 96 registers, although a CU's LDS holds 16 of these one-wave
// workgroups = four per SIMD either way.  In the frame the waves of other streams' kernels share the SIMDs with these, and
// what four waves leave of the 512 registers is what those get: 32 at 120 (113 to 120 registers are allocated as 120),
// 64 at 112, 128 at 96.  Measured on the bench frame, four frames in flight (profiles/primary_finish_bench.txt): 113
// registers 0.7444 ms, 109 registers 0.7331, 96 registers 0.7204, each against 0.735 to 0.738 of the build before.  So
// nothing may be held across the flushes that can be had again: the ray's direction is read back from s_dir, the pixel's
// index is formed at the end, the all-ones word per item.  tools/kernel_resources.py shows the count; 97 would spill.
template <bool REC, bool WIDE, bool COUNT>
__global__ __launch_bounds__(64, 5) void k_trace_primary(CamBlock cam, const float *__restrict__ tex,
						       const WItem *__restrict__ items,
						       const u32 *__restrict__ nitems_p,
						       const u32 *__restrict__ value_list,
						       const float *__restrict__ verts, const int *__restrict__ tris,
						       const float4 *__restrict__ rec, PrimaryOut out,
						       u64 *__restrict__ best, int p0, unsigned long long *__restrict__ counters,
						       u32 ORDER, u32 CHUNK, u32 SLICES, WideSrc ws, u32 *__restrict__ left)
{
	__shared__ __attribute__((aligned(16))) float lds[SURV_CAP * TRI_STRIDE];
	__shared__ unsigned short jobs[JOB_CAP]; // survivor slot | lane offset of the quadrant << 7
	__shared__ unsigned short jobs2[JOB_CAP]; // the same jobs, nearest triangles first (ORDER)
	__shared__ unsigned short ready[64];     // the jobs of the current 64 that are still worth their tests
	__shared__ float s_dir[64 * 3];
	__shared__ unsigned long long s_best[64];
	const int lane = threadIdx.x;
	// a job's 16 rays: lane bits 0,1 (column) and 3,4 (row) inside the quadrant; the quadrant adds bits 2 and 5
	const int group = lane >> 4, rbase = (lane & 3) | (((lane >> 2) & 3) << 3);
	const u32 nitems = *nitems_p;
	const float ex = cam.cc[0], ey = cam.cc[1], ez = cam.cc[2];
	unsigned long long ps[PS_END] = { 0 };
	// SLICES 1: persistent waves, a contiguous slice of the list per XCD; otherwise one wave per item, runs of
	// 2^((SLICES >> 1) - 1) items per XCD in turn (workgroup b runs on XCD b % 8; a power of two: every wave maps its
	// index, and a division by a launch parameter is ~35 instructions)
	u32 first = blockIdx.x;
	if (SLICES == 1u) {
		first = d_xcd_block();
	} else if (SLICES > 1u) {
		const u32 rl = (SLICES >> 1) - 1u, j = blockIdx.x >> 3;
		u32 g = j >> rl; // round of eight runs
		if (SLICES & 1u) {
			// Centre out: the rounds are taken from the middle of the list outwards (mid, mid + 1, mid - 1, ...).  The list is
			// in screen order, column by column, and the cells that cost most (the long lists a camera looks at) sit around the
			// middle of the view: in list order their items start half-way through the launch and ARE its tail (the longest
			// last four times the mean: profiles/r03_primary_timeline.txt); started first they are over when the cheap ones run out.
			const u32 G = (nitems + (8u << rl) - 1u) >> (rl + 3u);
			if (g >= G)
				return;
			const u32 mid = (G - 1u) >> 1;
			g = (g & 1u) ? mid + ((g + 1u) >> 1) : mid - (g >> 1);
		}
		first = (((g << 3) + (blockIdx.x & 7u)) << rl) + (j & ((1u << rl) - 1u));
	}
	for (u32 it = first; it < nitems; it += gridDim.x) {
		const WItem w = items[it];
		if (COUNT) {
			ps[PS_ITEMS]++;
			ps[PS_REFS] += w.count;
		}
		// Two dependent gathers stand before every batch of 64 references (id, then record); issued where
		// they are needed, a wave spends three quarters of a batch waiting for them.  So they run one batch
		// ahead: the records of the next batch and the ids of the one after are in flight while the current
		// one is culled, and the item's first batch while its rays are set up.  (Indices are clamped to the
		// item's last reference instead of being masked: loads under a divergent branch make the compiler
		// wait for everything outstanding at the join.)
		const u32 last = w.count ? w.count - 1u : 0u;
		// WIDE: reference i of the item is number w.begin + i of the cell's stream: narrow run, then the wide list (ONE
		// load from a selected address: see above about loads under divergent branches)
		u32 ns = 0;
		const u32 *np = nullptr;
		if (WIDE) {
			const u32 Wn = ws.rw ? ws.rw[1] : ws.W, sp = ws.span[w.cell];
			ns = sp > Wn ? sp - Wn : 0u;
			np = ws.nvals + ws.cstart[w.cell];
		}
		auto fetch = [&](u32 i) -> u32 {
			if (!WIDE)
				return value_list[w.begin + i];
			const u32 s = w.begin + i;
			return *(s < ns ? np + s : ws.wl + (s - ns));
		};
		u32 id_next = 0, id_rec = 0; // id_rec: the triangle whose record is in ra, rb, rcx
		float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
		float rcx = 0.f;
		if (REC && w.count)
			id_next = fetch(min((u32)lane, last));
		const int bx = (int)(w.multi >> 16), by = (int)((w.multi >> 1) & 0x7FFFu);
		const int col = bx * 8 + (lane & 7), row = by * 8 + (lane >> 3);
		float dir0[3];
		d_ray_dir(cam, tex, col, row, dir0);
		if (REC && w.count) {
			ra = rec[id_next * 3u + 0u];
			rb = rec[id_next * 3u + 1u];
			rcx = reinterpret_cast<const float *>(rec)[id_next * 12u + 8u];
			if (WIDE)
				id_rec = id_next;
			id_next = fetch(min(64u + (u32)lane, last));
		}
		// direction boxes: reduce inside the quadrants (lane bits 0,1,3,4), then across them (bits 2,5);
		// centre and half width are formed per lane and read from one lane of each quadrant, so that
		// the boxes live in scalar registers
		CBox qb[4], tb;
		float qrmax[3]; // the largest of the four quadrants' half widths, per component (d_cull_cr4)
#pragma unroll
		for (int k = 0; k < 3; k++) {
			// (through the order-preserving int images of the floats: integer min / max fold into the DPP instruction)
			const int ilo = d_quadrant_reduce<DOpMin>(d_ordered(dir0[k])), ihi = d_quadrant_reduce<DOpMax>(d_ordered(dir0[k]));
			float lo = d_unordered(ilo), hi = d_unordered(ihi);
			const float qc = 0.5f * (lo + hi);
			const float qr = 0.5f * (hi - lo) * 1.0001f + 1e-6f; // far more than the rounding of c and r
			qrmax[k] = d_readlane(d_unordered(d_across_quadrants<DOpMax>(d_ordered(qr))), 0);
			lo = d_unordered(d_across_quadrants<DOpMin>(ilo));
			hi = d_unordered(d_across_quadrants<DOpMax>(ihi));
			tb.c[k] = d_readlane(0.5f * (lo + hi), 0);
			tb.r[k] = d_readlane(0.5f * (hi - lo) * 1.0001f + 1e-6f, 0);
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const int src = ((q & 1) << 2) | ((q & 2) << 4);
				qb[q].c[k] = d_readlane(qc, src);
				qb[q].r[k] = d_readlane(qr, src);
			}
		}
		s_dir[lane * 3 + 0] = dir0[0];
		s_dir[lane * 3 + 1] = dir0[1];
		s_dir[lane * 3 + 2] = dir0[2];
		{
			// (the all-ones word is made here: as a constant the compiler keeps it in two registers across every flush)
			u32 ones;
			asm volatile("v_mov_b32 %0, -1" : "=v"(ones));
			s_best[lane] = ((unsigned long long)ones << 32) | ones;
		}
		u32 nsurv = 0, njobs = 0;
		// per quadrant: the farthest of its 16 rays' closest hits so far (NaN while a ray has none)
		float qfar[4] = { __uint_as_float(~0u), __uint_as_float(~0u), __uint_as_float(~0u), __uint_as_float(~0u) };
		for (u32 b = 0; b < w.count || nsurv; b += 64) {
			if (b < w.count) {
				const u32 cnt = (w.count - b) < 64u ? (w.count - b) : 64u;
				bool keep = false;
				float t9[9];
				CullTri ct;
				u32 tie = w.begin + b + (u32)lane; // what breaks ties: the position in the list (WIDE: the triangle id)
				if (REC) {
					// (the same subtractions d_load_triangle makes)
					t9[0] = ex - ra.x, t9[1] = ey - ra.y, t9[2] = ez - ra.z;
					t9[3] = ra.w, t9[4] = rb.x, t9[5] = rb.y, t9[6] = rb.z, t9[7] = rb.w, t9[8] = rcx;
					if (WIDE)
						tie = id_rec, id_rec = id_next;
					ra = rec[id_next * 3u + 0u];
					rb = rec[id_next * 3u + 1u];
					rcx = reinterpret_cast<const float *>(rec)[id_next * 12u + 8u];
					id_next = fetch(min(b + 128u + (u32)lane, last));
					if ((u32)lane < cnt) {
						ct = d_cull_prep(&t9[0], &t9[3], &t9[6]);
						keep = !d_cull_cr(ct, tb);
					}
				} else if ((u32)lane < cnt) {
					const u32 face = fetch(b + (u32)lane);
					if (WIDE)
						tie = face;
					d_load_triangle<REC>(rec, verts, tris, face, ex, ey, ez, t9);
					ct = d_cull_prep(&t9[0], &t9[3], &t9[6]);
					keep = !d_cull_cr(ct, tb);
				}
				if (COUNT) {
					ps[PS_BATCHES]++;
					ps[PS_TILE_SURVIVORS] += (u32)__popcll(__ballot(keep));
				}
				// The survivors of the tile cull are staged as they are; their quadrant culls, depth bounds and jobs are
				// made at the flush, lane = staged triangle: there the wave is full, here a batch has ~24 of them on 64 lanes
				// (the ~300 instructions of that part ran 110 k times for the bench frame, they now run 45 k times).
				const unsigned long long mask = __ballot(keep);
				if (mask != 0ull) {
					if (COUNT)
						ps[PS_BATCHES_KEPT]++;
					const u32 slot = nsurv + d_rank_in_mask(mask);
					if (keep) {
						float4 *dst = reinterpret_cast<float4 *>(&lds[slot * TRI_STRIDE]);
						dst[0] = make_float4(t9[0], t9[1], t9[2], t9[3]);
						dst[1] = make_float4(t9[4], t9[5], t9[6], t9[7]);
						dst[2] = make_float4(t9[8], __uint_as_float(tie), 0.0f, 0.0f);
					}
					nsurv += (u32)__popcll(mask);
				}
				if (nsurv < 64u && b + 64 < w.count)
					continue; // keep collecting
			}
			// The jobs are taken 64 at a time.  lane = job: a job whose triangle lies behind the closest hits of all
			// 16 rays of its quadrant is dropped (the rays of the bench scene cross eleven surfaces each; lists are
			// in id order, so most triangles come after a nearer one).  lane = (job, ray): the exact per-ray test
			// of the reference, four of the remaining jobs a round.
			__syncthreads();
			// quadrant culls, depth bounds, jobs: lane = staged triangle
			for (u32 s0 = 0; s0 < nsurv; s0 += 64u) {
				const u32 slot = s0 + (u32)lane;
				u32 km = 0;
				if (slot < nsurv) {
					const float4 *src = reinterpret_cast<const float4 *>(&lds[slot * TRI_STRIDE]);
					const float4 a = src[0], c = src[1];
					const float e2x = lds[slot * TRI_STRIDE + 8u];
					const float tv[3] = { a.x, a.y, a.z }, e1[3] = { a.w, c.x, c.y }, e2[3] = { c.z, c.w, e2x };
					const CullTri ct = d_cull_prep(tv, e1, e2);
					const float tlow = d_cull_tlow(ct, e2, tb);
					const u32 out4 = d_cull_cr4(ct, qb, qrmax);
#pragma unroll
					for (int q = 0; q < 4; q++)
						km |= (((out4 >> q) & 1u) || tlow > qfar[q]) ? 0u : (1u << q);
					lds[slot * TRI_STRIDE + 10u] = tlow;
				}
#pragma unroll
				for (int q = 0; q < 4; q++) {
					const unsigned long long mq = __ballot((km >> q) & 1u);
					const u32 qoff = (u32)(((q & 1) << 2) | ((q & 2) << 4));
					if ((km >> q) & 1u)
						jobs[njobs + d_rank_in_mask(mq)] = (unsigned short)(slot | (qoff << 7));
					njobs += (u32)__popcll(mq);
				}
			}
			__syncthreads();
			if (COUNT) {
				ps[PS_FLUSHES]++;
				ps[PS_SURVIVORS] += nsurv;
				ps[PS_JOBS] += njobs;
			}
			// Front to back.  The cell lists are in id order, so a flush's jobs meet their rays in no particular depth
			// order: 3.3 M of the bench frame's 4.2 M jobs lie behind the hits their quadrant ends the flush with, and
			// the depth bound dropped 0.9 M of them.  The jobs are therefore put in the order of their triangles'
			// lower bounds t_low before they run (a counting sort into 8 buckets of the bounds' float images, by
			// ballots: ~3 exact rounds' worth of instructions per flush), and the rays' closest hits are looked at every
			// CHUNK jobs.  The order only decides what is tested: the closest hits are merged by minimum.
			const unsigned short *jl = jobs;
			if (ORDER && njobs > CHUNK) {
				int kmin = 0x7FFFFFFF, kmax = 0;
				for (u32 j0 = 0; j0 < njobs; j0 += 64u)
					if (j0 + (u32)lane < njobs) {
						const int key = __float_as_int(lds[(jobs[j0 + (u32)lane] & 127u) * TRI_STRIDE + 10u]); // t_low >= 0
						kmin = key < kmin ? key : kmin;
						kmax = key > kmax ? key : kmax;
					}
				kmin = d_wave_imin(kmin);
				kmax = d_wave_imax(kmax);
				const u32 range = (u32)(kmax - kmin);
				const u32 bits = range ? 32u - (u32)__builtin_clz(range) : 0u;
				const u32 sh = bits > 3u ? bits - 3u : 0u; // (key - kmin) >> sh < 8
				u32 base[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
				for (u32 j0 = 0; j0 < njobs; j0 += 64u) {
					const bool valid = j0 + (u32)lane < njobs;
					const u32 bk = valid ? ((u32)(__float_as_int(lds[(jobs[j0 + (u32)lane] & 127u) * TRI_STRIDE + 10u]) - kmin) >> sh) : 8u;
#pragma unroll
					for (u32 k = 0; k < 7u; k++)
						base[k + 1] += (u32)__popcll(__ballot(bk == k));
				}
#pragma unroll
				for (u32 k = 1; k < 8u; k++)
					base[k] += base[k - 1];
				for (u32 j0 = 0; j0 < njobs; j0 += 64u) {
					const bool valid = j0 + (u32)lane < njobs;
					const u32 job = valid ? jobs[j0 + (u32)lane] : 0u;
					const u32 bk = valid ? ((u32)(__float_as_int(lds[(job & 127u) * TRI_STRIDE + 10u]) - kmin) >> sh) : 8u;
					u32 pos = 0;
#pragma unroll
					for (u32 k = 0; k < 8u; k++) {
						const unsigned long long m = __ballot(bk == k);
						if (bk == k)
							pos = base[k] + d_rank_in_mask(m);
						base[k] += (u32)__popcll(m);
					}
					if (valid)
						jobs2[pos] = (unsigned short)job;
				}
				__syncthreads();
				jl = jobs2;
			}
			for (u32 j0 = 0; j0 < njobs; j0 += CHUNK) {
				d_quadrant_far(s_best, lane, qfar);
				bool live = false;
				u32 myjob = 0;
				if ((u32)lane < CHUNK && j0 + (u32)lane < njobs) {
					myjob = jl[j0 + (u32)lane];
					const float tlow = lds[(myjob & 127u) * TRI_STRIDE + 10u];
					const u32 qo = myjob >> 7;
					const float far = qo == 0u ? qfar[0] : (qo == 4u ? qfar[1] : (qo == 32u ? qfar[2] : qfar[3]));
					live = !(tlow > far);
				}
				const unsigned long long lm = __ballot(live);
				const u32 nready = (u32)__popcll(lm);
				if (COUNT)
					ps[PS_PRUNED] += (u32)__popcll(__ballot((u32)lane < CHUNK && j0 + (u32)lane < njobs)) - nready;
				if (live)
					ready[d_rank_in_mask(lm)] = (unsigned short)myjob;
				__syncthreads();
				for (u32 r0 = 0; r0 < nready; r0 += 4u) {
					int stage = -1;
					if (r0 + (u32)group < nready) {
						const u32 job = ready[r0 + (u32)group];
						const int home = rbase | (int)(job >> 7);
						const float4 *src = reinterpret_cast<const float4 *>(&lds[(job & 127u) * TRI_STRIDE]);
						const float4 a = src[0], c = src[1], e = src[2];
						const float tv[3] = { a.x, a.y, a.z }, e1[3] = { a.w, c.x, c.y }, e2[3] = { c.z, c.w, e.x };
						const float rd[3] = { s_dir[home * 3 + 0], s_dir[home * 3 + 1], s_dir[home * 3 + 2] };
						const float v = d_intersect_tri_uv(tv, e1, e2, rd, 99999999.9f);
						if (v != 0.0f)
							atomicMin(&s_best[home], ((unsigned long long)__float_as_uint(v) << 32) |
											 (unsigned long long)__float_as_uint(e.y));
						if (COUNT)
							stage = v != 0.0f ? 4 : d_mt_stage(tv, e1, e2, rd);
					}
					if (COUNT) {
						ps[PS_ROUNDS]++;
						ps[PS_ROUNDS_DIV] += __ballot(stage >= 1) != 0ull;
						ps[PS_ROUNDS_V] += __ballot(stage >= 2) != 0ull;
						ps[PS_ROUNDS_T] += __ballot(stage >= 3) != 0ull;
						ps[PS_LANE_TESTS] += (u32)__popcll(__ballot(stage >= 0));
						ps[PS_HITS] += (u32)__popcll(__ballot(stage == 4));
					}
				}
				__syncthreads();
			}
			d_quadrant_far(s_best, lane, qfar); // for the culls of the batches to come
			if (COUNT) {
				// what a front-to-back order of the flush's jobs could have dropped: jobs whose triangle lies behind the
				// closest hits their quadrant ends up with (PS_PRUNED: the jobs the depth bound did drop in list order)
				for (u32 j0 = 0; j0 < njobs; j0 += 64u) {
					bool behind = false;
					if (j0 + (u32)lane < njobs) {
						const u32 job = jobs[j0 + (u32)lane];
						const float tlow = lds[(job & 127u) * TRI_STRIDE + 10u];
						const u32 qo = job >> 7;
						const float far = qo == 0u ? qfar[0] : (qo == 4u ? qfar[1] : (qo == 32u ? qfar[2] : qfar[3]));
						behind = tlow > far;
					}
					ps[PS_PRUNABLE] += (u32)__popcll(__ballot(behind));
				}
			}
			__syncthreads();
			nsurv = 0;
			njobs = 0;
		}
		const unsigned long long mine = s_best[lane];
		const int pixelID = (by * 8 + (lane >> 3)) * cam.W + bx * 8 + (lane & 7);
		// (the ray's direction is read back from where the rounds read it: three registers less across the flushes)
		const float dir[3] = { s_dir[lane * 3 + 0], s_dir[lane * 3 + 1], s_dir[lane * 3 + 2] };
		if (!(w.multi & 1u)) {
			const bool hit = mine != ~0ull;
			d_finish_pixel<REC, WIDE>(cam, out, pixelID, dir, hit ? __uint_as_float((u32)(mine >> 32)) : 99999999.9f,
					    hit ? (u32)mine : 0xFFFFFFFFu, value_list, verts, tris, rec);
		} else {
			// A split cell: the segments' waves merge their hits in best[], and the one that arrives last finishes the
			// tile.  left[cell] holds the number of the cell's segments (the work list's scan wrote it with the items).  Every
			// wave waits until its atomics have been acknowledged, then takes 1 off; the wave whose subtraction returns 1
			// knows that all others have subtracted, so that their minima are in: it takes each pixel's merged word with an
			// exchange against ~0 (which re-arms the slot) and finishes the pixel.  The counter is then 0, as it is between
			// traces.  Nobody waits for anybody, and the order of the waves does not matter.
			// What is handed over are device-scope atomics on both sides, performed in L2 and beyond, so no cache has to be
			// written back (as for the scans' last tile, ugrt_scan.h): a release fence here writes back every dirty line of
			// the XCD's L2, the finished pixels of all other tiles, once per split item, and the frame was 1 % slower for it.
			unsigned long long *slot = reinterpret_cast<unsigned long long *>(&best[pixelID - p0]);
			if (mine != ~0ull)
				atomicMin(slot, mine);
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			u32 before = 0;
			if (lane == 0)
				before = __hip_atomic_fetch_sub(left + w.cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			before = (u32)__builtin_amdgcn_readfirstlane((int)before);
			if (before == 1u) {
				__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
				const unsigned long long m = __hip_atomic_exchange(slot, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				const bool hit = m != ~0ull;
				d_finish_pixel<REC, WIDE>(cam, out, pixelID, dir, hit ? __uint_as_float((u32)(m >> 32)) : 99999999.9f,
						    hit ? (u32)m : 0xFFFFFFFFu, value_list, verts, tris, rec);
			}
		}
	}
	if (COUNT && lane == 0)
		for (int i = 0; i < PS_END; i++)
			if (ps[i])
				atomicAdd(&counters[i], ps[i]);
}

template <bool REC>
__global__ __launch_bounds__(64) void k_trace_primary_slabs(CamBlock cam, const float *__restrict__ tex, int slabs,
							     int gy_lo, int rows, u32 ntiles,
							     const u32 *__restrict__ span, const u32 *__restrict__ offset,
							     const u32 *__restrict__ value_list,
							     const float *__restrict__ verts, const int *__restrict__ tris,
							     const float4 *__restrict__ rec, PrimaryOut out)
{
	__shared__ __attribute__((aligned(16))) float lds[64 * TRI_STRIDE];
	const int lane = threadIdx.x;
	const float ex = cam.cc[0], ey = cam.cc[1], ez = cam.cc[2];
	for (u32 it = d_xcd_block(); it < ntiles; it += gridDim.x) {
		const int bx = (int)(it / (u32)rows), by = gy_lo + (int)(it % (u32)rows);
		const u32 cell = (u32)bx * (u32)cam.nby + (u32)by;
		const int col = bx * 8 + (lane & 7), row = by * 8 + (lane >> 3);
		const int pixelID = row * cam.W + col;
		float dir[3];
		d_ray_dir(cam, tex, col, row, dir);
		CBox tb;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			const float lo = d_wave_fmin(dir[k]), hi = d_wave_fmax(dir[k]);
			tb.c[k] = 0.5f * (lo + hi);
			tb.r[k] = 0.5f * (hi - lo) * 1.0001f + 1e-6f;
		}
		float oldt = 99999999.9f;
		u32 ref = 0xFFFFFFFFu;
		int rayDone = 0;
		for (int slab = 0; slab < slabs; slab++) {
			const u32 sp = span[cell * (u32)slabs + (u32)slab], off = offset[cell * (u32)slabs + (u32)slab];
			for (u32 b = 0; b < sp; b += 64u) {
				const u32 cnt = (sp - b) < 64u ? (sp - b) : 64u;
				bool keep = false;
				float t9[9];
				if ((u32)lane < cnt) {
					d_load_triangle<REC>(rec, verts, tris, value_list[off + b + lane], ex, ey, ez, t9);
					const CullTri ct = d_cull_prep(&t9[0], &t9[3], &t9[6]);
					keep = !d_cull_cr(ct, tb);
				}
				const unsigned long long mask = __ballot(keep);
				const u32 nsurv = (u32)__popcll(mask);
				__syncthreads();
				if (keep) {
					float4 *dst = reinterpret_cast<float4 *>(&lds[d_rank_in_mask(mask) * TRI_STRIDE]);
					dst[0] = make_float4(t9[0], t9[1], t9[2], t9[3]);
					dst[1] = make_float4(t9[4], t9[5], t9[6], t9[7]);
					dst[2] = make_float4(t9[8], __uint_as_float(off + b + lane), 0.0f, 0.0f);
				}
				__syncthreads();
				if (rayDone != 2) {
					for (u32 k = 0; k < nsurv; k++) {
						const float4 *src = reinterpret_cast<const float4 *>(&lds[k * TRI_STRIDE]);
						const float4 a = src[0], c = src[1], e = src[2];
						const float tv[3] = { a.x, a.y, a.z }, e1[3] = { a.w, c.x, c.y }, e2[3] = { c.z, c.w, e.x };
						const float v = d_intersect_tri_uv(tv, e1, e2, dir, oldt);
						if (v != 0.0f) {
							oldt = v;
							rayDone = 1;
							ref = __float_as_uint(e.y);
						}
					}
				}
			}
			// isWithin, trace_kernel.cu:56-82
			if (rayDone == 0 || rayDone == 2) {
				rayDone = 0;
			} else {
				const float px = ex + oldt * dir[0], py = ey + oldt * dir[1], pz = ez + oldt * dir[2];
				const float *m = cam.cc;
				float hz = D_MULMV_ROW(m, 48, 2, px, py, pz);
				const float hw = D_MULMV_ROW(m, 48, 3, px, py, pz);
				hz /= hw;
				rayDone = ugrt_floor2i(hz * (float)slabs) == slab ? 2 : 1;
			}
			if (__ballot(rayDone != 2) == 0ull)
				break; // the beam is done, trace_kernel.cu:217-228
		}
		if (rayDone == 2) {
			const u32 face = value_list[ref];
			float tri[9];
			d_load_triangle<REC>(rec, verts, tris, face, 0.0f, 0.0f, 0.0f, tri);
			float *e1 = &tri[3], *e2 = &tri[6], nrm[3];
			D_NORMALIZE(e1);
			D_NORMALIZE(e2);
			D_CROSS(nrm, e1, e2);
			D_NORMALIZE(nrm);
			nrm[0] = nrm[0] < 0 ? nrm[0] * -1 : nrm[0];
			nrm[1] = nrm[1] < 0 ? nrm[1] * -1 : nrm[1];
			nrm[2] = nrm[2] < 0 ? nrm[2] * -1 : nrm[2];
			out.t_value[pixelID] = oldt;
			out.intersect_id[pixelID] = (int)face;
			out.normal[pixelID * 3 + 0] = nrm[0];
			out.normal[pixelID * 3 + 1] = nrm[1];
			out.normal[pixelID * 3 + 2] = nrm[2];
		} else {
			out.t_value[pixelID] = -1.0f;
			out.intersect_id[pixelID] = -2;
			out.normal[pixelID * 3 + 0] = -1.0f;
			out.normal[pixelID * 3 + 1] = -1.0f;
			out.normal[pixelID * 3 + 2] = -1.0f;
		}
		out.shadowed[pixelID] = 0;
		out.ray_dir[pixelID * 3 + 0] = dir[0];
		out.ray_dir[pixelID * 3 + 1] = dir[1];
		out.ray_dir[pixelID * 3 + 2] = dir[2];
	}
}

// total refs behind a span/offset pair: known for the context's own grids,
// read back (one 8-byte copy) for arrays that came from elsewhere
static int refs_of(ugrt_ctx *ctx, const u32 *d_span, const u32 *d_offset, u32 C, u32 *R)
{
	for (int g = 0; g < 3; g++)
		if (ctx->grid[g].valid && d_span == (const u32 *)ctx->grid[g].span.p &&
		    d_offset == (const u32 *)ctx->grid[g].offset.p) {
			*R = ctx->grid[g].R;
			return UGRT_OK;
		}
	UGRT_HIP(hipMemcpyAsync(ctx->h_pinned + UGRT_PIN_REFS, d_span + (C - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
	UGRT_HIP(hipMemcpyAsync(ctx->h_pinned + UGRT_PIN_REFS + 1, d_offset + (C - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
	UGRT_HIP(hipStreamSynchronize(ctx->stream));
	*R = ctx->h_pinned[UGRT_PIN_REFS] + ctx->h_pinned[UGRT_PIN_REFS + 1];
	return UGRT_OK;
}

// the kernel of a trace, in its position-keyed or id-keyed (WideSrc) instantiations
typedef void (*TraceKernel)(CamBlock, const float *, const WItem *, const u32 *, const u32 *, const float *, const int *,
			    const float4 *, PrimaryOut, u64 *, int, unsigned long long *, u32, u32, u32, WideSrc, u32 *);
template <bool WIDE>
static TraceKernel trace_kernel_of(bool use_rec, bool counting)
{
	return counting ? (use_rec ? k_trace_primary<true, WIDE, true> : k_trace_primary<false, WIDE, true>)
			: (use_rec ? k_trace_primary<true, WIDE, false> : k_trace_primary<false, WIDE, false>);
}

// FrustumTracer::trace, frustum_tracer.h:35-58.  wide: null = the references are value_list[offset[c] ...]; otherwise
// the context's own screen grid with its merge put off (d_value_list is then not read)
static int trace_primary_run(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
			     const unsigned *d_offset, float *d_normal, float *d_t_value, float *d_ray_dir,
			     int *d_shadowed, int *d_intersect_id, const float *d_vertlist, const int *d_trilist,
			     const WideSrc *wide)
{
	UGRT_HIP(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	const int rows = ctx->cfg.row_end - ctx->cfg.row_begin;
	const u32 ncell = (u32)ctx->nbx * (u32)rows;
	const u32 C = (u32)ctx->nbx * (u32)ctx->nby;
	const float *tex = ugrt_ctx_tex(ctx); // (stores the current camera's direction table first, if it is new)
	// the kernels' REC variants gather the context's triangle records, if those were made of these arrays
	const float4 *rec = ugrt_trirec_of(ctx, d_vertlist, d_trilist);
	const bool use_rec = rec != nullptr;
	const PrimaryOut out = { d_normal, d_t_value, d_ray_dir, d_shadowed, d_intersect_id };
	if (ctx->cfg.slabs > 1) { // NUM_SLABS > 1: the slab walk of trace_kernel.cu:132-229, one wave per tile
		ugrt_prof_begin(ctx, UGRT_ST_TRACE_PRIMARY);
		hipLaunchKernelGGL(use_rec ? k_trace_primary_slabs<true> : k_trace_primary_slabs<false>,
				   dim3(launch_blocks_for(ncell)), dim3(64), 0, st, ctx->cam, tex, ctx->cfg.slabs,
				   ctx->cfg.row_begin, rows, ncell, d_span, d_offset, d_value_list, d_vertlist, d_trilist, rec, out);
		ugrt_prof_end(ctx, UGRT_ST_TRACE_PRIMARY);
		UGRT_HIP(hipGetLastError());
		return UGRT_OK;
	}
	u32 R = 0;
	int rc = refs_of(ctx, d_span, d_offset, C, &R);
	if (rc)
		return rc;
	// triangles per work item: long cells are cut into segments that run on different waves and are
	// merged with atomicMin, the last of them to arrive finishes the tile; cells up to SEG triangles finish inside their one wave.
	// Every cell of a closed scene carries the few hundred eye-plane-straddling triangles (Q9), so the
	// cut-off sits above that baseline.
	u32 SEG = ctx->opt[UGRT_OPT_PRIMARY_SEG] > 0 ? (u32)ctx->opt[UGRT_OPT_PRIMARY_SEG] : 1024u;
	SEG = SEG < 64u ? 64u : (SEG + 63u) / 64u * 64u;
	const size_t cap = (size_t)ncell + R / SEG + 1;
	if ((rc = ugrt_buf_reserve(ctx, ctx->wscan, (size_t)ncell * 4)))
		return rc;
	if ((rc = ugrt_buf_reserve(ctx, ctx->witems, cap * sizeof(WItem))))
		return rc;
	u32 *incl = (u32 *)ctx->wscan.p;
	WItem *items = (WItem *)ctx->witems.p;
	const WideSrc ws = wide ? *wide : WideSrc{ nullptr, nullptr, nullptr, nullptr, nullptr, 0u };
	ugrt_prof_begin(ctx, UGRT_ST_WORKLIST);
	{
		const WlPrimaryLoad load = { d_span, (u32)ctx->nby, (u32)ctx->cfg.row_begin, (u32)rows, SEG };
		const WlPrimaryStore store = { d_span, d_offset, (u32)ctx->nby, (u32)ctx->cfg.row_begin, (u32)rows, SEG, items, (u32 *)ctx->pdone.p };
		const WlPrimaryStoreT<true> store_rel = { d_span, d_offset, (u32)ctx->nby, (u32)ctx->cfg.row_begin, (u32)rows, SEG, items, (u32 *)ctx->pdone.p };
		if ((rc = wide ? ugrt_scan_launch<true>(ctx, load, incl, ncell, ScanTailNone(), store_rel)
			       : ugrt_scan_launch<true>(ctx, load, incl, ncell, ScanTailNone(), store)))
			return rc;
	}
	ugrt_prof_end(ctx, UGRT_ST_WORKLIST);
	UGRT_HIP(hipGetLastError());
	// One wave per work item, in list order: the dispatcher then evens out items of unequal cost by itself.  (Round 2
	// gave 16384 persistent waves two items each, in contiguous slices of the list per XCD for the sake of its L2: 0.305
	// ms alone on the 1 M-triangle frame, with a tail of long second items and of the XCD that holds the heavy screen
	// region - profiles/r03_primary_timeline.txt.  One item per wave in those slices 0.349, two per wave dealt item by
	// item over the XCDs 0.326, one per wave so dealt 0.254; profiles/r03_primary_waves.txt.)  "primary_waves" restores the
	// persistent form with that many waves.
	const bool p_slices = ctx->opt[UGRT_OPT_PRIMARY_WAVES] > 0;
	// (what an XCD gets are runs of `p_run` neighbouring items - neighbours share triangles and the XCD's L2 -, run r
	// going to XCD r % 8; 0 = item i to XCD i % 8.  128: the 1 M-triangle frame is indifferent up to 256 (0.254-0.258
	// ms, 0.278 at 1024), the 79 k-triangle hall, whose items cost the same, likes them long (0.126 at 0-32, 0.119 at
	// 128, 0.115 at 2048, 0.113 in the slices))
	u32 p_run = ctx->opt[UGRT_OPT_PRIMARY_XCD_RUN] >= 0 ? (u32)ctx->opt[UGRT_OPT_PRIMARY_XCD_RUN] : 128u;
	u32 p_run_log2 = 0;
	while (p_run >> (p_run_log2 + 1u))
		p_run_log2++;
	p_run = p_run ? 1u << p_run_log2 : 0u; // (a power of two: rounded down)
	size_t one_each = cap;
	if (p_run)
		one_each = (cap + 8u * p_run - 1) / (8u * p_run) * (8u * p_run); // (a whole number of rounds of runs: the mapping is a permutation)
	const int pwaves = p_slices ? launch_blocks_for((u32)cap, ctx->opt[UGRT_OPT_PRIMARY_WAVES]) : (int)(one_each < 0x7FFFFFFFu ? one_each : 0x7FFFFFFFu);
	ugrt_prof_begin(ctx, UGRT_ST_TRACE_PRIMARY);
	const bool counting = (ctx->cfg.flags & UGRT_FLAG_COUNT_WORK) != 0;
	unsigned long long *pc = (unsigned long long *)(ctx->d_small + UGRT_DSMALL_PRIMARY);
	// launch shape of the flushes (no effect on results): jobs nearest first, closest hits looked at every p_chunk jobs
	const u32 p_order = ctx->opt[UGRT_OPT_PRIMARY_ORDER] == 0 ? 0u : 1u;
	u32 p_chunk = ctx->opt[UGRT_OPT_PRIMARY_CHUNK] > 0 ? (u32)ctx->opt[UGRT_OPT_PRIMARY_CHUNK] : (p_order ? 32u : 64u);
	p_chunk = p_chunk > 64u ? 64u : (p_chunk < 4u ? 4u : p_chunk);
	const TraceKernel kernel = wide ? trace_kernel_of<true>(use_rec, counting) : trace_kernel_of<false>(use_rec, counting);
	if (counting)
		UGRT_HIP(hipMemsetAsync(pc, 0, UGRT_PRIMARY_STATS * 8, st));
	hipLaunchKernelGGL(kernel, dim3(pwaves), dim3(64), 0, st, ctx->cam, tex, (const WItem *)items,
			   (const u32 *)(incl + (ncell - 1)), d_value_list, d_vertlist, d_trilist, rec, out, (u64 *)ctx->best.p,
			   ctx->p0, pc, p_order, p_chunk,
			   p_slices ? 1u : (p_run ? ((p_run_log2 + 1u) << 1) | (ctx->opt[UGRT_OPT_PRIMARY_CENTRE] != 0 ? 1u : 0u) : 0u), ws,
			   (u32 *)ctx->pdone.p);
	if (counting)
		UGRT_HIP(hipMemcpyAsync(ctx->primary_stats, pc, UGRT_PRIMARY_STATS * 8, hipMemcpyDeviceToHost, st));
	ugrt_prof_end(ctx, UGRT_ST_TRACE_PRIMARY);
	UGRT_HIP(hipGetLastError());
	ctx->stats[0] = cap; // upper bound of primary work items
	return UGRT_OK;
}

extern "C" int ugrt_trace_primary(ugrt_ctx *ctx, const unsigned *d_value_list, const unsigned *d_span,
				  const unsigned *d_offset, float *d_normal, float *d_t_value, float *d_ray_dir,
				  int *d_shadowed, int *d_intersect_id, const float *d_vertlist, const int *d_trilist)
{
	if (!ctx || !d_value_list || !d_span || !d_offset || !d_normal || !d_t_value || !d_ray_dir || !d_shadowed ||
	    !d_intersect_id || !d_vertlist || !d_trilist)
		return ugrt_fail(UGRT_EINVAL, "trace_primary: null argument");
	// the context's own screen-grid arrays (pointers kept from an earlier ugrt_grid_get_info: the buffers rarely move)
	// while the merge of the last build is put off: the value list is about to be read, so it is written first
	Grid &G = ctx->grid[UGRT_GRID_PERSPECTIVE];
	if (G.valid && G.merge_pending && d_value_list == (const unsigned *)G.vals && d_span == (const unsigned *)G.span.p &&
	    d_offset == (const unsigned *)G.offset.p)
		if (int rc = ugrt_grid_complete(ctx, G))
			return rc;
	return trace_primary_run(ctx, d_value_list, d_span, d_offset, d_normal, d_t_value, d_ray_dir, d_shadowed,
				 d_intersect_id, d_vertlist, d_trilist, nullptr);
}

// The same trace through the context's current screen grid, without asking for its lists: while the merge of the last
// ugrt_grid_build_perspective is put off, the tracer reads the sorted narrow references and the one list of wide
// triangles, and the merged lists are never written.  Otherwise (no wide triangle, z slabs, a merge that has been
// carried out) this is ugrt_trace_primary on the grid's arrays.
extern "C" int ugrt_trace_primary_grid(ugrt_ctx *ctx, float *d_normal, float *d_t_value, float *d_ray_dir,
				       int *d_shadowed, int *d_intersect_id, const float *d_vertlist, const int *d_trilist)
{
	if (!ctx || !d_normal || !d_t_value || !d_ray_dir || !d_shadowed || !d_intersect_id || !d_vertlist || !d_trilist)
		return ugrt_fail(UGRT_EINVAL, "trace_primary_grid: null argument");
	Grid &G = ctx->grid[UGRT_GRID_PERSPECTIVE];
	if (!G.valid)
		return ugrt_fail(UGRT_EINVAL, "trace_primary_grid: the perspective grid has not been built");
	const WideSrc ws = { (const u32 *)G.val[1].p, (const u32 *)G.span.p + G.C, (const u32 *)G.span.p, (const u32 *)G.wide.p,
			     (const u32 *)G.merge_plan.rw, G.merge_plan.W };
	return trace_primary_run(ctx, (const unsigned *)G.vals, (const unsigned *)G.span.p, (const unsigned *)G.offset.p, d_normal,
				 d_t_value, d_ray_dir, d_shadowed, d_intersect_id, d_vertlist, d_trilist,
				 (G.merge_pending && ctx->cfg.slabs == 1) ? &ws : nullptr);
}

// work counters of the primary tracer's last counting launch (UGRT_FLAG_COUNT_WORK), in the order of the PS_* enum
extern "C" int ugrt_stats_primary(ugrt_ctx *ctx, unsigned long long *stats, int n)
{
	if (!ctx || !stats || n < 0)
		return ugrt_fail(UGRT_EINVAL, "stats_primary: bad argument");
	UGRT_HIP(hipSetDevice(ctx->device));
	UGRT_HIP(hipStreamSynchronize(ctx->stream));
	for (int i = 0; i < n; i++)
		stats[i] = i < UGRT_PRIMARY_STATS ? ctx->primary_stats[i] : 0ull;
	return UGRT_OK;
}
