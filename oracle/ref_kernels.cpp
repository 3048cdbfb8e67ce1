// ref_kernels -- test-infrastructure driver around the REFERENCE's own CUDA kernels, compiled as host C++.
//
// oracle/Makefile target "ref" builds it where the reference checkout is present: this file and ref_shim.h are
// ours; main.cu.h and the *_kernel.cu files are #included straight from the checkout and are not modified.
// tests/test_reference_kernels.py feeds every stage the CPU oracle's inputs for that stage and requires the
// kernel's outputs to equal the oracle's (and the records under tests/golden/, tests/golden/make_ref_kernels.py).
//
// Launches:
// * barrier-free kernels run as plain (blockIdx, threadIdx) loops;
// * rckernel_alpha and mod_light_rckernel run as 64 fibers (ucontext) per block that switch at __syncthreads: a
//   block runs each barrier interval of every thread in turn.  The launch runs every interval once in forward and
//   once in reverse thread order (two runs on separate output copies); the stage reports whether they agree, so a
//   result that depends on the schedule (a race between barriers) shows up as itself;
// * blocks are spread over at most 16 worker threads;
// * shared memory: every block gets its launched size, zeroed (on the GPU it is undefined), followed by a guard
//   zone holding a canary; writes into the guard zone are counted and reported (the least and the most bytes past
//   the launched size over the blocks that overran).  The guard zone lies inside the same array, so AddressSanitizer
//   cannot see such a write: the canary is what detects it.
//
// Image size: main.cu.h fixes SCREEN_WIDTH/HEIGHT at 1024 and NUM_BLOCKS_X/Y at 128 = the image's 8x8 tiles, which
// are also the light grid's cells (mapSort_Effective_kernel uses one constant for both).  Here they are runtime
// globals: W x H, NUM_BLOCKS = (W/8, H/8) for the perspective stages and the light grid's dimensions for the
// spherical ones; NUM_SLABS is 1 unless the input names it ("slabs": the z-slab build, "slab" stage, its bounds, and
// the traces over it, "primary" and "shadow"); every stage that sets it restores 1.  MAX_TRIANGLES and the 8x8
// thread shape stay as the reference has them.
//
// Platform maths: see ref_shim.h.  A float -> int cast written as a cast in the kernel text, (int)((angle / max) *
// (NUM_BLOCKS_X / 2)) in getEffective_x/y (grid_kernel.cu) and the colour stores of lambertian_shade, is x86's here
// (INT_MIN for NaN and out-of-range values) where CUDA truncates to 0 / saturates: the fixture inputs keep those
// operands finite and in range (no vertex and no hit point on the light's position).
//
// Reference behaviours that read out of bounds are given defined values, as the oracle defines them:
// the light grid's sentinel cell (Q11) gets span = offset = 0 (NUM_SLABS extra entries: the kernel reads
// blockcnt[C * NUM_SLABS + p] for every p), and the material index of a miss,
// mat_idx[-2] (Q17, shader_kernel.cu:170), is -2, that of an id of -1 is -1 (two entries in front of the list).
//
// I/O: one binary input file (named arrays; "stage" names the stage) -> one binary output file in the same format
// (tests/oracle_lib.py: write_ref_io / read_ref_io):
//   "UGRK", u32 count, then per array: u32 name length, name, u8 type ('f' f32, 'i' i32, 'u' u32, 'b' u8),
//   u64 element count, data.
// Usage: ref_kernels in.bin out.bin; ref_kernels --stamp prints the hash of this file and ref_shim.h it was built
// from (oracle/Makefile), so that a binary left from other sources is recognised as such.
#include <stdint.h>
#include <ucontext.h>

#include <atomic>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "ref_shim.h"

// ---------------------------------------------------------------------------------------------------------------
// run-time image / grid geometry (replaces main.cu.h's compile-time constants after its #include)
static int g_W = 1024, g_H = 1024, g_nbx = 128, g_nby = 128, g_slabs = 1;

thread_local ref_uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;

enum { SHM_WORDS = 8192, GUARD_WORDS = 4096 };
static const int CANARY = 0x5a17c0de;
thread_local int sharedmem[SHM_WORDS + GUARD_WORDS];

#include "main.cu.h"
#undef SCREEN_WIDTH
#undef SCREEN_HEIGHT
#undef NUM_BLOCKS_X
#undef NUM_BLOCKS_Y
#define SCREEN_WIDTH g_W
#define SCREEN_HEIGHT g_H
#define NUM_BLOCKS_X g_nbx
#define NUM_BLOCKS_Y g_nby
#undef NUM_SLABS
#define NUM_SLABS g_slabs

#include "grid_kernel.cu"
#include "trace_kernel.cu"
#include "light_kernel.cu"
#include "misc_kernel.cu"
#include "shader_kernel.cu"
#include "transformation_kernel.cu"

// ---------------------------------------------------------------------------------------------------------------
// texture fetch: pinned by DEFINITION, not by the reference, whose texture unit is not available.
// The default form is the exact float bilinear interpolation at texel coordinate 4*ftx of the calling thread's pixel,
// as the oracle's ray set-up computes it; the kernel's own coordinate (ftx*0.8+0.1) is checked against that pixel.
// UGRT_FLAG_STRICT_TEXTURE ("strict_texture" input) uses ugrt_tex_linear8 on the coordinate the kernel passes.
static const float *g_tex;
static int g_strict_texture;
static std::atomic<long> g_tex_coord_mismatch(0);

float4 ref_tex2D(float x, float y)
{
	int col = blockIdx.x * NUM_THREADS_X + threadIdx.x, row = blockIdx.y * NUM_THREADS_Y + threadIdx.y;
	float ftx = 1 - (float)col / (float)g_W, fty = (float)row / (float)g_H;
	if (fabsf(x - (ftx * 0.8f + 0.1f)) > 1e-6f || fabsf(y - (fty * 0.8f + 0.1f)) > 1e-6f)
		g_tex_coord_mismatch++;
	float xs = ftx * 4.0f, ys = fty * 4.0f, a, b;
	int i = ugrt_f2i(xs), j = ugrt_f2i(ys);
	if (i > 3)
		i = 3;
	if (j > 3)
		j = 3;
	a = xs - (float)i;
	b = ys - (float)j;
	if (g_strict_texture) {
		ugrt_tex_linear8(x, 5, &i, &a);
		ugrt_tex_linear8(y, 5, &j, &b);
	}
	float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b, T[3];
	for (int k = 0; k < 3; k++) {
		float t00 = g_tex[(j * 5 + i) * 4 + k], t10 = g_tex[(j * 5 + i + 1) * 4 + k];
		float t01 = g_tex[((j + 1) * 5 + i) * 4 + k], t11 = g_tex[((j + 1) * 5 + i + 1) * 4 + k];
		T[k] = ((w00 * t00 + w10 * t10) + w01 * t01) + w11 * t11;
	}
	float4 r = { T[0], T[1], T[2], 0.0f };
	return r;
}

// getEffective_x/y cast (angle / max) * (NUM_BLOCKS / 2) to an integer; a NaN angle gives 0 on CUDA, INT_MIN here
static std::atomic<long> g_acos_nan(0);
float ref_acosf(float x)
{
	float r = ugrt_acosf(x);
	if (r != r)
		g_acos_nan++;
	return r;
}

// ---------------------------------------------------------------------------------------------------------------
// launches
enum { MAX_BLOCK_THREADS = 256, FIBER_STACK = 64 * 1024, MAX_WORKERS = 16 };

struct Worker {
	ucontext_t sched;
	ucontext_t fib[MAX_BLOCK_THREADS];
	int done[MAX_BLOCK_THREADS];
	int cur = 0;
	bool in_fiber = false;
	std::vector<char> stacks;
	const std::function<void()> *kernel = nullptr;
};
static thread_local Worker *tw;

static bool g_reverse;
static std::atomic<long> g_overrun_blocks(0), g_divergent_barriers(0);
static std::atomic<int> g_overrun_bytes(0), g_overrun_min_bytes(1 << 30);

void __syncthreads()
{
	if (tw && tw->in_fiber)
		swapcontext(&tw->fib[tw->cur], &tw->sched);
}

static void fiber_entry()
{
	Worker *w = tw;
	(*w->kernel)();
	w->done[w->cur] = 1; // returns to uc_link = the scheduler
}

static void set_thread(int t)
{
	threadIdx.x = t % blockDim.x;
	threadIdx.y = (t / blockDim.x) % blockDim.y;
	threadIdx.z = t / (blockDim.x * blockDim.y);
}

static void run_block(Worker &w, unsigned lin, int shm_words, bool fibers)
{
	blockIdx.x = lin % gridDim.x;
	blockIdx.y = lin / gridDim.x;
	blockIdx.z = 0;
	memset(sharedmem, 0, sizeof(int) * shm_words);
	for (int i = 0; i < GUARD_WORDS; i++)
		sharedmem[shm_words + i] = CANARY;
	int n = blockDim.x * blockDim.y * blockDim.z;
	if (!fibers) {
		for (int t = 0; t < n; t++) {
			set_thread(t);
			(*w.kernel)();
		}
	} else {
		if (w.stacks.empty())
			w.stacks.resize((size_t)MAX_BLOCK_THREADS * FIBER_STACK);
		for (int t = 0; t < n; t++) {
			getcontext(&w.fib[t]);
			w.fib[t].uc_stack.ss_sp = &w.stacks[(size_t)t * FIBER_STACK];
			w.fib[t].uc_stack.ss_size = FIBER_STACK;
			w.fib[t].uc_link = &w.sched;
			makecontext(&w.fib[t], fiber_entry, 0);
			w.done[t] = 0;
		}
		int alive = n;
		w.in_fiber = true;
		while (alive) {
			int at_barrier = 0, finished = 0;
			for (int k = 0; k < n; k++) {
				int t = g_reverse ? n - 1 - k : k;
				if (w.done[t])
					continue;
				w.cur = t;
				set_thread(t);
				swapcontext(&w.sched, &w.fib[t]);
				if (w.done[t]) {
					alive--;
					finished++;
				} else
					at_barrier++;
			}
			if (at_barrier && finished)
				g_divergent_barriers++;
		}
		w.in_fiber = false;
	}
	int over = 0;
	for (int i = 0; i < GUARD_WORDS; i++)
		if (sharedmem[shm_words + i] != CANARY)
			over = 4 * (i + 1);
	if (over) {
		g_overrun_blocks++;
		int prev = g_overrun_bytes.load();
		while (over > prev && !g_overrun_bytes.compare_exchange_weak(prev, over)) {
		}
		prev = g_overrun_min_bytes.load();
		while (over < prev && !g_overrun_min_bytes.compare_exchange_weak(prev, over)) {
		}
	}
}

// grid x block threads; shm_bytes = the launch's dynamic shared memory; blocks = linear block ids to run (all if
// null); fibers = the kernel has barriers.
static void launch(dim3 grid, dim3 block, int shm_bytes, bool fibers, const std::vector<unsigned> *blocks,
		   const std::function<void()> &k)
{
	gridDim = grid;
	blockDim = block;
	if ((int)(block.x * block.y * block.z) > MAX_BLOCK_THREADS || shm_bytes > 4 * SHM_WORDS) {
		fprintf(stderr, "launch shape out of range\n");
		exit(5);
	}
	int shm_words = (shm_bytes + 3) / 4;
	size_t nb = blocks ? blocks->size() : (size_t)grid.x * grid.y;
	int nw = (int)std::min<size_t>(MAX_WORKERS, std::max<size_t>(1, nb / 16));
	unsigned hc = std::thread::hardware_concurrency();
	if (hc && (int)hc < nw)
		nw = hc;
	std::atomic<size_t> next(0);
	auto body = [&]() {
		Worker *w = new Worker;
		w->kernel = &k;
		tw = w;
		for (size_t i; (i = next++) < nb;)
			run_block(*w, blocks ? (*blocks)[i] : (unsigned)i, shm_words, fibers);
		tw = nullptr;
		delete w;
	};
	std::vector<std::thread> th;
	for (int i = 1; i < nw; i++)
		th.emplace_back(body);
	body();
	for (auto &t : th)
		t.join();
}

// ---------------------------------------------------------------------------------------------------------------
// I/O
struct Arr {
	char type;
	std::vector<char> data;
	size_t n() const { return data.size() / (type == 'b' ? 1 : 4); }
	template <class T> T *p() { return (T *)data.data(); }
};
typedef std::map<std::string, Arr> Arrays;

static Arrays read_io(const char *path)
{
	Arrays m;
	FILE *fp = fopen(path, "rb");
	if (!fp) {
		perror(path);
		exit(3);
	}
	char magic[4];
	uint32_t count;
	if (fread(magic, 1, 4, fp) != 4 || memcmp(magic, "UGRK", 4) || fread(&count, 4, 1, fp) != 1)
		exit(3);
	for (uint32_t c = 0; c < count; c++) {
		uint32_t len;
		uint64_t n;
		Arr a;
		if (fread(&len, 4, 1, fp) != 1 || len > 256)
			exit(3);
		std::string name(len, '\0');
		if (fread(&name[0], 1, len, fp) != len || fread(&a.type, 1, 1, fp) != 1 || fread(&n, 8, 1, fp) != 1)
			exit(3);
		a.data.resize(n * (a.type == 'b' ? 1 : 4));
		if (n && fread(a.data.data(), 1, a.data.size(), fp) != a.data.size())
			exit(3);
		m[name] = a;
	}
	fclose(fp);
	return m;
}

static void write_io(const char *path, Arrays &m)
{
	FILE *fp = fopen(path, "wb");
	if (!fp) {
		perror(path);
		exit(4);
	}
	uint32_t count = m.size();
	fwrite("UGRK", 1, 4, fp);
	fwrite(&count, 4, 1, fp);
	for (auto &kv : m) {
		uint32_t len = kv.first.size();
		uint64_t n = kv.second.n();
		fwrite(&len, 4, 1, fp);
		fwrite(kv.first.data(), 1, len, fp);
		fwrite(&kv.second.type, 1, 1, fp);
		fwrite(&n, 8, 1, fp);
		fwrite(kv.second.data.data(), 1, kv.second.data.size(), fp);
	}
	fclose(fp);
}

static Arrays g_in, g_out;

static Arr &in(const char *name)
{
	auto it = g_in.find(name);
	if (it == g_in.end()) {
		fprintf(stderr, "missing input array %s\n", name);
		exit(6);
	}
	return it->second;
}
static int in_int(const char *name)
{
	return in(name).p<int>()[0];
}
static float in_float(const char *name)
{
	return in(name).p<float>()[0];
}
template <class T> static T *out(const char *name, char type, size_t n, const T *init = nullptr)
{
	Arr &a = g_out[name];
	a.type = type;
	a.data.assign(n * sizeof(T), 0);
	if (init)
		memcpy(a.data.data(), init, n * sizeof(T));
	return a.p<T>();
}
static void out_int(const char *name, long v)
{
	*out<int>(name, 'i', 1) = (int)v;
}

static void set_camcoords(const char *name)
{
	memcpy(dd_camcoords, in(name).p<float>(), sizeof(float) * 64);
}

// optional list of blocks to run (a seeded sample of a large frame); null = all
static std::vector<unsigned> g_blocks;
static const std::vector<unsigned> *blocks_opt()
{
	auto it = g_in.find("blocks");
	if (it == g_in.end())
		return nullptr;
	g_blocks.assign(it->second.p<unsigned>(), it->second.p<unsigned>() + it->second.n());
	return &g_blocks;
}

// runs a barrier kernel forward and reversed on copies of its outputs; keeps the forward result, reports agreement
static void run_both_orders(const std::vector<std::pair<const char *, size_t>> &outs, const std::function<void()> &run)
{
	std::map<std::string, std::vector<char>> init, fwd;
	for (auto &o : outs)
		init[o.first] = g_out[o.first].data;
	g_reverse = false;
	run();
	long overrun_blocks = g_overrun_blocks.load(), divergent = g_divergent_barriers.load();
	for (auto &o : outs) {
		fwd[o.first] = g_out[o.first].data;
		g_out[o.first].data = init[o.first];
	}
	g_reverse = true;
	run();
	g_reverse = false;
	g_overrun_blocks = overrun_blocks; // the reports count the forward run's blocks (barriers: both runs)
	g_divergent_barriers += divergent;
	long differ = 0;
	for (auto &o : outs) {
		std::vector<char> &r = g_out[o.first].data, &f = fwd[o.first];
		for (size_t i = 0; i < r.size(); i += 4)
			differ += memcmp(&r[i], &f[i], std::min<size_t>(4, r.size() - i)) != 0;
		r = f;
	}
	out_int("schedule_differs", differ);
}

// ---------------------------------------------------------------------------------------------------------------
// stages

// DSKernel + DSFillkernel (frustum_grid.h:210-290), NUM_SLABS = 1.  Inputs: cc, faces, verts, nbx, nby, scan
// (the inclusive scan of sizes, an integer primitive: the oracle's).
static void stage_persp()
{
	set_camcoords("cc");
	g_nbx = in_int("nbx");
	g_nby = in_int("nby");
	int F = in("faces").n() / 3;
	int *faces = in("faces").p<int>();
	float *verts = in("verts").p<float>();
	int modelParams[1] = { F };
	unsigned *sizes = out<unsigned>("sizes", 'u', F);
	float *zmin = out<float>("zmin", 'f', F);
	dim3 g((F + NUMTHREADSDS - 1) / NUMTHREADSDS), b(NUMTHREADSDS);
	launch(g, b, 0, false, nullptr, [&] { DSKernel(sizes, zmin, faces, verts, modelParams); });
	Arr &scan = in("scan");
	unsigned R = F ? scan.p<unsigned>()[F - 1] : 0;
	unsigned *keys = out<unsigned>("keys", 'u', R), *vals = out<unsigned>("vals", 'u', R);
	std::vector<unsigned> zs(F, 0);
	launch(g, b, 0, false, nullptr,
	       [&] { DSFillkernel(keys, vals, scan.p<unsigned>(), zs.data(), faces, verts, modelParams); });
}

// DS_spherical_Kernel + DS_spherical_Fillkernel (frustum_grid.h:368-450).  Inputs: cc (light camera), faces, verts,
// nbx, nby (light grid), xM, yM, scan.
static void stage_sph()
{
	set_camcoords("cc");
	g_nbx = in_int("nbx");
	g_nby = in_int("nby");
	float xM = in_float("xM"), yM = in_float("yM");
	int F = in("faces").n() / 3;
	int *faces = in("faces").p<int>();
	float *verts = in("verts").p<float>();
	int modelParams[1] = { F };
	unsigned *sizes = out<unsigned>("sizes", 'u', F);
	float *zmin = out<float>("zmin", 'f', F);
	dim3 g((F + NUMTHREADSDS - 1) / NUMTHREADSDS), b(NUMTHREADSDS);
	launch(g, b, 0, false, nullptr, [&] { DS_spherical_Kernel(sizes, zmin, faces, verts, modelParams, xM, yM); });
	Arr &scan = in("scan");
	unsigned R = F ? scan.p<unsigned>()[F - 1] : 0;
	unsigned *keys = out<unsigned>("keys", 'u', R), *vals = out<unsigned>("vals", 'u', R);
	std::vector<unsigned> zs(F, 0);
	launch(g, b, 0, false, nullptr, [&] {
		DS_spherical_Fillkernel(keys, vals, scan.p<unsigned>(), zs.data(), faces, verts, modelParams, xM, yM);
	});
}

// do_scan_dump, compaction, set_as_zero, create_histogram, exclusive scan (frustum_grid.h:304-362).  Inputs: sorted
// keys, nbx, nby.  The compaction and the scan are CUDPP's integer primitives, written out by their definitions.
static void stage_bounds()
{
	g_nbx = in_int("nbx");
	g_nby = in_int("nby");
	g_slabs = g_in.count("slabs") ? in_int("slabs") : 1;
	Arr &ka = in("keys");
	int R = ka.n();
	unsigned *keys = ka.p<unsigned>();
	unsigned C = (unsigned)g_nbx * g_nby * g_slabs;
	std::vector<unsigned> pos(R + 1), flag(R + 1), compacted(R + 1);
	launch(dim3(R / 256 + 1), dim3(256), 0, false, nullptr,
	       [&] { do_scan_dump(keys, pos.data(), flag.data(), R); });
	int used = 0;
	for (int i = 0; i < R; i++)
		if (flag[i])
			compacted[used++] = pos[i];
	unsigned *span = out<unsigned>("span", 'u', C);
	for (unsigned i = 0; i < C; i++)
		span[i] = 0xdeadbeefu; // set_as_zero has to clear it
	launch(dim3(C / 256 + 1), dim3(256), 0, false, nullptr, [&] { set_as_zero(span); });
	launch(dim3(used / 256 + 1), dim3(256), 0, false, nullptr,
	       [&] { create_histogram(compacted.data(), used, R, keys, span); });
	unsigned *offset = out<unsigned>("offset", 'u', C);
	unsigned acc = 0;
	for (unsigned i = 0; i < C; i++) {
		offset[i] = acc;
		acc += span[i];
	}
	out_int("used", used);
	g_slabs = 1;
}

// rckernel_alpha (frustum_tracer.h:40-52).  Inputs: cc, tex, W, H, vals, span, offset, verts, faces; blocks
// (optional); slabs (optional, NUM_SLABS: span/offset hold (W/8)*(H/8)*slabs cells).  Outputs: normal, t, dir,
// shadowed, id (untouched pixels keep 0 / the "init" value).
static void stage_primary()
{
	set_camcoords("cc");
	g_slabs = g_in.count("slabs") ? in_int("slabs") : 1;
	g_tex = in("tex").p<float>();
	g_strict_texture = g_in.count("strict_texture") ? in_int("strict_texture") : 0;
	g_W = in_int("W");
	g_H = in_int("H");
	g_nbx = g_W / NUM_THREADS_X;
	g_nby = g_H / NUM_THREADS_Y;
	size_t N = (size_t)g_W * g_H;
	unsigned *vals = in("vals").p<unsigned>(), *span = in("span").p<unsigned>(), *offs = in("offset").p<unsigned>();
	float *verts = in("verts").p<float>();
	int *faces = in("faces").p<int>();
	out<float>("normal", 'f', 3 * N);
	out<float>("t", 'f', N);
	out<float>("dir", 'f', 3 * N);
	out<int>("shadowed", 'i', N);
	out<int>("id", 'i', N);
	// trace_kernel.cu:116-119 / frustum_tracer.h: metadata (4 ints), 64 x 9 vertex floats, 64 x 3 normals
	int shm = sizeof(int) * 4 + sizeof(float) * MAX_TRIANGLES * 9 + sizeof(float) * MAX_TRIANGLES * 3;
	const std::vector<unsigned> *blocks = blocks_opt();
	run_both_orders({ { "normal", 0 }, { "t", 0 }, { "dir", 0 }, { "shadowed", 0 }, { "id", 0 } }, [&] {
		float *normal = g_out["normal"].p<float>(), *t = g_out["t"].p<float>(), *dir = g_out["dir"].p<float>();
		int *sh = g_out["shadowed"].p<int>(), *id = g_out["id"].p<int>();
		launch(dim3(g_nbx, g_nby), dim3(NUM_THREADS_X, NUM_THREADS_Y), shm, true, blocks,
		       [&] { rckernel_alpha(vals, span, offs, normal, t, dir, sh, id, verts, faces); });
	});
	out_int("shm_bytes", shm);
	g_slabs = 1;
}

// mapSort_Effective_kernel (per_frame_funcs.h:95-111).  The kernel's NUM_BLOCKS_X/Y are both the image's tiles and
// the light grid's cells, so the light grid here is (W/8, H/8).  Inputs: cc (light camera), t, dir, cam_pos, W, H,
// xM, yM.  Output: d_map (pixel ids, then keys).
static void stage_map()
{
	set_camcoords("cc");
	g_W = in_int("W");
	g_H = in_int("H");
	g_nbx = g_W / NUM_THREADS_X;
	g_nby = g_H / NUM_THREADS_Y;
	float xM = in_float("xM"), yM = in_float("yM");
	size_t N = (size_t)g_W * g_H;
	unsigned *d_map = out<unsigned>("d_map", 'u', 2 * N);
	float *t = in("t").p<float>(), *dir = in("dir").p<float>(), *cam = in("cam_pos").p<float>();
	launch(dim3(g_nbx, g_nby), dim3(NUM_THREADS_X, NUM_THREADS_Y), 0, false, nullptr,
	       [&] { mapSort_Effective_kernel(t, dir, d_map, cam, xM, yM); });
}

// blockScan, segmented inclusive scan, preStreamCompaction, tag_thread, compaction (DecisionData, decision_data.h:
// 180-271).  Input: d_map after the (stable, integer) sort by key; W, H.  Outputs: prefix (chunk starts), nchunks.
static void stage_chunks()
{
	g_W = in_int("W");
	g_H = in_int("H");
	g_nbx = g_W / NUM_THREADS_X;
	g_nby = g_H / NUM_THREADS_Y;
	size_t N = (size_t)g_W * g_H;
	unsigned *d_map = in("d_map").p<unsigned>();
	std::vector<unsigned> valid(N), scratch(N), seg(N), scanArray(N);
	dim3 g(g_nbx, g_nby), b(NUM_THREADS_X, NUM_THREADS_Y);
	launch(g, b, 0, false, nullptr, [&] { blockScan(&d_map[N], valid.data(), scratch.data(), (int)N); });
	for (size_t i = 0; i < N; i++) // CUDPP_SEGMENTED_SCAN, FORWARD | INCLUSIVE: flags start segments
		seg[i] = (i == 0 || valid[i]) ? scratch[i] : seg[i - 1] + scratch[i];
	launch(g, b, 0, false, nullptr, [&] { preStreamCompaction(seg.data(), valid.data(), MAX_RAYS_PER_BLOCK); });
	launch(g, b, 0, false, nullptr, [&] { tag_thread(scanArray.data()); });
	std::vector<unsigned> prefix;
	for (size_t i = 0; i < N; i++) // CUDPP_COMPACT
		if (valid[i])
			prefix.push_back(scanArray[i]);
	out<unsigned>("prefix", 'u', prefix.size(), prefix.data());
	out_int("nchunks", prefix.size());
}

// mod_light_rckernel (per_frame_funcs.h:138-151), launched on (W/8) x (H/8) blocks with size = nchunks.  Inputs:
// cc (light camera), vals, span, offset (light grid, C cells), verts, faces, t, dir, is_shadowed, d_map (sorted),
// prefix, cam_pos, nchunks, W, H; blocks (optional); slabs (optional, NUM_SLABS: C * slabs cells).  Output:
// is_shadowed.
static void stage_shadow()
{
	set_camcoords("cc");
	g_slabs = g_in.count("slabs") ? in_int("slabs") : 1;
	g_W = in_int("W");
	g_H = in_int("H");
	g_nbx = g_W / NUM_THREADS_X;
	g_nby = g_H / NUM_THREADS_Y;
	size_t N = (size_t)g_W * g_H;
	int nchunks = in_int("nchunks");
	Arr &sp = in("span"), &of = in("offset");
	std::vector<unsigned> span(sp.p<unsigned>(), sp.p<unsigned>() + sp.n()), offs(of.p<unsigned>(), of.p<unsigned>() + of.n());
	span.resize(span.size() + g_slabs, 0); // Q11: the sentinel cell, blockcnt[C * NUM_SLABS + p] for p < NUM_SLABS
	offs.resize(offs.size() + g_slabs, 0);
	Arr &pf = in("prefix");
	std::vector<unsigned> prefix(pf.p<unsigned>(), pf.p<unsigned>() + pf.n());
	prefix.resize(std::max<size_t>(prefix.size(), (size_t)g_nbx * g_nby + 1), 0);
	unsigned *vals = in("vals").p<unsigned>(), *d_map = in("d_map").p<unsigned>();
	float *verts = in("verts").p<float>(), *t = in("t").p<float>(), *dir = in("dir").p<float>();
	float *cam = in("cam_pos").p<float>();
	int *faces = in("faces").p<int>();
	out<int>("is_shadowed", 'i', N, in("is_shadowed").p<int>());
	// per_frame_funcs.h:140-141: 7 ints + 64 x 9 floats; the kernel's rayDoneMap lies past that (light_kernel.cu:66)
	int shm = sizeof(int) * 7 + sizeof(float) * MAX_TRIANGLES * 9;
	const std::vector<unsigned> *blocks = blocks_opt();
	run_both_orders({ { "is_shadowed", 0 } }, [&] {
		int *is_shadowed = g_out["is_shadowed"].p<int>();
		launch(dim3(g_nbx, g_nby), dim3(NUM_THREADS_X, NUM_THREADS_Y), shm, true, blocks, [&] {
			mod_light_rckernel(vals, verts, faces, span.data(), offs.data(), t, dir, is_shadowed, d_map,
					   prefix.data(), cam, nchunks);
		});
	});
	out_int("shm_bytes", shm);
	g_slabs = 1;
}

// lambertian_shade then shadow_kernel (shader.h:56-84).  Inputs: cc (the matrices in dd_camcoords at that point: the
// light camera's, Q17), light_pos, normal, t, dir, id, cam_pos, mat_idx, mat_list, is_shadowed, W, H.  Outputs:
// image_unshadowed, mat_ids (lambertian_shade overwrites the ids with material indices), image.
static void stage_shade()
{
	set_camcoords("cc");
	memcpy(dd_light_position, in("light_pos").p<float>(), sizeof(float) * 3);
	g_W = in_int("W");
	g_H = in_int("H");
	g_nbx = g_W / NUM_THREADS_X;
	g_nby = g_H / NUM_THREADS_Y;
	size_t N = (size_t)g_W * g_H;
	Arr &mi = in("mat_idx");
	std::vector<int> mat_idx(mi.n() + 2, -2); // Q17: mat_idx[-2] of a miss
	mat_idx[1] = -1;                          // ... and mat_idx[-1] of an id of -1: a miss keeps its id
	memcpy(&mat_idx[2], mi.p<int>(), sizeof(int) * mi.n());
	Arr &ml = in("mat_list");
	int nmat = ml.n() / MATERIAL_SIZE;
	unsigned char *img = out<unsigned char>("image", 'b', 3 * N);
	int *ids = out<int>("mat_ids", 'i', N, in("id").p<int>());
	float *normal = in("normal").p<float>(), *t = in("t").p<float>(), *dir = in("dir").p<float>();
	float *cam = in("cam_pos").p<float>();
	int *sh = in("is_shadowed").p<int>();
	dim3 g(g_nbx, g_nby), b(NUM_THREADS_X, NUM_THREADS_Y);
	launch(g, b, 0, false, nullptr,
	       [&] { lambertian_shade(img, normal, t, dir, ids, cam, &mat_idx[2], ml.p<float>(), nmat); });
	out<unsigned char>("image_unshadowed", 'b', 3 * N, img);
	img = g_out["image"].p<unsigned char>();
	launch(g, b, 0, false, nullptr, [&] { shadow_kernel(img, sh); });
}

// SlabKernel, then DSFillkernel / DS_spherical_Fillkernel with NUM_SLABS = slabs (frustum_grid.h:241-281 /
// :405-447).  Inputs: zmin (projCoordZ), zMin, zMax (the host's min/max loop), slabs, spherical, and the fill's
// inputs (cc, faces, verts, nbx, nby, scan; xM, yM when spherical).  Outputs: zlist, keys, vals.  zList starts at 0:
// SlabKernel leaves it unwritten for zmin < 0 (Q20).
static void stage_slab()
{
	set_camcoords("cc");
	g_nbx = in_int("nbx");
	g_nby = in_int("nby");
	g_slabs = in_int("slabs");
	int F = in("faces").n() / 3, sph = in_int("spherical");
	int *faces = in("faces").p<int>();
	float *verts = in("verts").p<float>(), *zmin = in("zmin").p<float>();
	float zMin = in_float("zMin"), zMax = in_float("zMax");
	int modelParams[1] = { F };
	unsigned *zlist = out<unsigned>("zlist", 'u', F);
	dim3 g((F + NUMTHREADSDS - 1) / NUMTHREADSDS), b(NUMTHREADSDS);
	launch(g, b, 0, false, nullptr, [&] { SlabKernel(zlist, zmin, modelParams, zMin, zMax); });
	Arr &scan = in("scan");
	unsigned R = F ? scan.p<unsigned>()[F - 1] : 0;
	unsigned *keys = out<unsigned>("keys", 'u', R), *vals = out<unsigned>("vals", 'u', R);
	if (sph) {
		float xM = in_float("xM"), yM = in_float("yM");
		launch(g, b, 0, false, nullptr, [&] {
			DS_spherical_Fillkernel(keys, vals, scan.p<unsigned>(), zlist, faces, verts, modelParams, xM, yM);
		});
	} else
		launch(g, b, 0, false, nullptr,
		       [&] { DSFillkernel(keys, vals, scan.p<unsigned>(), zlist, faces, verts, modelParams); });
	g_slabs = 1;
}

// spot_shade (shader.h:88-112; frames >= 2, Q19).  Inputs as "shade" (no is_shadowed).  Outputs: image, mat_ids,
// dump (the two angles per pixel).
static void stage_spot()
{
	set_camcoords("cc");
	memcpy(dd_light_position, in("light_pos").p<float>(), sizeof(float) * 3);
	g_W = in_int("W");
	g_H = in_int("H");
	g_nbx = g_W / NUM_THREADS_X;
	g_nby = g_H / NUM_THREADS_Y;
	size_t N = (size_t)g_W * g_H;
	Arr &mi = in("mat_idx");
	std::vector<int> mat_idx(mi.n() + 2, -2); // Q17: mat_idx[-2] of a miss
	mat_idx[1] = -1;                          // ... and mat_idx[-1] of an id of -1: a miss keeps its id
	memcpy(&mat_idx[2], mi.p<int>(), sizeof(int) * mi.n());
	Arr &ml = in("mat_list");
	int nmat = ml.n() / MATERIAL_SIZE;
	unsigned char *img = out<unsigned char>("image", 'b', 3 * N);
	int *ids = out<int>("mat_ids", 'i', N, in("id").p<int>());
	float *dump = out<float>("dump", 'f', 2 * N);
	float *normal = in("normal").p<float>(), *t = in("t").p<float>(), *dir = in("dir").p<float>();
	float *cam = in("cam_pos").p<float>();
	launch(dim3(g_nbx, g_nby), dim3(NUM_THREADS_X, NUM_THREADS_Y), 0, false, nullptr,
	       [&] { spot_shade(img, normal, t, dir, ids, cam, &mat_idx[2], ml.p<float>(), nmat, dump); });
}

// perlin_noise_shade (shader.h:115-128).  Inputs: id (primary hit ids), W, H.  Output: image.
static void stage_perlin()
{
	g_W = in_int("W");
	g_H = in_int("H");
	g_nbx = g_W / NUM_THREADS_X;
	g_nby = g_H / NUM_THREADS_Y;
	size_t N = (size_t)g_W * g_H;
	unsigned char *img = out<unsigned char>("image", 'b', 3 * N);
	std::vector<int> ids(in("id").p<int>(), in("id").p<int>() + N);
	std::vector<float> t(N), dir(3 * N), cam(3);
	launch(dim3(g_nbx, g_nby), dim3(NUM_THREADS_X, NUM_THREADS_Y), 0, false, nullptr,
	       [&] { perlin_noise_shade(img, t.data(), dir.data(), cam.data(), ids.data()); });
}

// copy_data_transform (scene.h:120-136).  Inputs: verts, orig, offset, rot.  Output: verts.
static void stage_animate()
{
	Arr &o = in("orig");
	int size = o.n() / 3, offset = in_int("offset");
	float rot = in_float("rot");
	float *v = out<float>("verts", 'f', in("verts").n(), in("verts").p<float>());
	launch(dim3(size / 256 + 1), dim3(256), 0, false, nullptr,
	       [&] { copy_data_transform(v, o.p<float>(), size, offset, rot); });
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "--stamp")) {
		puts(REF_DRIVER_STAMP);
		return 0;
	}
	if (argc < 3) {
		fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
		return 2;
	}
	g_in = read_io(argv[1]);
	Arr &st = in("stage");
	std::string stage(st.data.begin(), st.data.end());
	static const std::map<std::string, void (*)()> stages = {
		{ "persp", stage_persp },   { "sph", stage_sph },       { "bounds", stage_bounds },
		{ "primary", stage_primary }, { "map", stage_map },     { "chunks", stage_chunks },
		{ "shadow", stage_shadow }, { "shade", stage_shade },   { "animate", stage_animate },
		{ "slab", stage_slab },     { "spot", stage_spot },     { "perlin", stage_perlin },
	};
	auto it = stages.find(stage);
	if (it == stages.end()) {
		fprintf(stderr, "unknown stage %s\n", stage.c_str());
		return 2;
	}
	it->second();
	out_int("overrun_blocks", g_overrun_blocks.load());
	out_int("overrun_bytes", g_overrun_bytes.load());
	out_int("overrun_min_bytes", g_overrun_blocks.load() ? g_overrun_min_bytes.load() : 0);
	out_int("divergent_barriers", g_divergent_barriers.load());
	out_int("tex_coord_mismatch", g_tex_coord_mismatch.load());
	out_int("acos_nan", g_acos_nan.load());
	write_io(argv[2], g_out);
	return 0;
}
