// ugrt_selftest.hip -- device self-tests of the arithmetic and cross-lane helpers the tracers rely on (ugrt_dev.h,
// ugrt_packet.h): each kernel counts mismatches against the plain form.  ugrt_context.hip runs them and keeps the counts.
#include "ugrt_packet.h"

// Every float bit pattern through d_recip_det against the division it stands for (ugrt_dev.h); *mismatches = operands whose
// reciprocal differs by a bit.  ugrt_ctx_get_state "recip_mismatches".
__global__ __launch_bounds__(256) void k_recip_selftest(unsigned long long *bad)
{
	unsigned long long mine = 0;
	const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
	for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
		const float x = __uint_as_float((u32)i);
		if (x > -D_EPSILON && x < D_EPSILON) // the tests return before they divide
			continue;
		const float want = 1.0f / x, got = d_recip_det(x);
		const bool same = __float_as_uint(want) == __float_as_uint(got) || (want != want && got != got);
		mine += same ? 0u : 1u;
	}
	if (mine)
		atomicAdd(bad, mine);
}

// The cross-lane reductions of ugrt_packet.h (DPP controls, v_permlane16_swap / v_permlane32_swap) against the same
// reductions by __shfl_xor, on pseudo-random values; *mismatches = lanes that differ.  ugrt_ctx_get_state "lane_reduce_mismatches".
__global__ __launch_bounds__(64) void k_lane_reduce_selftest(unsigned long long *bad)
{
	const int lane = threadIdx.x;
	u32 mine = 0;
	for (u32 round = 0; round < 64u; round++) {
		u32 x = (blockIdx.x * 64u + (u32)lane) * 2654435761u + round * 40503u;
		x ^= x >> 15;
		x *= 2246822519u;
		x ^= x >> 13;
		const int v = (int)x;
		// inside the quadrants: lane bits 0, 1, 3, 4
		int lo = v, hi = v;
		for (int m = 1; m <= 16; m <<= 1) {
			if (m == 4)
				continue;
			const int ol = __shfl_xor(lo, m), oh = __shfl_xor(hi, m);
			lo = ol < lo ? ol : lo;
			hi = oh > hi ? oh : hi;
		}
		const int qlo = d_quadrant_reduce<DOpMin>(v), qhi = d_quadrant_reduce<DOpMax>(v);
		mine += (qlo != lo) + (qhi != hi);
		// across them: bits 2 and 5
		int alo = lo, ahi = hi;
		for (int m = 4; m <= 32; m <<= 3) {
			const int ol = __shfl_xor(alo, m), oh = __shfl_xor(ahi, m);
			alo = ol < alo ? ol : alo;
			ahi = oh > ahi ? oh : ahi;
		}
		mine += (d_across_quadrants<DOpMin>(qlo) != alo) + (d_across_quadrants<DOpMax>(qhi) != ahi);
		// the whole wave, floats (a quarter of the lanes do not contribute)
		const float f = __int_as_float((v & 0x3FFFFFFF) | 0x20000000) * ((v & 4) ? -1.0f : 1.0f);
		const bool in = (v & 3) != 0;
		float wlo = in ? f : __builtin_huge_valf(), whi = in ? f : -__builtin_huge_valf();
		for (int m = 32; m >= 1; m >>= 1) {
			wlo = fminf(wlo, __shfl_xor(wlo, m));
			whi = fmaxf(whi, __shfl_xor(whi, m));
		}
		mine += (d_wave_fmin(in ? f : __builtin_huge_valf()) != wlo) + (d_wave_fmax(in ? f : -__builtin_huge_valf()) != whi);
	}
	if (mine)
		atomicAdd(bad, (unsigned long long)mine);
}

// Every float bit pattern through the device forms of ugrt_f2i / ugrt_f2u / ugrt_floor2i (one or two instructions) against
// the portable forms of include/ugrt_fmath.h; *mismatches = operands that differ in any of the three.
// ugrt_ctx_get_state "f2i_mismatches".
__global__ __launch_bounds__(256) void k_f2i_selftest(unsigned long long *bad)
{
	unsigned long long mine = 0;
	const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
	for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
		const float x = __uint_as_float((u32)i);
		const bool same = ugrt_f2i(x) == ugrt_f2i_portable(x) && ugrt_f2u(x) == ugrt_f2u_portable(x) &&
				  ugrt_floor2i(x) == ugrt_floor2i_portable(x);
		mine += same ? 0u : 1u;
	}
	if (mine)
		atomicAdd(bad, mine);
}

// one counter on the device: cleared, filled by `kernel`, copied to *mismatches; waits for the stream
static int selftest_run(ugrt_ctx *ctx, void (*kernel)(unsigned long long *), unsigned grid, unsigned block, unsigned long long *mismatches)
{
	UGRT_HIP(hipSetDevice(ctx->device));
	unsigned long long *d = nullptr;
	UGRT_HIP(hipMalloc((void **)&d, sizeof *d));
	hipError_t e = hipMemsetAsync(d, 0, sizeof *d, ctx->stream);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, ctx->stream, d);
		e = hipMemcpyAsync(mismatches, d, sizeof *d, hipMemcpyDeviceToHost, ctx->stream);
	}
	if (e == hipSuccess)
		e = hipStreamSynchronize(ctx->stream);
	(void)hipFree(d);
	UGRT_HIP(e);
	return UGRT_OK;
}

int ugrt_recip_selftest(ugrt_ctx *ctx, unsigned long long *mismatches) { return selftest_run(ctx, k_recip_selftest, 4096, 256, mismatches); }
int ugrt_lane_reduce_selftest(ugrt_ctx *ctx, unsigned long long *mismatches) { return selftest_run(ctx, k_lane_reduce_selftest, 1024, 64, mismatches); }
int ugrt_f2i_selftest(ugrt_ctx *ctx, unsigned long long *mismatches) { return selftest_run(ctx, k_f2i_selftest, 4096, 256, mismatches); }
