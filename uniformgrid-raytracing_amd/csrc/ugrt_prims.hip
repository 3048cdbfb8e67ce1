// ugrt_prims.hip -- the data-parallel primitives of the grid build, on rocPRIM.
//
// Replaces the reference's CUDPP 1.1 call sites (cudpp/cudpp.h:426-471):
//   cudppScan inclusive/exclusive  frustum_grid.h:249,361  -> ugrt_scan.hip (own single-kernel scan)
//   cudppSort key-value radix      frustum_grid.h:298, decision_data.h:177
//                                  -> rocprim::radix_sort_pairs (stable LSD radix sort)
// The reference sorts all 32 key bits although keys < number of cells
// (frustum_grid.h:298); here only ceil(log2(cells)) bits are sorted, which
// gives the same permutation in half the passes.
#include <cstring> // must precede rocprim on ROCm 7.2

#include <rocprim/rocprim.hpp>

#include "ugrt_ctx.h"

// (the prefix sums live in ugrt_scan.hip)

int ugrt_prim_sort_pairs(ugrt_ctx *ctx, const u32 *kin, u32 *kout, const u32 *vin, u32 *vout, size_t n,
			 int end_bit, const u32 *n_dev)
{
	if (!n_dev && (ctx->opt[UGRT_OPT_SORT_LIBRARY] == 1 || n > ((size_t)1 << 30)))
		return ugrt_prim_sort_pairs_rocprim(ctx, kin, kout, vin, vout, n, end_bit);
	return ugrt_sort_pairs_u32(ctx, kin, kout, vin, vout, n, end_bit, n_dev);
}

int ugrt_prim_sort_pairs_rocprim(ugrt_ctx *ctx, const u32 *kin, u32 *kout, const u32 *vin, u32 *vout, size_t n,
				 int end_bit)
{
	if (n == 0)
		return UGRT_OK;
	if (end_bit < 1)
		end_bit = 1;
	if (end_bit > 32)
		end_bit = 32;
	size_t bytes = 0;
	UGRT_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit,
					   ctx->stream));
	int rc = ugrt_buf_reserve(ctx, ctx->temp, bytes);
	if (rc)
		return rc;
	UGRT_HIP(rocprim::radix_sort_pairs(ctx->temp.p, bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit,
					   ctx->stream));
	return UGRT_OK;
}

// 64-bit keys: the shadow tracer's private re-grouping of rays (light cell, direction Morton code)
int ugrt_prim_sort_pairs64(ugrt_ctx *ctx, const u64 *kin, u64 *kout, const u32 *vin, u32 *vout, size_t n,
			   int end_bit)
{
	if (n == 0)
		return UGRT_OK;
	if (end_bit < 1)
		end_bit = 1;
	if (end_bit > 64)
		end_bit = 64;
	size_t bytes = 0;
	UGRT_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit,
					   ctx->stream));
	int rc = ugrt_buf_reserve(ctx, ctx->temp, bytes);
	if (rc)
		return rc;
	UGRT_HIP(rocprim::radix_sort_pairs(ctx->temp.p, bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit,
					   ctx->stream));
	return UGRT_OK;
}

extern "C" int ugrt_sort_pairs(ugrt_ctx *ctx, const unsigned *d_keys_in, unsigned *d_keys_out,
			       const unsigned *d_values_in, unsigned *d_values_out, size_t n, int key_bits,
			       int use_library)
{
	if (!ctx || (n && (!d_keys_in || !d_keys_out || !d_values_in || !d_values_out)))
		return ugrt_fail(UGRT_EINVAL, "sort_pairs: null argument");
	if (key_bits < 1 || key_bits > 32)
		return ugrt_fail(UGRT_EINVAL, "sort_pairs: key_bits %d outside [1,32]", key_bits);
	if (n && (d_keys_in == d_keys_out || d_values_in == d_values_out))
		return ugrt_fail(UGRT_EINVAL, "sort_pairs: outputs alias inputs");
	UGRT_HIP(hipSetDevice(ctx->device));
	if (use_library)
		return ugrt_prim_sort_pairs_rocprim(ctx, d_keys_in, d_keys_out, d_values_in, d_values_out, n, key_bits);
	return ugrt_prim_sort_pairs(ctx, d_keys_in, d_keys_out, d_values_in, d_values_out, n, key_bits);
}

// ugrt_sort_pairs_batch as a C-ABI call: two lists per launch, device counts, in place (ugrt.h)
extern "C" int ugrt_sort_pairs_lists(ugrt_ctx *ctx, int nlists, const unsigned *const *d_keys_in, unsigned *const *d_keys_out,
				     const unsigned *const *d_values_in, unsigned *const *d_values_out, const size_t *n,
				     const int *key_bits, const unsigned *const *d_counts)
{
	if (!ctx)
		return ugrt_fail(UGRT_EINVAL, "sort_pairs_lists: null argument");
	if (nlists < 1 || nlists > 2)
		return ugrt_fail(UGRT_EINVAL, "sort_pairs_lists: %d lists (1..2)", nlists);
	if (!d_keys_in || !d_keys_out || !d_values_in || !d_values_out || !n || !key_bits)
		return ugrt_fail(UGRT_EINVAL, "sort_pairs_lists: null argument");
	RsJob jobs[2];
	const void *arr[2][4];
	for (int j = 0; j < nlists; j++) {
		if (key_bits[j] < 1 || key_bits[j] > 32)
			return ugrt_fail(UGRT_EINVAL, "sort_pairs_lists: key_bits %d of list %d outside [1,32]", key_bits[j], j);
		jobs[j] = { d_keys_in[j], d_values_in[j], d_keys_out[j], d_values_out[j], n[j], key_bits[j], d_counts ? d_counts[j] : nullptr };
		arr[j][0] = d_keys_in[j], arr[j][1] = d_values_in[j], arr[j][2] = d_keys_out[j], arr[j][3] = d_values_out[j];
		if (!n[j])
			continue;
		if (!d_keys_in[j] || !d_keys_out[j] || !d_values_in[j] || !d_values_out[j])
			return ugrt_fail(UGRT_EINVAL, "sort_pairs_lists: null argument (list %d)", j);
		const bool kalias = d_keys_in[j] == d_keys_out[j], valias = d_values_in[j] == d_values_out[j];
		if (kalias != valias)
			return ugrt_fail(UGRT_EINVAL, "sort_pairs_lists: list %d aliases only one of its two arrays", j);
		// in place: an even number of passes reads the input in the first pass only, which writes the sort's own buffers
		if (kalias && ((key_bits[j] + 7) / 8) % 2 != 0)
			return ugrt_fail(UGRT_EINVAL, "sort_pairs_lists: list %d in place needs 2 or 4 passes, %d key bits take %d", j,
					 key_bits[j], (key_bits[j] + 7) / 8);
	}
	// an output may be no other array of the call (but its own input, checked above)
	for (int j = 0; j < nlists; j++)
		for (int o = 2; o < 4 && n[j]; o++)
			for (int k = 0; k < nlists; k++)
				for (int a = 0; a < 4 && n[k]; a++) {
					const bool self = k == j && (a == o || a == o - 2);
					if (!self && arr[j][o] == arr[k][a])
						return ugrt_fail(UGRT_EINVAL, "sort_pairs_lists: an output of list %d is another array of the call", j);
				}
	UGRT_HIP(hipSetDevice(ctx->device));
	return ugrt_sort_pairs_batch(ctx, jobs, nlists);
}
