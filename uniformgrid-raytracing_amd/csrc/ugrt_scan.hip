// ugrt_scan.hip -- prefix sums of u32 arrays in ONE kernel.
//
// Replaces cudppScan (cudpp/cudpp.h:426-471; call sites frustum_grid.h:249 inclusive over the triangles' cell
// counts, frustum_grid.h:361 exclusive over the cells' spans, decision_data.h:209 the rays' in-run ranks) for the
// eleven scans of a frame.  The library's scan is two launches (it initialises its look-back state in a kernel of
// its own); the arrays here are 16 K - 1 M words, so a scan is bound by its launches, not by its bytes.
// Tiles of 4096 words (16 consecutive words per thread, 16-byte accesses) with a decoupled look-back: tiles are
// taken from a ticket in launch order (a tile only waits for tiles that run or have finished); the state words
// carry the EPOCH of the launch beside their value, so nothing has to be cleared between scans, and the last tile
// to finish resets the ticket.  (One workgroup walking a 16-32 K array by itself - no state at all - was measured
// too: 15-20 us per scan against 5-6, the frame 0.04 ms slower.)
#include "ugrt_scan.h"

static int scan_u32(ugrt_ctx *ctx, const u32 *in, u32 *out, size_t n, bool inclusive)
{
	// 16-byte accesses when both arrays allow them (hipMalloc is 256-B aligned; callers also pass offsets into buffers)
	ScanLoadArray load = { in, ((((uintptr_t)in) | ((uintptr_t)out)) & 15u) == 0 ? 1u : 0u };
	if (inclusive)
		return ugrt_scan_launch<true>(ctx, load, out, n, ScanTailNone());
	return ugrt_scan_launch<false>(ctx, load, out, n, ScanTailNone());
}

int ugrt_prim_inclusive_scan(ugrt_ctx *ctx, const u32 *in, u32 *out, size_t n) { return scan_u32(ctx, in, out, n, true); }
int ugrt_prim_exclusive_scan(ugrt_ctx *ctx, const u32 *in, u32 *out, size_t n) { return scan_u32(ctx, in, out, n, false); }

// the scans as C-ABI calls (ugrt.h): for callers that drive a stage themselves, and for the tests
extern "C" int ugrt_scan(ugrt_ctx *ctx, const unsigned *d_in, unsigned *d_out, size_t n, int inclusive)
{
	if (!ctx || (n && (!d_in || !d_out)))
		return ugrt_fail(UGRT_EINVAL, "scan: null argument");
	if (n && d_in == d_out)
		return ugrt_fail(UGRT_EINVAL, "scan: the output aliases the input");
	UGRT_HIP(hipSetDevice(ctx->device));
	return scan_u32(ctx, d_in, d_out, n, inclusive != 0);
}

extern "C" int ugrt_scan_pair(ugrt_ctx *ctx, const unsigned *d_in_a, unsigned *d_out_a, const unsigned *d_in_b,
			      unsigned *d_out_b, size_t n, int inclusive)
{
	if (!ctx || (n && (!d_in_a || !d_out_a || !d_in_b || !d_out_b)))
		return ugrt_fail(UGRT_EINVAL, "scan_pair: null argument");
	if (n && (d_in_a == d_out_a || d_in_b == d_out_b || d_out_a == d_out_b || d_in_a == d_out_b || d_in_b == d_out_a))
		return ugrt_fail(UGRT_EINVAL, "scan_pair: an output aliases another array of the call");
	UGRT_HIP(hipSetDevice(ctx->device));
	// (16-byte loads per input; the launch decides on 16-byte stores from both outputs)
	const ScanLoadArray load_a = { d_in_a, (((uintptr_t)d_in_a) & 15u) == 0 ? 1u : 0u };
	const ScanLoadArray load_b = { d_in_b, (((uintptr_t)d_in_b) & 15u) == 0 ? 1u : 0u };
	if (inclusive)
		return ugrt_scan_launch_pair<true>(ctx, load_a, d_out_a, load_b, d_out_b, n);
	return ugrt_scan_launch_pair<false>(ctx, load_a, d_out_a, load_b, d_out_b, n);
}
