// ref_shim.h -- test infrastructure: what the reference's CUDA kernel files need to compile as host C++.
//
// oracle/ref_kernels.cpp includes this header, then the reference's main.cu.h and *_kernel.cu files as they lie
// (oracle/Makefile target "ref").  Nothing here is linked into the product.
//
// * __device__ / __global__ / __constant__ are defined away; __shared__ becomes thread_local: the blocks of a launch
//   are spread over worker threads, a block runs on one thread, so one thread_local array is one block's shared
//   memory (ref_kernels.cpp sizes it, zeroes it and guards it with a canary zone).
// * threadIdx / blockIdx are per worker thread and are switched with the fiber that runs; blockDim / gridDim are the
//   launch's.
// * __syncthreads() is a real barrier for the kernels run as fibers (ref_kernels.cpp), a no-op otherwise.
// * Platform arithmetic that DESIGN section 3 fixes in include/ugrt_fmath.h goes through that header: acosf (and
//   acos of a float, which the device compiler maps to acosf) is ugrt_acosf, and floor() -> int is ugrt_floorf
//   followed by ugrt_f2i (truncate, NaN -> 0, saturate: what CUDA does, where x86 would give INT_MIN).
//   A plain (int) cast in the kernel text cannot be redirected; see ref_kernels.cpp for where that applies.
// * sqrt / sinf / cosf are host libm.  sqrt of a float is correctly rounded either way; sinf/cosf appear only in
//   copy_data_transform, whose product equivalent evaluates them with host libm as well (ugrt_rot_cos_sin).
// * tex2D: see ref_kernels.cpp (the texture fetch is pinned by definition, not by the reference).
#ifndef UGRT_REF_SHIM_H
#define UGRT_REF_SHIM_H

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ugrt_fmath.h"

#define __device__
#define __global__
#define __constant__
#define __shared__ thread_local

struct ref_uint3 {
	unsigned int x, y, z;
};
struct dim3 {
	unsigned int x, y, z;
	dim3(unsigned int a = 1, unsigned int b = 1, unsigned int c = 1) : x(a), y(b), z(c) {}
};
extern thread_local ref_uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;

void __syncthreads();

struct float4 {
	float x, y, z, w;
};
typedef unsigned int GLuint;
struct cudaArray;
enum cudaTextureReadMode { cudaReadModeElementType };
template <class T, int dim, cudaTextureReadMode mode> struct texture {
};
float4 ref_tex2D(float x, float y);
template <class T, int dim, cudaTextureReadMode mode> static inline float4 tex2D(texture<T, dim, mode> &, float x, float y)
{
	return ref_tex2D(x, y);
}

// floor() whose conversion to int is the ABI's (ugrt_floor2i); the kernels only ever store it to an int
struct ref_floored {
	float v;
	operator int() const { return ugrt_f2i(v); }
};
static inline ref_floored ref_floor(float x)
{
	ref_floored r = { ugrt_floorf(x) };
	return r;
}
// acos of |x| > 1 is NaN, and the kernels cast the angle to int: counted, since x86 and CUDA differ there
float ref_acosf(float x);
#define floor(x) ref_floor(x)
#define acosf(x) ref_acosf(x)
#define acos(x) ref_acosf(x)

#endif
