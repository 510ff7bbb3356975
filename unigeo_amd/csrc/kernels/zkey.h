// The order-preserving integer key of a float32 that the z-buffers of kernels/register.hip and kernels/render.hip take their integer
// atomicMin on: one copy for both.
#pragma once
#include <hip/hip_runtime.h>

// float32 -> uint32 whose unsigned order is the float order (-inf < ... < -0 < +0 < ... < +inf); NaN never reaches it
__device__ __forceinline__ unsigned reg_key(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float reg_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
