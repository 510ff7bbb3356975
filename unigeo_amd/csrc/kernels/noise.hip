// Clip inputs made on the device: the counter-based normal generator behind the seeded noise mode
// (Philox4x32-10 + Box-Muller) and the uint8 planar -> float32 channels-last frame conversion.  Streaming kernels, no LDS:
// one thread makes four elements / four pixels and writes them with 16-byte stores.
//
// Generator, as restated by tests/noise_oracle.py: key = the 64-bit seed (lo, hi); counter = (q lo, q hi, stream, 0) with q = e >> 2
// for the linear element index e of the tensor in its own layout; the four output words of block q make elements 4q .. 4q + 3:
//   u(x) = ((x >> 9) + 0.5) * 2^-23 in (0, 1),  r = sqrt(-2 ln u(x0)),  (4q, 4q+1) = r (cos, sin)(2 pi u(x1));  (4q+2, 4q+3) from (x2, x3).
// An element depends on (seed, stream, e) only: not on the launch geometry, the context or what ran before.
#include "../common.h"

namespace {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(kPhiloxM0, c.x), l0 = kPhiloxM0 * c.x;
    const uint32_t h1 = __umulhi(kPhiloxM1, c.z), l1 = kPhiloxM1 * c.z;
    c = make_uint4(h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0);
    k0 += kPhiloxW0; k1 += kPhiloxW1;
  }
  return c;
}

__device__ __forceinline__ uint4 philox_block(unsigned long long q, uint32_t stream, unsigned long long seed) {
  return philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), stream, 0u), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// exact in float32: (x >> 9) < 2^23, + 0.5 needs 24 bits, the scale is a power of two
__device__ __forceinline__ float unit_open(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// accurate logf / sincospif (not the fast intrinsics); sincospif(2u) takes the exact argument 2u, so 2 pi u is never rounded
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(unit_open(xa)));
  float sn, cs;
  sincospif(2.0f * unit_open(xb), &sn, &cs);
  z0 = r * cs; z1 = r * sn;
}

}  // namespace

#define GS_LOOP(i, n) for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)
static inline dim3 gs_grid(long n, int block = 256) {
  long g = (n + block - 1) / block;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return dim3((unsigned)g);
}

// raw words of blocks q0 .. q0 + nblocks - 1 (test entry point: the generator against the published known answers)
__global__ void k_philox_u32(uint32_t* out, long nblocks, unsigned long long seed, uint32_t stream, unsigned long long q0) {
  GS_LOOP(b, nblocks) *(uint4*)(out + b * 4) = philox_block(q0 + (unsigned long long)b, stream, seed);
}
void launch_philox_u32(uint32_t* out, long nblocks, uint64_t seed, uint32_t stream, uint64_t q0, hipStream_t s) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(k_philox_u32, gs_grid(nblocks), dim3(256), 0, s, out, nblocks, (unsigned long long)seed, stream, (unsigned long long)q0);
}

// out[i] = element e0 + i of the stream, i in [0, n).  Thread b makes block (e0 >> 2) + b; a block that lies inside [0, n) with
// e0 % 4 == 0 (the pipeline's tensors: always) is one 16-byte store, the head / tail blocks of an odd offset or n % 4 != 0 are
// written element by element, inside [0, n) only.
__global__ void k_randn(float* out, long n, unsigned long long seed, uint32_t stream, unsigned long long e0) {
  const int lead = (int)(e0 & 3);
  const long nblocks = (n + lead + 3) >> 2;
  GS_LOOP(b, nblocks) {
    const uint4 x = philox_block((e0 >> 2) + (unsigned long long)b, stream, seed);
    float4 z;
    box_muller(x.x, x.y, z.x, z.y);
    box_muller(x.z, x.w, z.z, z.w);
    const long i0 = b * 4 - lead;      // index in out of the block's first element
    if (lead == 0 && i0 + 4 <= n) {
      *(float4*)(out + i0) = z;
    } else {
      const float v[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j >= 0 && i0 + j < n) out[i0 + j] = v[j];
    }
  }
}
void launch_randn(float* out, long n, uint64_t seed, uint32_t stream, uint64_t e0, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_randn, gs_grid((n + (long)(e0 & 3) + 3) >> 2), dim3(256), 0, s, out, n, (unsigned long long)seed, stream,
                     (unsigned long long)e0);
}

// frames [T,3,H,W] uint8 (planar, what np.stack(data["images"]) is) -> [T,H,W,3] float32 = x / 255 (correctly rounded float32
// division: bit-identical to prepare_input's x.astype(float32) / 255.0).  HW % 4 == 0; a thread reads 4 bytes of each plane and writes
// 48 contiguous bytes.
__global__ void k_u8_to_frames(const unsigned char* in, float* out, long T, long HW) {
  const long q = HW >> 2, n = T * q;
  GS_LOOP(g, n) {
    const long t = g / q, p = (g - t * q) << 2;
    const unsigned char* src = in + t * 3 * HW + p;
    const uchar4 r = *(const uchar4*)src, gg = *(const uchar4*)(src + HW), b = *(const uchar4*)(src + 2 * HW);
    float4* dst = (float4*)(out + (t * HW + p) * 3);
    dst[0] = make_float4((float)r.x / 255.0f, (float)gg.x / 255.0f, (float)b.x / 255.0f, (float)r.y / 255.0f);
    dst[1] = make_float4((float)gg.y / 255.0f, (float)b.y / 255.0f, (float)r.z / 255.0f, (float)gg.z / 255.0f);
    dst[2] = make_float4((float)b.z / 255.0f, (float)r.w / 255.0f, (float)gg.w / 255.0f, (float)b.w / 255.0f);
  }
}
void launch_u8_to_frames(const unsigned char* in, float* out, int T, long HW, hipStream_t s) {
  hipLaunchKernelGGL(k_u8_to_frames, gs_grid((long)T * (HW >> 2)), dim3(256), 0, s, in, out, (long)T, HW);
}
