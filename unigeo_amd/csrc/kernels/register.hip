// 7-Scenes depth registration on the device: the Kinect depth image warped into the colour camera, which the reference does
// once, offline, with a Python loop over every pixel (dataset/sevenScenes/preprocess.py:82-140).  A forward splat with a z-buffer: every source
// pixel is back-projected, moved by a rigid transform, projected and rounded to a target pixel, and the target keeps the smallest depth that
// reaches it.  The minimum is taken with ONE integer atomicMin per source pixel on an order-preserving key of the float32 depth, so the result
// does not depend on the order in which the threads arrive: no floating-point atomic, no lock, equal bytes from run to run.
// Every double step below is one IEEE operation, in the order include/unigeo_hip.h documents, which is the order harness/rgbd.py's
// register_depth evaluates on the host.  The pragma below is what keeps a product and a sum from being contracted into an FMA: the __d*_rn
// functions of this toolchain's headers are plain operators compiled with contraction allowed, so they would not.  A check on the compiled
// k_reg_splat: it holds the definition's 15 v_add_f64 (a contraction would remove one) and 19 v_mul_f64 (13 of the definition, one inside each
// of the four divisions, W / 2 and H / 2); its v_fma_f64 all belong to the division sequences.
// Addresses: a source pixel reads depth[i] with i < n; its target index is t * H * W + yi * W + xi with 0 <= yi < H and 0 <= xi < W tested
// in the positive form (a NaN fails it and is dropped), so it stays inside frame t of the z-buffer.
#include "../common.h"
#include "zkey.h"      // reg_key / reg_unkey: the order-preserving key of a float32, shared with render.hip

#pragma clang fp contract(off)

#define RB 256       // threads per block
#define RMAXB 2048   // grid cap; the loops below stride over the rest

__global__ __launch_bounds__(RB) void k_reg_fill(unsigned* __restrict__ zbuf, long n, float init) {
  const unsigned k = reg_key(init);
  for (long i = (long)blockIdx.x * RB + threadIdx.x; i < n; i += (long)gridDim.x * RB) zbuf[i] = k;
}

// One thread per source pixel of the chunk (n = T * H * W).  A wave reads 128 contiguous bytes of depth; its 64 atomics land on neighbouring
// words of one or two target rows (the warp is close to a shift), a handful of them on the same word where the colour camera's shorter focal
// folds two sources onto one target.
__global__ __launch_bounds__(RB) void k_reg_splat(const unsigned short* __restrict__ depth, unsigned* __restrict__ zbuf, long n, int H, int W,
                                                  const RegArgs a) {
  const long plane = (long)H * W;
  const double hw = 0.5 * (double)W, hh = 0.5 * (double)H;          // W / 2 and H / 2: exact
  for (long i = (long)blockIdx.x * RB + threadIdx.x; i < n; i += (long)gridDim.x * RB) {
    const unsigned short raw = depth[i];
    const float d32 = __fdiv_rn((float)raw, a.divisor);
    if (!(d32 > 0.f && d32 < a.max_valid)) continue;
    if (a.drop_sentinel && raw == 65535) continue;
    const long t = i / plane;
    const long rem = i - t * plane;
    const int row = (int)(rem / W), col = (int)(rem - (long)row * W);
    const double d = (double)d32;
    const double X = (((0.5 + (double)col) - hw) / a.src_focal) * d;
    const double Y = (((0.5 + (double)row) - hh) / a.src_focal) * d;
    const double* m = a.m;
    const double x3 = ((m[0] * X + m[1] * Y) + m[2] * d) + m[3];
    const double y3 = ((m[4] * X + m[5] * Y) + m[6] * d) + m[7];
    const double z3 = ((m[8] * X + m[9] * Y) + m[10] * d) + m[11];
    const double xi = rint(((x3 / z3) * a.dst_focal) + hw);       // ties to even
    const double yi = rint(((y3 / z3) * a.dst_focal) + hh);
    if (!(xi >= 0.0 && yi >= 0.0 && yi < (double)H && xi < (double)W)) continue;            // compared as doubles; NaN is dropped
    atomicMin(&zbuf[t * plane + (long)(int)yi * W + (int)xi], reg_key(__double2float_rn(z3)));
  }
}

// zbuf > 1000 -> 0; v = fl32(1000 * zbuf); out = the low 16 bits of int32(trunc(v)); a v outside int32 (custom options only) gives 0
__global__ __launch_bounds__(RB) void k_reg_finalize(const unsigned* __restrict__ zbuf, unsigned short* __restrict__ out, long n) {
  for (long i = (long)blockIdx.x * RB + threadIdx.x; i < n; i += (long)gridDim.x * RB) {
    float z = reg_unkey(zbuf[i]);
    if (z > 1000.f) z = 0.f;
    const float v = __fmul_rn(1000.f, z);
    out[i] = (v > -2147483648.f && v < 2147483648.f) ? (unsigned short)((unsigned)(int)v & 0xffffu) : (unsigned short)0;
  }
}

static int reg_blocks(long n) { long b = (n + RB - 1) / RB; return (int)(b > RMAXB ? RMAXB : (b < 1 ? 1 : b)); }

// depth: [T,H,W] uint16; zbuf: T*H*W words of scratch; out: [T,H,W] uint16.  All three on the device, T * H * W < 2^31.
void launch_register_depth(const unsigned short* depth, int T, int H, int W, const RegArgs& a, unsigned* zbuf, unsigned short* out, hipStream_t s) {
  const long n = (long)T * H * W;
  const int nb = reg_blocks(n);
  hipLaunchKernelGGL(k_reg_fill, dim3(nb), dim3(RB), 0, s, zbuf, n, 2000.f);
  hipLaunchKernelGGL(k_reg_splat, dim3(nb), dim3(RB), 0, s, depth, zbuf, n, H, W, a);
  hipLaunchKernelGGL(k_reg_finalize, dim3(nb), dim3(RB), 0, s, (const unsigned*)zbuf, out, n);
}
