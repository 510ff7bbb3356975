// Temporal alignment error of a video depth on the device (the numpy mirror is harness/temporal.py).  UNPINNED: the
// reference has no such metric; it is restated from the published definition (ChronoDepth, Video Depth Anything).  Every frame's aligned
// depth is carried into its neighbour's camera and compared there with the neighbour's own aligned depth.  P = 2 * (T - stride) directed
// pairs: pair 2i carries frame a = i into b = i + stride, pair 2i + 1 carries a = i + stride into b = i.
//
// Aligned depth d of a pixel (tae_depth), float32, every operation rounded on its own, from the ORIGINAL prediction: a = fl(fl(s * pred) + t);
// with the disparity flag a = c where a < c (c = NaN: no floor), d = 1 / a where a > 0, else 0; then d = lo where d < lo, d = hi where d > hi
// (the post-clip bounds, -inf / +inf when off; a NaN d stays NaN and takes no part).
//
// k_tae_splat, one thread per source pixel per pair, i = p * H * W + row * W + col < n = P * H * W: it reads pred[a * H * W + row * W + col]
// with a < T (i / (H * W) = p < P, so p / 2 < T - stride), the 9 floats of K_a and K_b and the 12 doubles of M_p = (inv(C_b) C_a)[:3], a table
// the host builds (harness/temporal.py relative_poses).  With d > 0 and finite, in float64, one IEEE operation per step, contraction off:
//   D = d;  X = ((col - cx_a) * D) / fx_a;  Y = ((row - cy_a) * D) / fy_a;  x3 = ((m0 * X + m1 * Y) + m2 * D) + m3, likewise y3, z3;
//   u = rint(((x3 / z3) * fx_b) + cx_b), v likewise (ties to even);  z = float32(z3)
// The pixel is kept when z3 > 0, z > 0, z finite, u >= 0, v >= 0, v < H and u < W, all tested in the positive form as doubles: a NaN anywhere
// fails a test and drops the pixel, so the target index p * H * W + v * W + u stays inside plane p of the z-buffer (n words).  The target keeps the
// smallest z: ONE integer atomicMin per kept source pixel on reg_key(z).  A minimum does not depend on the order of arrival, so the bytes do
// not depend on thread order; no floating-point atomic, no lock.  k_tae_fill sets every word to TAE_EMPTY = 0xffffffff, which is above the key
// of every finite positive float32 (at most 0xff7fffff), so "reached" is key != TAE_EMPTY.
//
// k_tae_score, grid (blocks, pairs): block (bx, y) walks the target pixels q = bx * EVAL_NT + tid + j * gridDim.x * EVAL_NT < H * W of pair
// p = p0 + y < P; it reads zbuf[p * H * W + q], pred / gt / mask at b * H * W + q with b < T, and writes warp_out / err_out at p * H * W + q < n.
// A reached pixel with d_b > 0, gt_b > 0, !(gt_b >= max_depth) and the custom mask is scored: e = fl(|z - d_b|) / d_b in float32.  The block's
// sum of double(e) and its count go through eval_block_reduce (kernels/eval_reduce.h) to part[(p * gridDim.x + bx) * 2 + {0, 1}] with vector
// stores; the host adds a pair's partials in block order.  Nothing here depends on the order in which blocks or threads run.
#include "../common.h"
#include "eval_reduce.h"
#include "zkey.h"

#pragma clang fp contract(off)

#define TB 256          // threads per block of the fill and splat kernels
#define TMAXB 2048      // their grid cap; the loops stride over the rest
#define TAE_EMPTY 0xffffffffu

__device__ __forceinline__ float tae_depth(float pred, const TaeArgs& a) {
  const float m = a.s * pred;
  float d = m + a.t;
  if (a.disparity) {
    if (d < a.floor_) d = a.floor_;
    d = d > 0.f ? 1.0f / d : 0.f;
  }
  if (d < a.plo) d = a.plo;
  if (d > a.phi) d = a.phi;
  return d;
}
// pair p -> its source frame a and target frame b
__device__ __forceinline__ void tae_pair(long p, int stride, long& a, long& b) {
  const long i = p >> 1;
  if (p & 1) { a = i + stride; b = i; } else { a = i; b = i + stride; }
}

__global__ __launch_bounds__(TB) void k_tae_fill(unsigned* __restrict__ zbuf, long n) {
  for (long i = (long)blockIdx.x * TB + threadIdx.x; i < n; i += (long)gridDim.x * TB) zbuf[i] = TAE_EMPTY;
}

// A wave reads 256 contiguous bytes of one source row; its 64 atomics land on neighbouring words of one or two target rows (between
// consecutive frames the warp is close to a shift), several on one word only where the motion folds sources together.
__global__ __launch_bounds__(TB) void k_tae_splat(const float* __restrict__ pred, const float* __restrict__ K, const double* __restrict__ rel,
                                                  unsigned* __restrict__ zbuf, long n, int H, int W, const TaeArgs args) {
  const long plane = (long)H * W;
  for (long i = (long)blockIdx.x * TB + threadIdx.x; i < n; i += (long)gridDim.x * TB) {
    const long p = i / plane, rem = i - p * plane;
    long a, b;
    tae_pair(p, args.stride, a, b);
    const float d = tae_depth(pred[a * plane + rem], args);
    if (!(d > 0.f && d <= 3.402823466e+38f)) continue;      // positive and finite; a NaN fails
    const int row = (int)(rem / W), col = (int)(rem - (long)row * W);
    const float* ka = K + a * 9;
    const float* kb = K + b * 9;
    const double* m = rel + p * 12;
    const double D = (double)d;
    const double X = (((double)col - (double)ka[2]) * D) / (double)ka[0];
    const double Y = (((double)row - (double)ka[5]) * D) / (double)ka[4];
    const double x3 = ((m[0] * X + m[1] * Y) + m[2] * D) + m[3];
    const double y3 = ((m[4] * X + m[5] * Y) + m[6] * D) + m[7];
    const double z3 = ((m[8] * X + m[9] * Y) + m[10] * D) + m[11];
    const double u = rint(((x3 / z3) * (double)kb[0]) + (double)kb[2]);      // ties to even
    const double v = rint(((y3 / z3) * (double)kb[4]) + (double)kb[5]);
    const float z = __double2float_rn(z3);
    if (!(z3 > 0.0 && z > 0.f && z <= 3.402823466e+38f && u >= 0.0 && v >= 0.0 && v < (double)H && u < (double)W)) continue;
    atomicMin(&zbuf[p * plane + (long)(int)v * W + (int)u], reg_key(z));
  }
}

__global__ __launch_bounds__(EVAL_NT) void k_tae_score(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const unsigned char* __restrict__ cmask, const unsigned* __restrict__ zbuf, long p0, int H,
                                                       int W, const TaeArgs args, double* __restrict__ part, float* __restrict__ warp_out,
                                                       float* __restrict__ err_out) {
  __shared__ double sh[EVAL_NT];
  const long plane = (long)H * W;
  const long p = p0 + blockIdx.y;
  long a, b;
  tae_pair(p, args.stride, a, b);
  double acc[2] = {0.0, 0.0};
  for (long q = (long)blockIdx.x * EVAL_NT + threadIdx.x; q < plane; q += (long)gridDim.x * EVAL_NT) {
    const unsigned key = zbuf[p * plane + q];
    const bool reached = key != TAE_EMPTY;
    const float z = reached ? reg_unkey(key) : 0.f;
    const float db = tae_depth(pred[b * plane + q], args);
    const float g = gt[b * plane + q];
    const bool ok = reached && db > 0.f && g > 0.f && !(g >= args.md) && (!cmask || cmask[b * plane + q]);
    float e = 0.f;
    if (ok) {
      const float diff = z - db;
      e = fabsf(diff) / db;
      acc[0] += (double)e; acc[1] += 1.0;
    }
    if (warp_out) warp_out[p * plane + q] = z;
    if (err_out) err_out[p * plane + q] = e;
  }
  eval_store_sums<2>(acc, sh, part + (p * (long)gridDim.x) * 2);
}

static int tae_blocks(long n) { long b = (n + TB - 1) / TB; return (int)(b > TMAXB ? TMAXB : (b < 1 ? 1 : b)); }

// pred / gt: [T,H,W]; cmask: NULL or [T,H,W]; K: [T,9] float32; rel: [P,12] doubles; zbuf, warp_out, err_out (either may be NULL): P*H*W words;
// part: P * nb * 2 doubles with nb = eval_nblocks(H * W), returned in *nb_out.  All on the device, P >= 1, P * H * W < 2^31.
void launch_tae(const float* pred, const float* gt, const unsigned char* cmask, const float* K, const double* rel, int P, int H, int W,
                const TaeArgs& a, unsigned* zbuf, double* part, float* warp_out, float* err_out, int* nb_out, hipStream_t s) {
  const long plane = (long)H * W, n = (long)P * plane;
  const int nb = tae_blocks(n), nbs = eval_nblocks(plane);
  hipLaunchKernelGGL(k_tae_fill, dim3(nb), dim3(TB), 0, s, zbuf, n);
  hipLaunchKernelGGL(k_tae_splat, dim3(nb), dim3(TB), 0, s, pred, K, rel, zbuf, n, H, W, a);
  for (long p0 = 0; p0 < P; p0 += 32768) {      // gridDim.y stays below 65536
    const int py = (int)((P - p0) < 32768 ? (P - p0) : 32768);
    hipLaunchKernelGGL(k_tae_score, dim3(nbs, py), dim3(EVAL_NT), 0, s, pred, gt, cmask, (const unsigned*)zbuf, p0, H, W, a, part, warp_out, err_out);
  }
  *nb_out = nbs;
}
