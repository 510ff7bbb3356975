// On-device evaluation metrics - the reference computes them on the host:
//   depth : /root/reference/metrics/eval_depth.py:6-246 as called by eval.py:49 (mask 0 < gt < 80, least-squares
//           scale/shift of metrics/alignment.py:150-167, AbsRel / SqRel / RMSE / LogRMSE / delta thresholds on the
//           custom mask)
//   normal: /root/reference/metrics/eval_normal.py:4-34 (angular error in degrees; mean / median / rmse / % under
//           5, 7.5, 11.25, 22.5, 30 degrees)
// All reductions are two-stage with a fixed order (eval_reduce.h: per-block fp64 partials, summed by the host in block order), the
// median is an exact two-pass histogram selection with integer atomics: results are deterministic.
// Depth has ONE least-squares fit kernel (k_depth_fit) and ONE metric kernel template (k_depth_metrics<UNFUSED, DISPARITY>): every entry point
// and every alignment mode goes through them, with clip bounds of -inf / +inf where a mode has none.
#include "../common.h"
#include "eval_reduce.h"
#include <utility>

// one selected pixel's terms of the nine metric sums: n, absrel, sqrel, sq, logsq, d1, d125, d125^2, d125^3 (prediction p, target g > 0)
__device__ __forceinline__ void metric_terms(float p, float g, double* a) {
  const float d = p - g;
  a[0] += 1.0; a[1] += fabsf(d) / g; a[2] += d * d / g; a[3] += d * d;
  const float pc = fmaxf(p, 1e-5f);
  const float l = logf(pc) - logf(g);
  a[4] += l * l;
  const float r = fmaxf(pc / g, g / pc);
  a[5] += r < 1.0f; a[6] += r < 1.25f; a[7] += r < 1.5625f; a[8] += r < 1.953125f;
}

// angular error per pixel (degrees), -1 for masked pixels; partial sums n, sum e, sum e^2, counts under 5 thresholds;
// coarse histogram (4096 bins over [0,180]) for the median
__global__ __launch_bounds__(EVAL_NT) void k_normal_err(const float* pn, const float* gn, const unsigned char* mask, long n, float* err,
                                                   double* part, unsigned* hist) {
  __shared__ double sh[EVAL_NT];
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    float e = -1.f;
    if (!mask || mask[i]) {
      const float px = pn[i * 3], py = pn[i * 3 + 1], pz = pn[i * 3 + 2];
      const float gx = gn[i * 3], gy = gn[i * 3 + 1], gz = gn[i * 3 + 2];
      const float dot = px * gx + py * gy + pz * gz;
      const float na = sqrtf(px * px + py * py + pz * pz), nb = sqrtf(gx * gx + gy * gy + gz * gz);
      float c = dot / (na * nb + 1e-6f);
      c = fminf(fmaxf(c, -1.f), 1.f);
      e = acosf(c) * 57.29577951308232f;
      a[0] += 1.0; a[1] += e; a[2] += (double)e * e;
      a[3] += e < 5.f; a[4] += e < 7.5f; a[5] += e < 11.25f; a[6] += e < 22.5f; a[7] += e < 30.f;
      int bin = (int)(e * (4096.0f / 180.0f)); bin = bin < 0 ? 0 : (bin > 4095 ? 4095 : bin);
      atomicAdd(&hist[bin], 1u);
    }
    err[i] = e;
  }
  eval_store_sums<8>(a, sh, part);
}

// collect the errors that fall into one histogram bin (the bin holding the median)
__global__ void k_collect_bin(const float* err, long n, int bin, float* out, unsigned* count, unsigned cap) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float e = err[i];
    if (e < 0.f) continue;
    int b = (int)(e * (4096.0f / 180.0f)); b = b < 0 ? 0 : (b > 4095 ? 4095 : b);
    if (b == bin) { const unsigned k = atomicAdd(count, 1u); if (k < cap) out[k] = e; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Alignment modes beyond least squares (restated from /root/reference/metrics/eval_depth.py:59-204 and
// metrics/alignment.py:170-195): optional clamps of the prediction before / after the alignment, the ratio of the (lower) medians,
// the Weiszfeld L1 scale, and the per-pixel error map.  mask1 = gt > 0 && !(gt >= max_depth); max_depth = NaN switches the upper
// bound off.  Clip bounds arrive as -inf / +inf when off, so the clamp is the identity.
__device__ __forceinline__ bool depth_valid(float g, float max_depth) { return g > 0.f && !(g >= max_depth); }
__device__ __forceinline__ float clipf(float p, float lo, float hi) { return fminf(fmaxf(p, lo), hi); }
// order-preserving 32-bit key of a float: negative values have all bits flipped, the others only the sign bit (-0.0 sorts just below 0.0)
__device__ __forceinline__ unsigned f32_key(float f) { const unsigned u = __float_as_uint(f); return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float key_f32(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// Exact masked selection: radix select of element (count - 1) / 2 of the sorted clamp(pred) and of the sorted gt over mask1, both in the
// same passes, 8 key bits per pass from the top.  Select state in device memory (unsigned words, zeroed before pass 0):
//   [(pass * 2 + a) * 256 + bin] histograms, a = 0 prediction / 1 ground truth; SEL_PREFIX + a the key bits fixed so far;
//   SEL_RANK + a the rank still to find inside that prefix; SEL_COUNT the mask1 count; SEL_MED + a the selected float (bits).
// (offsets in common.h.)  Counts are integers: the result does not depend on the order in which workgroups arrive.

template <int PASS>
__global__ __launch_bounds__(EVAL_NT) void k_select_hist(const float* pred, const float* gt, long n, float max_depth, float lo, float hi,
                                                    unsigned* sel) {
  __shared__ unsigned h[2][256];
  const int tid = threadIdx.x;
  h[0][tid] = 0; h[1][tid] = 0;
  __syncthreads();
  constexpr int shift = 24 - 8 * PASS;
  const unsigned pp = sel[SEL_PREFIX], pg = sel[SEL_PREFIX + 1];
  for (long i = (long)blockIdx.x * EVAL_NT + tid; i < n; i += (long)gridDim.x * EVAL_NT) {
    const float g = gt[i];
    if (!depth_valid(g, max_depth)) continue;
    const unsigned kp = f32_key(clipf(pred[i], lo, hi)), kg = f32_key(g);
    if constexpr (PASS == 0) {
      atomicAdd(&h[0][kp >> 24], 1u);
      atomicAdd(&h[1][kg >> 24], 1u);
    } else {
      if ((kp >> (shift + 8)) == (pp >> (shift + 8))) atomicAdd(&h[0][(kp >> shift) & 255u], 1u);
      if ((kg >> (shift + 8)) == (pg >> (shift + 8))) atomicAdd(&h[1][(kg >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  for (int a = 0; a < 2; ++a) {
    const unsigned cnt = h[a][tid];
    if (cnt) atomicAdd(&sel[(PASS * 2 + a) * 256 + tid], cnt);
  }
}

// one workgroup: pick the bin that holds the wanted rank and the rank inside it; the last pass turns the finished key back into the float
template <int PASS>
__global__ __launch_bounds__(256) void k_select_scan(unsigned* sel) {
  __shared__ unsigned sc[256];
  const int tid = threadIdx.x;
  constexpr int shift = 24 - 8 * PASS;
  for (int a = 0; a < 2; ++a) {
    const unsigned cnt = sel[(PASS * 2 + a) * 256 + tid];
    sc[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const unsigned v = tid >= o ? sc[tid - o] : 0u;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    const unsigned incl = sc[tid], excl = incl - cnt, total = sc[255];
    const unsigned k = PASS == 0 ? (total ? (total - 1) / 2 : 0u) : sel[SEL_RANK + a];
    __syncthreads();   // every thread has read the rank and sc[255] before one of them writes
    if (PASS == 0 && a == 0 && tid == 0) sel[SEL_COUNT] = total;
    if (cnt && excl <= k && k < incl) {
      const unsigned prefix = sel[SEL_PREFIX + a] | ((unsigned)tid << shift);
      sel[SEL_PREFIX + a] = prefix;
      sel[SEL_RANK + a] = k - excl;
      if (PASS == 3) sel[SEL_MED + a] = __float_as_uint(key_f32(prefix));
    }
  }
}

// Weiszfeld chain for the L1 scale: wz[0] = s, wz[1] = mask1 count.  INIT: partials of n, sum p, sum g -> s0 = mean(g) / mean(p);
// otherwise w = 1 / (|s p - g| + 1e-8), partials of sum(w p g), sum(w p p) -> s.  fp64 throughout, fixed grid, fixed order.
template <bool INIT>
__global__ __launch_bounds__(EVAL_NT) void k_wz_pass(const float* pred, const float* gt, long n, float max_depth, float lo, float hi,
                                                const double* wz, double* part) {
  __shared__ double sh[EVAL_NT];
  const double s = INIT ? 0.0 : wz[0];
  double a[3] = {0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const float gf = gt[i];
    if (!depth_valid(gf, max_depth)) continue;
    const double p = clipf(pred[i], lo, hi), g = gf;
    if (INIT) { a[0] += 1.0; a[1] += p; a[2] += g; }
    else { const double w = 1.0 / (fabs(s * p - g) + 1e-8); a[0] += w * p * g; a[1] += w * p * p; }
  }
  eval_store_sums<3>(a, sh, part);
}

// one workgroup: the partials summed in block order by one thread, the next s written for the next pass
template <bool INIT>
__global__ __launch_bounds__(EVAL_NT) void k_wz_reduce(const double* part, int nb, double* wz) {
  __shared__ double sh[EVAL_MAXB * 3];
  for (int i = threadIdx.x; i < nb * 3; i += EVAL_NT) sh[i] = part[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double a[3] = {0, 0, 0};
    for (int b = 0; b < nb; ++b) for (int k = 0; k < 3; ++k) a[k] += sh[b * 3 + k];
    if (INIT) { wz[1] = a[0]; wz[0] = (a[2] / a[0]) / (a[1] / a[0]); }
    else wz[0] = a[0] / a[1];
  }
}

// normal-equation sums of the least-squares fit over mask1, on the pre-clipped prediction: n, sum p, sum p^2, sum g, sum p*g
__global__ __launch_bounds__(EVAL_NT) void k_depth_fit(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, double* part) {
  __shared__ double sh[EVAL_NT];
  double a[5] = {0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const float g = gt[i];
    if (depth_valid(g, max_depth)) {
      const double p = clipf(pred[i], lo, hi);
      a[0] += 1.0; a[1] += p; a[2] += p * p; a[3] += g; a[4] += p * (double)g;
    }
  }
  eval_store_sums<5>(a, sh, part);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Alignment in disparity space (UG_DEPTH_ALIGN_DISPARITY; the disp_input branch of /root/reference/metrics/eval_depth.py:75-78,
// 123-126,169-198 with the depth2disparity it never defines supplied: y = 1 / x where x > 0, else 0).  The prediction is a disparity: it is fitted
// against gd = 1 / (gt + 1e-8f) on mask1, the aligned disparity is inverted, and the metrics are taken against the real gt.
// Target pass: gfit = mask1 ? gd : 0.  gd > 0 on mask1, so the fit kernels above, launched with gfit in the place of gt and the depth bound off, see
// mask1 through their own test g > 0.
__global__ __launch_bounds__(EVAL_NT) void k_disp_target(const float* gt, long n, float max_depth, float* gfit) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const float g = gt[i];
    gfit[i] = depth_valid(g, max_depth) ? 1.0f / (g + 1e-8f) : 0.f;
  }
}
// aligned disparity -> depth: the optional floor (NaN: off; a NaN disparity stays NaN), then 1 / a where a > 0, else 0.  The division is the
// compiler's default, correctly rounded one.
__device__ __forceinline__ float disp_to_depth(float a, float floor_) {
  if (a < floor_) a = floor_;
  return a > 0.f ? 1.0f / a : 0.f;
}

// The nine metric sums of p' = clamp(A(s, clamp(p, lo, hi)), plo, phi) on mask1 & custom mask; optional error map |A(pred, s) - gt| / gt on mask1
// (0 elsewhere) from the ORIGINAL prediction.  A(a, b) is the aligned value a * b + t, in disparity space inverted by disp_to_depth (floor_ = NaN:
// no floor) before it meets the real gt.  The reference's tensor expressions round the product and the sum separately; a fused multiply-add
// moves the map by more than its tolerance where the residual is small.
// UNFUSED: in this toolchain __fmul_rn / __fadd_rn are plain operators, and the default instantiation's s * p + t does come out as one fused
// operation (see world_point below).  With t = 0 (median, scale, metric) that changes no bit, and least squares is compared within a tolerance; the
// L1 alignment's line passes through two of the pixels, where the residual is a rounding error and the fused form differs from the host's in every
// digit.  It instantiates the kernel with contraction off; the other modes keep the code, and the bytes, they had.
// DISPARITY implies UNFUSED in every mode: the inversion carries a rounding of the aligned disparity into the depth, and the depth is compared
// with the host's byte for byte.
__device__ __forceinline__ float mul_add_unfused(float a, float b, float c) {
#pragma clang fp contract(off)
  const float m = a * b;
  return m + c;
}
template <bool UNFUSED, bool DISPARITY>
__device__ __forceinline__ float aligned_depth(float a, float b, float t, float floor_) {
  const float v = UNFUSED ? mul_add_unfused(a, b, t) : __fadd_rn(__fmul_rn(a, b), t);
  return DISPARITY ? disp_to_depth(v, floor_) : v;
}
template <bool UNFUSED, bool DISPARITY>
__global__ __launch_bounds__(EVAL_NT) void k_depth_metrics(const float* pred, const float* gt, const unsigned char* cmask, long n, float max_depth,
                                                           float lo, float hi, float plo, float phi, float floor_, float s, float t, double* part,
                                                           float* emap) {
  static_assert(UNFUSED || !DISPARITY, "the disparity form is unfused");
  __shared__ double sh[EVAL_NT];
  double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const float g = gt[i];
    const bool v1 = depth_valid(g, max_depth);
    const float p0 = pred[i];
    if (emap) emap[i] = v1 ? fabsf(__fsub_rn(aligned_depth<UNFUSED, DISPARITY>(p0, s, t, floor_), g)) / g : 0.f;
    if (v1 && (!cmask || cmask[i])) {
      const float p = clipf(aligned_depth<UNFUSED, DISPARITY>(s, clipf(p0, lo, hi), t, floor_), plo, phi);
      metric_terms(p, g, a);
    }
  }
  eval_store_sums<9>(a, sh, part);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Depth evaluation in global coordinates (restated from /root/reference/metrics/eval_depth.py:250-441 and
// utils/geometry_utils.py:246-253).  After the first fit (k_depth_fit) gave (s, t): the aligned, post-clipped depth
// d = clamp(s * pred + t, plo, phi) of EVERY pixel from the ORIGINAL prediction, float32 with the product and the sum rounded separately;
// then in fp64 from that float32 d: x = (col - cx) * d / fx, y = (row - cy) * d / fy, z = d (integer pixel indices), world = R (x, y, z) + t
// with the frame's pose, r = |world| rounded once to float32 and written out.  The same pass accumulates the normal-equation sums of the
// second fit, r against the ground-truth radius over mask1 of the ground-truth DEPTH: n, sum r, sum r^2, sum g_r, sum r * g_r.
// cam: 16 doubles per frame - fx, fy, cx, cy, R row-major, t - widened from float32 by the host.  The fp64 products and sums stay
// unfused: the arithmetic the fixture's generator emulates.
// One pixel of the chain above: the aligned, post-clipped float32 depth of pixel i -> its world coordinates in fp64 (shared by k_world_radius and
// k_world_points).  Contraction is switched off for the body: the __fmul_rn / __dmul_rn family are plain operators in this toolchain, and with
// them s * pred + t came out as ONE fused operation - a float32 depth one ulp away from the host's on a share of the pixels, which the point-cloud
// metrics see.
__device__ __forceinline__ void world_point(const float* pred, const double* cam, long i, long hw, int W, float plo, float phi, float s, float t,
                                            double& wx, double& wy, double& wz) {
#pragma clang fp contract(off)
  const long f = i / hw;
  const long rem = i - f * hw;
  const int row = (int)(rem / W), col = (int)(rem - (long)row * W);
  const double* q = cam + f * 16;
  const float d = s * pred[i] + t;
  const double z = clipf(d, plo, phi);
  const double x = ((double)col - q[2]) * z / q[0], y = ((double)row - q[3]) * z / q[1];
  wx = ((q[4] * x + q[5] * y) + q[6] * z) + q[13];
  wy = ((q[7] * x + q[8] * y) + q[9] * z) + q[14];
  wz = ((q[10] * x + q[11] * y) + q[12] * z) + q[15];
}

__global__ __launch_bounds__(EVAL_NT) void k_world_radius(const float* pred, const float* gt, const float* gt_radius, const double* cam, long n,
                                                     int H, int W, float max_depth, float plo, float phi, float s, float t, float* radius,
                                                     double* part) {
  __shared__ double sh[EVAL_NT];
  double a[5] = {0, 0, 0, 0, 0};
  const long hw = (long)H * W;
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    double wx, wy, wz;
    world_point(pred, cam, i, hw, W, plo, phi, s, t, wx, wy, wz);
    const float rf = (float)sqrt(__dadd_rn(__dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy)), __dmul_rn(wz, wz)));
    radius[i] = rf;
    if (depth_valid(gt[i], max_depth)) {
      const double r = rf, g = gt_radius[i];
      a[0] += 1.0; a[1] += r; a[2] += r * r; a[3] += g; a[4] += r * g;
    }
  }
  eval_store_sums<5>(a, sh, part);
}

// the world points themselves, each coordinate rounded once to float32 (ug_pcd_world_points)
__global__ __launch_bounds__(EVAL_NT) void k_world_points(const float* pred, const double* cam, long n, int H, int W, float plo, float phi, float s,
                                                     float t, float* pts) {
  const long hw = (long)H * W;
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    double wx, wy, wz;
    world_point(pred, cam, i, hw, W, plo, phi, s, t, wx, wy, wz);
    pts[i * 3] = (float)wx; pts[i * 3 + 1] = (float)wy; pts[i * 3 + 2] = (float)wz;
  }
}

// the nine metric sums of p' = s * r + t (two roundings, no clamp) against the ground-truth radius on mask1 of the ground-truth DEPTH & custom
// mask; p' of every pixel goes to rmap when one is asked for
__global__ __launch_bounds__(EVAL_NT) void k_radius_metrics(const float* radius, const float* gt, const float* gt_radius, const unsigned char* cmask,
                                                       long n, float max_depth, float s, float t, double* part, float* rmap) {
  __shared__ double sh[EVAL_NT];
  double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const float p = __fadd_rn(__fmul_rn(s, radius[i]), t);
    if (rmap) rmap[i] = p;
    if (depth_valid(gt[i], max_depth) && (!cmask || cmask[i])) metric_terms(p, gt_radius[i], a);
  }
  eval_store_sums<9>(a, sh, part);
}

void launch_normal_err(const float* pn, const float* gn, const unsigned char* mask, long n, float* err, double* part,
                       unsigned* hist, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_normal_err, dim3(*nb), dim3(EVAL_NT), 0, s, pn, gn, mask, n, err, part, hist);
}
void launch_collect_bin(const float* err, long n, int bin, float* out, unsigned* count, unsigned cap, hipStream_t s) {
  hipLaunchKernelGGL(k_collect_bin, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, err, n, bin, out, count, cap);
}

// the four histogram / scan pairs back to back on one stream: sel (SEL_WORDS unsigned words) ends with the count and the two medians
void launch_masked_median(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, unsigned* sel, hipStream_t s) {
  (void)hipMemsetAsync(sel, 0, SEL_WORDS * sizeof(unsigned), s);
  const dim3 g(eval_nblocks(n)), b(EVAL_NT);
  hipLaunchKernelGGL(k_select_hist<0>, g, b, 0, s, pred, gt, n, max_depth, lo, hi, sel);
  hipLaunchKernelGGL(k_select_scan<0>, dim3(1), dim3(256), 0, s, sel);
  hipLaunchKernelGGL(k_select_hist<1>, g, b, 0, s, pred, gt, n, max_depth, lo, hi, sel);
  hipLaunchKernelGGL(k_select_scan<1>, dim3(1), dim3(256), 0, s, sel);
  hipLaunchKernelGGL(k_select_hist<2>, g, b, 0, s, pred, gt, n, max_depth, lo, hi, sel);
  hipLaunchKernelGGL(k_select_scan<2>, dim3(1), dim3(256), 0, s, sel);
  hipLaunchKernelGGL(k_select_hist<3>, g, b, 0, s, pred, gt, n, max_depth, lo, hi, sel);
  hipLaunchKernelGGL(k_select_scan<3>, dim3(1), dim3(256), 0, s, sel);
}
// initial means + iters Weiszfeld steps, no host synchronisation in between: wz[0] = s, wz[1] = mask1 count; part holds EVAL_MAXB * 3 doubles
void launch_weiszfeld_scale(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, int iters, double* wz,
                            double* part, hipStream_t s) {
  const int nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_wz_pass<true>, dim3(nb), dim3(EVAL_NT), 0, s, pred, gt, n, max_depth, lo, hi, wz, part);
  hipLaunchKernelGGL(k_wz_reduce<true>, dim3(1), dim3(EVAL_NT), 0, s, part, nb, wz);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(k_wz_pass<false>, dim3(nb), dim3(EVAL_NT), 0, s, pred, gt, n, max_depth, lo, hi, wz, part);
    hipLaunchKernelGGL(k_wz_reduce<false>, dim3(1), dim3(EVAL_NT), 0, s, part, nb, wz);
  }
}
void launch_depth_fit(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, double* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_depth_fit, dim3(*nb), dim3(EVAL_NT), 0, s, pred, gt, n, max_depth, lo, hi, part);
}
void launch_depth_metrics(const float* pred, const float* gt, const unsigned char* cmask, long n, float max_depth, float lo, float hi, float plo,
                          float phi, float floor_, float sc, float sh, double* part, float* emap, int* nb, hipStream_t s, bool unfused,
                          bool disparity) {
  *nb = eval_nblocks(n);
  const auto k = disparity ? k_depth_metrics<true, true> : (unfused ? k_depth_metrics<true, false> : k_depth_metrics<false, false>);
  hipLaunchKernelGGL(k, dim3(*nb), dim3(EVAL_NT), 0, s, pred, gt, cmask, n, max_depth, lo, hi, plo, phi, floor_, sc, sh, part, emap);
}
void launch_disp_target(const float* gt, long n, float max_depth, float* gfit, hipStream_t s) {
  hipLaunchKernelGGL(k_disp_target, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, gt, n, max_depth, gfit);
}
void launch_world_radius(const float* pred, const float* gt, const float* gt_radius, const double* cam, long n, int H, int W, float max_depth,
                         float plo, float phi, float sc, float sh, float* radius, double* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_world_radius, dim3(*nb), dim3(EVAL_NT), 0, s, pred, gt, gt_radius, cam, n, H, W, max_depth, plo, phi, sc, sh, radius, part);
}
void launch_world_points(const float* pred, const double* cam, long n, int H, int W, float plo, float phi, float sc, float sh, float* pts,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_world_points, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, pred, cam, n, H, W, plo, phi, sc, sh, pts);
}
void launch_radius_metrics(const float* radius, const float* gt, const float* gt_radius, const unsigned char* cmask, long n, float max_depth,
                           float sc, float sh, double* part, float* rmap, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_radius_metrics, dim3(*nb), dim3(EVAL_NT), 0, s, radius, gt, gt_radius, cmask, n, max_depth, sc, sh, part, rmap);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Exact L1 scale-and-shift alignment (UG_ALIGN_L1): min over (s, t) of sum |s p_i + t - g_i| on mask1.  The pre-clipped
// prediction is held as the integers q = rint(p * 2^(36 - E)), E the smallest integer with max |p| < 2^E, so every weight |q_i - q_j| and every
// sum of weights is an exact integer; q and g of the valid pixels are compacted once, in pixel order.  One step from pivot j is a WEIGHTED
// radix select - the lower weighted median of the slopes r_i = (g_i - g_j) / ((q_i - q_j) * 2^(E - 36)) with the weights |q_i - q_j| - over the
// order-preserving 64-bit key of r_i, 8 bits per pass, then a pass that collects the points whose slope equals the result.  The host
// (capi_util.h: l1_fit_device) walks from vertex to vertex with k_l1_check.  Every accumulated quantity is an integer: no result depends on the
// order in which workgroups arrive.  State words (unsigned 64-bit, offsets in common.h): L1_HIST + pass * 256 + bin, L1_PREFIX the key bits
// fixed so far, L1_TARGET the weight still to reach inside that prefix, L1_W the total weight, L1_TIE_MIN / L1_TIE_CNT the lowest index and
// the number of points whose key equals the selected one, L1_CHK + 3 * slot the sums (below, above, total) of one k_l1_check.
typedef unsigned long long u64;

// the valid pixels are compacted in pixel order: block b owns the pixels [b * chunk, (b + 1) * chunk), chunk a multiple of the block size
static long l1_chunk(long n, int nb) { const long c = (n + nb - 1) / nb; return (c + EVAL_NT - 1) / EVAL_NT * EVAL_NT; }

__device__ __forceinline__ double l1_slope(long long dq, float gi, double gj, double down) {
#pragma clang fp contract(off)
  const double r = ((double)gi - gj) / ((double)dq * down);
  return r == 0.0 ? 0.0 : r;      // -0.0 -> 0.0
}

// the bits of max |clamp(pred)| over mask1 (integer atomicMax: non-negative floats order as their bits do) and every block's count of valid pixels
__global__ __launch_bounds__(EVAL_NT) void k_l1_maxabs(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, long chunk,
                                                  unsigned* maxbits, unsigned* bcount) {
  __shared__ unsigned sm[EVAL_NT], sc[EVAL_NT];
  const int tid = threadIdx.x;
  const long beg = (long)blockIdx.x * chunk, end = beg + chunk < n ? beg + chunk : n;
  unsigned mx = 0, cnt = 0;
  for (long i = beg + tid; i < end; i += EVAL_NT) {
    if (!depth_valid(gt[i], max_depth)) continue;
    const unsigned b = __float_as_uint(fabsf(clipf(pred[i], lo, hi)));
    mx = b > mx ? b : mx; ++cnt;
  }
  sm[tid] = mx; sc[tid] = cnt;
  __syncthreads();
  for (int o = EVAL_NT / 2; o > 0; o >>= 1) {
    if (tid < o) { sm[tid] = sm[tid + o] > sm[tid] ? sm[tid + o] : sm[tid]; sc[tid] += sc[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { if (sm[0]) atomicMax(maxbits, sm[0]); bcount[blockIdx.x] = sc[0]; }
}

// q = rint(clamp(pred) * up) and gt of the valid pixels, written in pixel order: a block starts at the sum of the counts of the blocks before
// it and scans each of its 256-pixel tiles.  *j0 = the lowest compacted index whose clamped prediction equals med.  cap = the compacted length.
// launch_pcd_compact (kernels/pcd.hip) keeps the same order but copies float32 pairs on the custom mask; this one selects on mask1, clamps and
// quantises as it writes and finds j0 in the same trip, and the block counts come from k_l1_maxabs, which reads the pixels anyway.
__global__ __launch_bounds__(EVAL_NT) void k_l1_compact(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, long chunk,
                                                   const unsigned* bcount, double up, float med, unsigned cap, long long* qc, float* gc,
                                                   unsigned* j0) {
  __shared__ unsigned sc[EVAL_NT];
  const int tid = threadIdx.x;
  unsigned part = 0;
  for (int b = tid; b < (int)blockIdx.x; b += EVAL_NT) part += bcount[b];
  sc[tid] = part;
  __syncthreads();
  for (int o = EVAL_NT / 2; o > 0; o >>= 1) {
    if (tid < o) sc[tid] += sc[tid + o];
    __syncthreads();
  }
  unsigned running = sc[0];
  __syncthreads();
  const long beg = (long)blockIdx.x * chunk, end = beg + chunk < n ? beg + chunk : n;
  for (long t0 = beg; t0 < end; t0 += EVAL_NT) {
    const long i = t0 + tid;
    const float g = i < end ? gt[i] : 0.f;
    const bool v = i < end && depth_valid(g, max_depth);
    sc[tid] = v;
    __syncthreads();
    for (int o = 1; o < EVAL_NT; o <<= 1) {
      const unsigned a = tid >= o ? sc[tid - o] : 0u;
      __syncthreads();
      sc[tid] += a;
      __syncthreads();
    }
    const unsigned pos = running + sc[tid] - 1u;
    running += sc[EVAL_NT - 1];
    if (v && pos < cap) {
      const float p = clipf(pred[i], lo, hi);
      qc[pos] = __double2ll_rn((double)p * up);
      gc[pos] = g;
      if (p == med) atomicMin(j0, pos);
    }
    __syncthreads();
  }
}

// one 8-bit pass of the weighted select: the weight |q_i - q_j| of every point whose key matches the prefix goes into the bin of its next 8 bits.
// A thread sums the weights of consecutive points that fall into one bin in a register and issues the LDS atomic only when the bin changes:
// in the first passes (sign and exponent bits) nearly every slope shares a bin, and one atomic per point would serialise on that address.
// The sums are integers, so the grouping changes no bit.
template <int PASS>
__global__ __launch_bounds__(EVAL_NT) void k_l1_hist(const long long* qc, const float* gc, long nv, long j, double down, u64* st) {
  __shared__ u64 h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  constexpr int shift = 56 - 8 * PASS;
  const long long qj = qc[j];
  const double gj = gc[j];
  const u64 prefix = st[L1_PREFIX];
  unsigned bin = 0;
  u64 run = 0;
  for (long i = (long)blockIdx.x * EVAL_NT + tid; i < nv; i += (long)gridDim.x * EVAL_NT) {
    const long long dq = qc[i] - qj;
    if (dq == 0) continue;
    const u64 key = pcd_key(l1_slope(dq, gc[i], gj, down));
    if constexpr (PASS > 0) { if ((key >> (shift + 8)) != (prefix >> (shift + 8))) continue; }
    const unsigned b = (unsigned)(key >> shift) & 255u;
    if (b != bin) {
      if (run) atomicAdd(&h[bin], run);
      bin = b; run = 0;
    }
    run += (u64)(dq < 0 ? -dq : dq);
  }
  if (run) atomicAdd(&h[bin], run);
  __syncthreads();
  const u64 c = h[tid];
  if (c) atomicAdd(&st[L1_HIST + PASS * 256 + tid], c);
}

// one workgroup: the bin in which the running weight first reaches the target; pass 0 sets the target ceil(W / 2) and arms the tie words
template <int PASS>
__global__ __launch_bounds__(256) void k_l1_scan(u64* st) {
  __shared__ u64 sc[256];
  const int tid = threadIdx.x;
  constexpr int shift = 56 - 8 * PASS;
  const u64 cnt = st[L1_HIST + PASS * 256 + tid];
  sc[tid] = cnt;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const u64 v = tid >= o ? sc[tid - o] : 0ull;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  const u64 incl = sc[tid], excl = incl - cnt, total = sc[255];
  const u64 target = PASS == 0 ? total / 2 + (total & 1ull) : st[L1_TARGET];
  __syncthreads();   // every thread has read the target before one of them writes
  if (PASS == 0 && tid == 0) { st[L1_W] = total; st[L1_TIE_MIN] = ~0ull; }
  if (cnt && excl < target && target <= incl) {
    st[L1_PREFIX] = st[L1_PREFIX] | ((u64)tid << shift);
    st[L1_TARGET] = target - excl;
  }
}

// the points whose slope through j has the selected key: the lowest index, how many, and the first L1_MAX_TIES of them (index and q, any order)
__global__ __launch_bounds__(EVAL_NT) void k_l1_tie(const long long* qc, const float* gc, long nv, long j, double down, u64* st, unsigned* tie_idx,
                                               long long* tie_q) {
  const long long qj = qc[j];
  const double gj = gc[j];
  const u64 want = st[L1_PREFIX];
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < nv; i += (long)gridDim.x * EVAL_NT) {
    const long long qi = qc[i], dq = qi - qj;
    if (dq == 0 || pcd_key(l1_slope(dq, gc[i], gj, down)) != want) continue;
    atomicMin(&st[L1_TIE_MIN], (u64)i);
    const u64 c = atomicAdd(&st[L1_TIE_CNT], 1ull);
    if (c < L1_MAX_TIES) { tie_idx[c] = (unsigned)i; tie_q[c] = qi; }
  }
}

// with pivot z: the weight of the slopes below S, above S, and the total weight -> out3 (one 64-bit integer atomicAdd per block and sum)
__global__ __launch_bounds__(EVAL_NT) void k_l1_check(const long long* qc, const float* gc, long nv, long z, double S, double down, u64* out3) {
  __shared__ u64 sh[3][EVAL_NT];
  const int tid = threadIdx.x;
  const long long qz = qc[z];
  const double gz = gc[z];
  u64 a[3] = {0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + tid; i < nv; i += (long)gridDim.x * EVAL_NT) {
    const long long dq = qc[i] - qz;
    if (dq == 0) continue;
    const double r = l1_slope(dq, gc[i], gz, down);
    const u64 w = (u64)(dq < 0 ? -dq : dq);
    if (r < S) a[0] += w;
    if (r > S) a[1] += w;
    a[2] += w;
  }
  for (int k = 0; k < 3; ++k) sh[k][tid] = a[k];
  __syncthreads();
  for (int o = EVAL_NT / 2; o > 0; o >>= 1) {
    if (tid < o) for (int k = 0; k < 3; ++k) sh[k][tid] += sh[k][tid + o];
    __syncthreads();
  }
  if (tid < 3 && sh[tid][0]) atomicAdd(&out3[tid], sh[tid][0]);
}

// aux: [0] the bits of max |p|, [1] j0, [2 ..] EVAL_MAXB block counts.  Counts the valid pixels per block and finds max |p|.
void launch_l1_maxabs(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, unsigned* aux, hipStream_t s) {
  const int nb = eval_nblocks(n);
  (void)hipMemsetAsync(aux, 0, 4, s);
  (void)hipMemsetAsync(aux + 1, 0xff, 4, s);
  hipLaunchKernelGGL(k_l1_maxabs, dim3(nb), dim3(EVAL_NT), 0, s, pred, gt, n, max_depth, lo, hi, l1_chunk(n, nb), aux, aux + 2);
}
void launch_l1_compact(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, unsigned* aux, double up, float med,
                       unsigned cap, long long* qc, float* gc, hipStream_t s) {
  const int nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_l1_compact, dim3(nb), dim3(EVAL_NT), 0, s, pred, gt, n, max_depth, lo, hi, l1_chunk(n, nb), aux + 2, up, med, cap, qc, gc,
                     aux + 1);
}
// one hist / scan pair of the weighted select, and the eight of them from the top byte of the key down
template <int PASS>
static void l1_select_pass(dim3 g, hipStream_t s, const long long* qc, const float* gc, long nv, long j, double down, u64* st) {
  hipLaunchKernelGGL(k_l1_hist<PASS>, g, dim3(EVAL_NT), 0, s, qc, gc, nv, j, down, st);
  hipLaunchKernelGGL(k_l1_scan<PASS>, dim3(1), dim3(256), 0, s, st);
}
template <int... PASS>
static void l1_select_passes(std::integer_sequence<int, PASS...>, dim3 g, hipStream_t s, const long long* qc, const float* gc, long nv, long j,
                             double down, u64* st) {
  (l1_select_pass<PASS>(g, s, qc, gc, nv, j, down, st), ...);
}
// one pivot step from point j of the nv compacted points: st ends with the selected key (L1_PREFIX), W, and the tie words; tie_idx / tie_q hold
// L1_MAX_TIES entries
void launch_l1_step(const long long* qc, const float* gc, long nv, long j, double down, u64* st, unsigned* tie_idx, long long* tie_q,
                    hipStream_t s) {
  (void)hipMemsetAsync(st, 0, L1_WORDS * sizeof(u64), s);
  const dim3 g(eval_nblocks(nv)), b(EVAL_NT);
  l1_select_passes(std::make_integer_sequence<int, 8>{}, g, s, qc, gc, nv, j, down, st);
  hipLaunchKernelGGL(k_l1_tie, g, b, 0, s, qc, gc, nv, j, down, st, tie_idx, tie_q);
}
// out3 must be zero before the launch
void launch_l1_check(const long long* qc, const float* gc, long nv, long z, double S, double down, u64* out3, hipStream_t s) {
  hipLaunchKernelGGL(k_l1_check, dim3(eval_nblocks(nv)), dim3(EVAL_NT), 0, s, qc, gc, nv, z, S, down, out3);
}
