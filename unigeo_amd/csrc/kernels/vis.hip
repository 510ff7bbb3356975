// Depth / normal visualisation panels composed on the device - the reference composes them on the host:
//   the reference's utils/vis_utils.py:38-84 (save_depth_normal_maps) and :139-199 (colorize_np), as called by eval.py:58-62.
// One image per frame: rgb | normals * 0.5 + 0.5 | depth through a 256-entry colour table over the clip's min..max | 5 black columns | colour bar,
// every float section turned into bytes by trunc(x * 255).  Each step is ONE float32 operation rounded on its own (__fmul_rn / __fadd_rn /
// __fsub_rn / __fdiv_rn keep the compiler from fusing them): the bytes equal the reference's, not only approximately.
#include "../common.h"

#define VB 256     // threads per block
#define VMAXB 1024

// trunc(x) as a byte: saturates to 0..255, NaN -> 0 (numpy's cast is undefined outside 0..255; no reference input gets there)
__device__ __forceinline__ unsigned to_u8(float v) { return !(v > 0.f) ? 0u : (v >= 255.f ? 255u : (unsigned)(int)v); }
__device__ __forceinline__ unsigned unit_to_u8(float x) { return to_u8(__fmul_rn(x, 255.f)); }

// clip-wide min and max, NaN ignored (fminf / fmaxf return the other operand): per-block partials (min, max), then k_vis_range_final
__global__ __launch_bounds__(VB) void k_vis_range(const float* x, long n, float* part) {
  __shared__ float smn[VB], smx[VB];
  const int tid = threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (long i = (long)blockIdx.x * VB + tid; i < n; i += (long)gridDim.x * VB) {
    const float v = x[i];
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  smn[tid] = mn; smx[tid] = mx;
  __syncthreads();
  for (int o = VB / 2; o > 0; o >>= 1) {
    if (tid < o) { smn[tid] = fminf(smn[tid], smn[tid + o]); smx[tid] = fmaxf(smx[tid], smx[tid + o]); }
    __syncthreads();
  }
  if (tid == 0) { part[blockIdx.x * 2] = smn[0]; part[blockIdx.x * 2 + 1] = smx[0]; }
}

// one workgroup: the nb partials -> out2 = (vmin, vmax); nothing but NaN (or nothing at all) leaves min = +inf > max = -inf -> (0, 0)
__global__ __launch_bounds__(VB) void k_vis_range_final(const float* part, int nb, float* out2) {
  __shared__ float smn[VB], smx[VB];
  const int tid = threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (int b = tid; b < nb; b += VB) { mn = fminf(mn, part[b * 2]); mx = fmaxf(mx, part[b * 2 + 1]); }
  smn[tid] = mn; smx[tid] = mx;
  __syncthreads();
  for (int o = VB / 2; o > 0; o >>= 1) {
    if (tid < o) { smn[tid] = fminf(smn[tid], smn[tid + o]); smx[tid] = fmaxf(smx[tid], smx[tid + o]); }
    __syncthreads();
  }
  if (tid == 0) { const bool none = smn[0] > smx[0]; out2[0] = none ? 0.f : smn[0]; out2[1] = none ? 0.f : smx[0]; }
}

struct VisArgs {
  const float* rgb;      // [T,H,W,3] in [0,1] or NULL (no rgb section)
  const float* normals;  // [T,H,W,3]
  const float* depth;    // [T,H,W]
  const float* lut;      // [256,3]
  const float* cbar;     // [H,Wc,3] or NULL (the panel ends after the depth section)
  unsigned char* out;    // [T,H,Wp,3]
  long rows;             // T * H
  int H, W, Wc, Wp;
  float vmin, vmax;
};

// the three bytes of output pixel (row = t * H + y, col), packed r | g << 8 | b << 16
__device__ __forceinline__ unsigned panel_pixel(const VisArgs& a, const unsigned char* slut, long row, int col) {
  if (a.rgb) {
    if (col < a.W) { const float* p = a.rgb + (row * a.W + col) * 3; return unit_to_u8(p[0]) | unit_to_u8(p[1]) << 8 | unit_to_u8(p[2]) << 16; }
    col -= a.W;
  }
  if (col < a.W) {
    const float* p = a.normals + (row * a.W + col) * 3;
    unsigned r = 0;
    for (int c = 0; c < 3; ++c) r |= unit_to_u8(__fadd_rn(__fmul_rn(p[c], 0.5f), 0.5f)) << (8 * c);
    return r;
  }
  col -= a.W;
  if (col < a.W) {
    const float d = a.depth[row * a.W + col];
    if (d != d) return 0u;                                                  // matplotlib's "bad" colour
    const float x = fminf(fmaxf(d, a.vmin), a.vmax);
    const float u = __fdiv_rn(__fsub_rn(x, a.vmin), __fsub_rn(a.vmax, a.vmin));
    if (!(u == u)) return 0u;                                               // vmax == vmin: 0 / 0
    const float v = __fmul_rn(u, 256.f);
    const int i = !(v > 0.f) ? 0 : (v >= 255.f ? 255 : (int)v);
    return slut[i * 3] | (unsigned)slut[i * 3 + 1] << 8 | (unsigned)slut[i * 3 + 2] << 16;
  }
  col -= a.W;
  if (col < 5) return 0u;
  col -= 5;
  const float* p = a.cbar + ((row % a.H) * a.Wc + col) * 3;
  return unit_to_u8(p[0]) | unit_to_u8(p[1]) << 8 | unit_to_u8(p[2]) << 16;
}

// Four consecutive pixels of the FLAT output (rows are Wp * 3 bytes with no padding, Wp is any number) per thread: pixel 4 q starts at byte
// 12 q, so the twelve bytes go out as three aligned 32-bit words wherever the rows start; a wave writes 768 contiguous bytes.  The last
// thread of the clip writes the npix % 4 leftover pixels byte by byte.  The colour table becomes 768 bytes in LDS once per workgroup.
__global__ __launch_bounds__(VB) void k_vis_panel(const VisArgs a) {
  __shared__ unsigned char slut[768];
  for (int i = threadIdx.x; i < 768; i += VB) slut[i] = (unsigned char)unit_to_u8(a.lut[i]);
  __syncthreads();
  const long npix = a.rows * a.Wp, nquad = (npix + 3) / 4;
  for (long q = (long)blockIdx.x * VB + threadIdx.x; q < nquad; q += (long)gridDim.x * VB) {
    const long p0 = q * 4;
    long row = p0 / a.Wp;
    int col = (int)(p0 - row * a.Wp);
    const int cnt = npix - p0 < 4 ? (int)(npix - p0) : 4;
    unsigned px[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < cnt; ++k) {
      px[k] = panel_pixel(a, slut, row, col);
      if (++col == a.Wp) { col = 0; ++row; }
    }
    if (cnt == 4) {
      unsigned* o = (unsigned*)(a.out + p0 * 3);                            // 12 q bytes into a 256-byte-aligned buffer
      o[0] = px[0] | px[1] << 24;
      o[1] = px[1] >> 8 | px[2] << 16;
      o[2] = px[2] >> 16 | px[3] << 8;
    } else {
      for (int k = 0; k < cnt; ++k)
        for (int c = 0; c < 3; ++c) a.out[(p0 + k) * 3 + c] = (unsigned char)(px[k] >> (8 * c));
    }
  }
}

static int vis_blocks(long n) { long b = (n + VB - 1) / VB; return (int)(b > VMAXB ? VMAXB : (b < 1 ? 1 : b)); }

// part: 2 * 1024 floats of scratch; out2 (device) = (vmin, vmax)
void launch_vis_range(const float* x, long n, float* part, float* out2, hipStream_t s) {
  const int nb = vis_blocks(n);
  hipLaunchKernelGGL(k_vis_range, dim3(nb), dim3(VB), 0, s, x, n, part);
  hipLaunchKernelGGL(k_vis_range_final, dim3(1), dim3(VB), 0, s, part, nb, out2);
}
// out: [T,H,Wp,3] bytes, 4-byte aligned, Wp = (rgb ? W : 0) + 2 W + (cbar ? 5 + Wc : 0)
void launch_vis_panel(const float* rgb, const float* normals, const float* depth, const float* lut, const float* cbar, unsigned char* out, int T,
                      int H, int W, int Wc, float vmin, float vmax, hipStream_t s) {
  VisArgs a;
  a.rgb = rgb; a.normals = normals; a.depth = depth; a.lut = lut; a.cbar = cbar; a.out = out;
  a.rows = (long)T * H; a.H = H; a.W = W; a.Wc = cbar ? Wc : 0;
  a.Wp = (rgb ? W : 0) + 2 * W + (cbar ? 5 + Wc : 0);
  a.vmin = vmin; a.vmax = vmax;
  const long nquad = (a.rows * a.Wp + 3) / 4;
  hipLaunchKernelGGL(k_vis_panel, dim3(vis_blocks(nquad)), dim3(VB), 0, s, a);
}
