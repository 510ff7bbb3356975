// ScanNet++ clip preparation on the device - the reference does it in numpy / scikit-image on the host:
//   dataset/dataset_core/transforms.py:38-110 (anti-aliased input resize, order-0 target resize) and dataset/scannetpp/scannetpp.py:81-187
//   (back-projection, normal decode, key-view transform, validity mask).
// The resize is a separable linear map whose per-axis tap tables (source index, float64 weight, fixed length) the HOST builds: no kernel here
// computes a coordinate or mirrors an index, it gathers what the table names.  The tables are validated before upload (0 <= idx < n_in), and
// every other address is an affine function of the thread's own output index.
#include "../common.h"
#include "prep_point.h"      // prep_point: the back-projection of one depth pixel and the loaders' `bad` rule

#define PB 256       // threads per block
#define PMAXB 1024   // grid cap; the loops below stride over the rest

// Vertical pass: frames uint8 [T,Hi,Wi,3] (channels last) -> mid float64 [T,3,Ho,Wi] (planar).  One thread per (t, oy, x): the three
// bytes of a source pixel are adjacent, a wave reads 192 contiguous bytes per tap and writes three contiguous runs.  The tables are
// tap-major ([K][Ho]); the sum runs in tap order.  mid stays float64: rounding it to float32 here would put the result up to 1.2 float32
// ulp from the float64 restatement after the second pass, a float64 intermediate keeps it at one rounding.
__global__ __launch_bounds__(PB) void k_prep_resize_v(const unsigned char* __restrict__ in, const int* __restrict__ idx,
                                                      const double* __restrict__ w, int K, long n, int Hi, int Wi, int Ho,
                                                      double* __restrict__ mid) {
  const long plane = (long)Ho * Wi;
  for (long i = (long)blockIdx.x * PB + threadIdx.x; i < n; i += (long)gridDim.x * PB) {
    const long t = i / plane;
    const long rem = i - t * plane;
    const int oy = (int)(rem / Wi), x = (int)(rem - (long)oy * Wi);
    const unsigned char* src = in + (t * Hi * Wi + x) * 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = 0; k < K; ++k) {
      const double wk = w[(long)k * Ho + oy];
      const unsigned char* p = src + (long)idx[(long)k * Ho + oy] * Wi * 3;
      a0 += wk * (double)p[0]; a1 += wk * (double)p[1]; a2 += wk * (double)p[2];
    }
    double* o = mid + t * 3 * plane + rem;
    o[0] = a0; o[plane] = a1; o[2 * plane] = a2;
  }
}

// Horizontal pass: mid float64 [R,Wi] (R = T * 3 * Ho rows) -> out float32 [R,Wo], one thread per output, one rounding.  Tables tap-major [K][Wo].
__global__ __launch_bounds__(PB) void k_prep_resize_h(const double* __restrict__ mid, const int* __restrict__ idx, const double* __restrict__ w,
                                                      int K, long n, int Wi, int Wo, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * PB + threadIdx.x; i < n; i += (long)gridDim.x * PB) {
    const long row = i / Wo;
    const int ox = (int)(i - row * Wo);
    const double* src = mid + row * Wi;
    double a = 0.0;
    for (int k = 0; k < K; ++k) a += w[(long)k * Wo + ox] * src[idx[(long)k * Wo + ox]];
    out[i] = (float)a;
  }
}

// Ground truth at the picked pixels (load_clip of harness/scannetpp.py, step for step).  One thread per output pixel (t, oy, ox) reads source
// pixel (row_idx[oy], col_idx[ox]) of frame t.  cam: 20 doubles per frame = fx, fy, cx, cy, M33 row-major, t3 (+ 4 unused).  Every float32 step
// of the host is one float32 operation here (__f*_rn: no fusing); the float64 expression (u - cx) * depth / fx has no sum to fuse into.
// depth_f64 (UG_PREP_DEPTH_F64, harness/rgbd.py's Bonn layout): the depth stays float64 from the division to the end of the back-projection
// and x, y, z are rounded once each; the mask still tests the float32 z, as the host does on -cam_coord[2].
struct PrepGtArgs {
  const unsigned short* depth;   // [T,Hi,Wi]
  const unsigned char* normals;  // [T,Hi,Wi,3] or NULL (normals 0)
  const double* cam;             // [T,20]
  const int* row_idx;            // [Ho]
  const int* col_idx;            // [Wo]
  float* cam_normal;             // [T,3,Ho,Wo] or NULL
  float* world_normal;           // [T,3,Ho,Wo] or NULL
  float* cam_coord;              // [T,3,Ho,Wo]
  float* world_coord;            // [T,3,Ho,Wo]
  float* mask;                   // [T,Ho,Wo]
  long n;                        // T * Ho * Wo
  int Hi, Wi, Ho, Wo;
  int zoomed;                    // UG_PREP_ZOOMED: the host's order-0 zoom ran, whose sum 0 + 1 * v turns a -0 into +0
  int depth_f64;                 // UG_PREP_DEPTH_F64
  float divisor, max_depth;
};

__global__ __launch_bounds__(PB) void k_prep_gt(const PrepGtArgs a) {
  const long plane = (long)a.Ho * a.Wo;
  for (long i = (long)blockIdx.x * PB + threadIdx.x; i < a.n; i += (long)gridDim.x * PB) {
    const long t = i / plane;
    const long rem = i - t * plane;
    const int oy = (int)(rem / a.Wo), ox = (int)(rem - (long)oy * a.Wo);
    const int sy = a.row_idx[oy], sx = a.col_idx[ox];
    const long sp = (t * a.Hi + sy) * a.Wi + sx;
    const double* q = a.cam + t * 20;
    const PrepPoint pt = prep_point(a.depth[sp], sx, sy, q, a.divisor, a.max_depth, a.depth_f64);      // shared with the normal fit (gt_normals.hip)
    float c[3] = {pt.c[0], pt.c[1], pt.c[2]};
    float nn[3] = {0.f, 0.f, 0.f};
    if (a.normals) {
      const unsigned char* p = a.normals + sp * 3;
      if (p[0] | p[1] | p[2])
        for (int j = 0; j < 3; ++j) nn[j] = __fsub_rn(__fmul_rn(__fdiv_rn((float)p[j], 255.f), 2.f), 1.f);
    }
    float wn[3], wc[3];
    for (int r = 0; r < 3; ++r) {
      const double* m = q + 4 + r * 3;
      wn[r] = (float)(m[0] * (double)nn[0] + m[1] * (double)nn[1] + m[2] * (double)nn[2]);
      wc[r] = (float)(m[0] * (double)c[0] + m[1] * (double)c[1] + m[2] * (double)c[2] + q[13 + r]);
    }
    const bool bad = pt.bad;
    if (a.zoomed)
      for (int j = 0; j < 3; ++j) { nn[j] = __fadd_rn(nn[j], 0.f); wn[j] = __fadd_rn(wn[j], 0.f); c[j] = __fadd_rn(c[j], 0.f); wc[j] = __fadd_rn(wc[j], 0.f); }
    const long o = t * 3 * plane + rem;
    for (int j = 0; j < 3; ++j) {
      if (a.cam_normal) a.cam_normal[o + j * plane] = bad ? 0.f : nn[j];
      if (a.world_normal) a.world_normal[o + j * plane] = bad ? 0.f : wn[j];
      a.cam_coord[o + j * plane] = bad ? 0.f : c[j];
      a.world_coord[o + j * plane] = bad ? 0.f : wc[j];
    }
    a.mask[i] = bad ? 0.f : 1.f;
  }
}

static int prep_blocks(long n) { long b = (n + PB - 1) / PB; return (int)(b > PMAXB ? PMAXB : (b < 1 ? 1 : b)); }

// frames: [T,Hi,Wi,3] bytes; row tables [Kr][Ho], column tables [Kc][Wo] (tap-major); mid: T*3*Ho*Wi doubles of scratch; out: [T,3,Ho,Wo]
void launch_prep_resize(const unsigned char* frames, const int* ridx, const double* rw, int Kr, const int* cidx, const double* cw, int Kc,
                        int T, int Hi, int Wi, int Ho, int Wo, double* mid, float* out, hipStream_t s) {
  const long nv = (long)T * Ho * Wi, nh = (long)T * 3 * Ho * Wo;
  hipLaunchKernelGGL(k_prep_resize_v, dim3(prep_blocks(nv)), dim3(PB), 0, s, frames, ridx, rw, Kr, nv, Hi, Wi, Ho, mid);
  hipLaunchKernelGGL(k_prep_resize_h, dim3(prep_blocks(nh)), dim3(PB), 0, s, (const double*)mid, cidx, cw, Kc, nh, Wi, Wo, out);
}

void launch_prep_gt(const unsigned short* depth, const unsigned char* normals, const double* cam, const int* row_idx, const int* col_idx, int T,
                    int Hi, int Wi, int Ho, int Wo, float divisor, float max_depth, int depth_f64, int zoomed, float* cam_normal, float* world_normal,
                    float* cam_coord, float* world_coord, float* mask, hipStream_t s) {
  PrepGtArgs a;
  a.depth = depth; a.normals = normals; a.cam = cam; a.row_idx = row_idx; a.col_idx = col_idx;
  a.cam_normal = cam_normal; a.world_normal = world_normal; a.cam_coord = cam_coord; a.world_coord = world_coord; a.mask = mask;
  a.n = (long)T * Ho * Wo; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.zoomed = zoomed; a.depth_f64 = depth_f64; a.divisor = divisor; a.max_depth = max_depth;
  hipLaunchKernelGGL(k_prep_gt, dim3(prep_blocks(a.n)), dim3(PB), 0, s, a);
}
