// ScanNet++ mesh renderer on the device: depth, normals and the triangle index of a triangle mesh seen from T pinhole
// cameras, which the reference makes once, offline, through pyrender, OpenGL and two GLSL shaders
// (dataset/scannetpp/preprocess_scannetpp_imu.py:470-497).  2-D homogeneous rasterisation in float64: per triangle the three edge planes
// c_k through the camera centre and the determinant D; per pixel three dot products with the pixel's ray, their sum, one division.  A pixel
// keeps the triangle of smallest fl32(z), equal depths the smaller index, with ONE 64-bit integer atomicMin per covered pixel on
// (reg_key(fl32(z)) << 32) | index: the result does not depend on the order in which the threads arrive - no floating-point atomic, no lock,
// equal bytes from run to run.  Every double step is one IEEE operation in the order include/unigeo_hip.h documents, which is the order
// harness/render.py's render_mesh evaluates on the host; the pragma below keeps a product and a sum from being contracted into an FMA.
// Work: k_rnd_splat owns one (frame, triangle) pair per thread, sets the triangle up and walks its screen box itself when the box holds at most
// RND_SMALL pixels; a larger box is cut into tiles of whole rows, about RND_TILE pixels each, appended to a list, and k_rnd_big walks one
// tile per workgroup in the next launch (the setup is recomputed there: the same operations, the same values).  When the list is full the
// owning thread walks the box after all, so its capacity is a matter of speed alone.  k_rnd_resolve, a launch of its own (the kernel
// boundary orders the atomics before its reads), turns the winner into depth, normal and index.
// Addresses: a box is clamped to 0 <= row < H, 0 <= col < W before it is walked, so t * H * W + row * W + col stays inside frame t; face
// indices have been checked against NV by the caller; a list slot is written only below the capacity.
#include "../common.h"
#include "zkey.h"

#pragma clang fp contract(off)

#define NB 256          // threads per block
#define NMAXB 4096      // grid cap; the loops below stride over the rest
#define RND_SMALL 32    // a box of at most this many pixels is walked by the thread that owns the triangle
#define RND_TILE 4096   // pixels of one tile of a larger box, in whole rows: one workgroup's share

#define RND_EMPTY 0xffffffffffffffffull

struct RndTri { double c[3][3]; double D; };

__device__ __forceinline__ void rnd_corner(const float* __restrict__ v, const double* __restrict__ m, double p[3]) {
  const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
  p[0] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
  p[1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  p[2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}
__device__ __forceinline__ void rnd_cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// the world normal (v1 - v0) x (v2 - v0) and its squared length; false: the triangle is skipped
__device__ __forceinline__ bool rnd_world_normal(const float* __restrict__ v0, const float* __restrict__ v1, const float* __restrict__ v2, double n[3],
                                                 double* l2) {
  double a[3], b[3];
  for (int j = 0; j < 3; ++j) { a[j] = (double)v1[j] - (double)v0[j]; b[j] = (double)v2[j] - (double)v0[j]; }
  rnd_cross(a, b, n);
  *l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  return *l2 > 0.0 && *l2 < INFINITY;
}

// Sets triangle `tri` up for the camera `cam` (16 doubles) and gives its screen box [r0, r1) x [c0, c1).  false: nothing to walk - a skipped
// triangle, one whose corners all lie before znear or all beyond zfar (the depth of a covered pixel is a convex combination of the corners';
// the factors leave the rounding of z room), or an empty box.  The box: with all three corners in front of the camera the pixel centres
// between the smallest and the largest projected coordinate, one more pixel each way; the whole frame otherwise.
__device__ __forceinline__ bool rnd_prepare(const float* __restrict__ verts, const int* __restrict__ faces, long tri, const double* __restrict__ cam,
                                            int H, int W, double znear, double zfar, RndTri& s, int& r0, int& r1, int& c0, int& c1) {
  const float* v0 = verts + 3l * faces[3 * tri];
  const float* v1 = verts + 3l * faces[3 * tri + 1];
  const float* v2 = verts + 3l * faces[3 * tri + 2];
  double n[3], l2;
  if (!rnd_world_normal(v0, v1, v2, n, &l2)) return false;
  double p[3][3];
  rnd_corner(v0, cam, p[0]); rnd_corner(v1, cam, p[1]); rnd_corner(v2, cam, p[2]);
  const double zmin = fmin(fmin(p[0][2], p[1][2]), p[2][2]), zmax = fmax(fmax(p[0][2], p[1][2]), p[2][2]);
  if (!(zmax >= znear * 0.999999 && zmin <= zfar * 1.000001)) return false;
  rnd_cross(p[1], p[2], s.c[0]); rnd_cross(p[2], p[0], s.c[1]); rnd_cross(p[0], p[1], s.c[2]);
  s.D = (p[0][0] * s.c[0][0] + p[0][1] * s.c[0][1]) + p[0][2] * s.c[0][2];
  r0 = 0; r1 = H; c0 = 0; c1 = W;
  if (zmin > 0.0) {
    const double fx = cam[12], fy = cam[13], cx = cam[14], cy = cam[15];
    double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
    for (int i = 0; i < 3; ++i) {
      const double u = (p[i][0] / p[i][2]) * fx + cx, v = (p[i][1] / p[i][2]) * fy + cy;
      ulo = fmin(ulo, u); uhi = fmax(uhi, u); vlo = fmin(vlo, v); vhi = fmax(vhi, v);
    }
    if (ulo > -1e9 && uhi < 1e9 && vlo > -1e9 && vhi < 1e9) {      // else (overflow, NaN): the whole frame
      c0 = (int)fmax(0.0, floor(ulo - 0.5) - 1.0); c1 = (int)fmin((double)W, floor(uhi - 0.5) + 2.0);
      r0 = (int)fmax(0.0, floor(vlo - 0.5) - 1.0); r1 = (int)fmin((double)H, floor(vhi - 0.5) + 2.0);
    }
  }
  return r1 > r0 && c1 > c0;
}

// rows of one tile of a box that is `w` pixels wide
__device__ __forceinline__ int rnd_tile_rows(int w) { const int r = RND_TILE / w; return r < 1 ? 1 : r; }

// one pixel against one triangle: the definition's ray, edges, den, coverage, z; zrow = the z-buffer at frame t, row `row`
__device__ __forceinline__ void rnd_pixel(const RndTri& s, const double* __restrict__ cam, double znear, double zfar, int row, int col, unsigned tri,
                                          unsigned long long* __restrict__ zrow) {
  const double rx = (((double)col + 0.5) - cam[14]) / cam[12];
  const double ry = (((double)row + 0.5) - cam[15]) / cam[13];
  const double e0 = (rx * s.c[0][0] + ry * s.c[0][1]) + s.c[0][2];
  const double e1 = (rx * s.c[1][0] + ry * s.c[1][1]) + s.c[1][2];
  const double e2 = (rx * s.c[2][0] + ry * s.c[2][1]) + s.c[2][2];
  const double den = (e0 + e1) + e2;
  if (!(den != 0.0)) return;
  if (!((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0))) return;      // a NaN edge fails both
  const double z = s.D / den;
  if (!(z >= znear && z <= zfar)) return;
  atomicMin(&zrow[col], ((unsigned long long)reg_key(__double2float_rn(z)) << 32) | (unsigned long long)tri);
}

__global__ __launch_bounds__(NB) void k_rnd_fill(unsigned long long* __restrict__ zbuf, long n, unsigned long long* __restrict__ big_count) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *big_count = 0ull;
  for (long i = (long)blockIdx.x * NB + threadIdx.x; i < n; i += (long)gridDim.x * NB) zbuf[i] = RND_EMPTY;
}

__global__ __launch_bounds__(NB) void k_rnd_splat(const float* __restrict__ verts, const int* __restrict__ faces, long NF, const double* __restrict__ cams,
                                                  int T, int H, int W, double znear, double zfar, unsigned long long* __restrict__ zbuf,
                                                  long long* __restrict__ big_id, int* __restrict__ big_tile, unsigned long long* __restrict__ big_count,
                                                  unsigned big_cap) {
  const long items = (long)T * NF, plane = (long)H * W;
  for (long i = (long)blockIdx.x * NB + threadIdx.x; i < items; i += (long)gridDim.x * NB) {
    const long t = i / NF, tri = i - t * NF;
    const double* cam = cams + t * 16;
    RndTri s; int r0, r1, c0, c1;
    if (!rnd_prepare(verts, faces, tri, cam, H, W, znear, zfar, s, r0, r1, c0, c1)) continue;
    if ((long)(r1 - r0) * (c1 - c0) > RND_SMALL) {
      const int rows = rnd_tile_rows(c1 - c0);
      const unsigned long long nt = (unsigned long long)((r1 - r0 + rows - 1) / rows);
      const unsigned long long slot = atomicAdd(big_count, nt);
      if (slot + nt <= (unsigned long long)big_cap) {
        for (unsigned long long k = 0; k < nt; ++k) { big_id[slot + k] = (long long)i; big_tile[slot + k] = (int)k; }
        continue;
      }
      for (unsigned long long k = slot; k < (unsigned long long)big_cap; ++k) big_id[k] = -1;      // the one range that crosses the end of the list
    }
    for (int row = r0; row < r1; ++row) {
      unsigned long long* zrow = zbuf + t * plane + (long)row * W;
      for (int col = c0; col < c1; ++col) rnd_pixel(s, cam, znear, zfar, row, col, (unsigned)tri, zrow);
    }
  }
}

// one workgroup per list entry: a tile of whole rows of one (frame, triangle) pair's box
__global__ __launch_bounds__(NB) void k_rnd_big(const float* __restrict__ verts, const int* __restrict__ faces, long NF, const double* __restrict__ cams,
                                                int H, int W, double znear, double zfar, unsigned long long* __restrict__ zbuf,
                                                const long long* __restrict__ big_id, const int* __restrict__ big_tile,
                                                const unsigned long long* __restrict__ big_count, unsigned big_cap) {
  const unsigned long long cnt = *big_count;
  const unsigned n = cnt < (unsigned long long)big_cap ? (unsigned)cnt : big_cap;
  const long plane = (long)H * W;
  for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
    const long long i = big_id[e];
    if (i < 0) continue;
    const long t = i / NF, tri = i - t * NF;
    const double* cam = cams + t * 16;
    RndTri s; int r0, r1, c0, c1;
    if (!rnd_prepare(verts, faces, tri, cam, H, W, znear, zfar, s, r0, r1, c0, c1)) continue;
    const int w = c1 - c0, rows = rnd_tile_rows(w);
    const int a = r0 + big_tile[e] * rows, b = min(r1, a + rows);
    const int npix = (b - a) * w;
    for (int p = threadIdx.x; p < npix; p += NB) {
      const int row = a + p / w, col = c0 + p % w;
      rnd_pixel(s, cam, znear, zfar, row, col, (unsigned)tri, zbuf + t * plane + (long)row * W);
    }
  }
}

// the winner of every pixel -> depth_mm, the twice-encoded normal, the triangle index
__global__ __launch_bounds__(NB) void k_rnd_resolve(const float* __restrict__ verts, const int* __restrict__ faces, const double* __restrict__ cams, long n,
                                                    long plane, const unsigned long long* __restrict__ zbuf, const unsigned char* __restrict__ mask,
                                                    unsigned short* __restrict__ depth, unsigned char* __restrict__ normal, int* __restrict__ tri_out) {
  for (long i = (long)blockIdx.x * NB + threadIdx.x; i < n; i += (long)gridDim.x * NB) {
    const unsigned long long key = zbuf[i];
    if (key == RND_EMPTY) {
      depth[i] = 0; normal[3 * i] = 0; normal[3 * i + 1] = 0; normal[3 * i + 2] = 0;
      if (tri_out) tri_out[i] = -1;
      continue;
    }
    const long tri = (long)(unsigned)(key & 0xffffffffull);
    const float z32 = reg_unkey((unsigned)(key >> 32));
    const unsigned short mm = (unsigned short)(int)__fmul_rn(z32, 1000.f);      // zfar <= 65.535: below 65536
    depth[i] = (mask && mask[i] < 255) ? (unsigned short)0 : mm;
    if (tri_out) tri_out[i] = (int)tri;
    const double* cam = cams + (i / plane) * 16;
    const float* v0 = verts + 3l * faces[3 * tri];
    const float* v1 = verts + 3l * faces[3 * tri + 1];
    const float* v2 = verts + 3l * faces[3 * tri + 2];
    double nw[3], l2, p0[3], p1[3], p2[3], c[3];
    rnd_world_normal(v0, v1, v2, nw, &l2);
    rnd_corner(v0, cam, p0); rnd_corner(v1, cam, p1); rnd_corner(v2, cam, p2);
    rnd_cross(p1, p2, c);
    const double D = (p0[0] * c[0] + p0[1] * c[1]) + p0[2] * c[2];
    const double len = sqrt(l2);
    double m[3];
    for (int j = 0; j < 3; ++j) {
      double u = nw[j] / len;
      if (D > 0.0) u = -u;
      const double q = floor(255.0 * (0.5 * u + 0.5) + 0.5);
      m[j] = (q / 255.0) * 2.0 - 1.0;
    }
    for (int j = 0; j < 3; ++j) {
      double g = (cam[4 * j] * m[0] + cam[4 * j + 1] * m[1]) + cam[4 * j + 2] * m[2];
      if (j) g = -g;
      const double e = trunc(((g + 1.0) / 2.0) * 255.0);
      normal[3 * i + j] = (unsigned char)(e >= 255.0 ? 255 : (e >= 0.0 ? (int)e : 0));      // a NaN gives 0
    }
  }
}

static int rnd_blocks(long n) { long b = (n + NB - 1) / NB; return (int)(b > NMAXB ? NMAXB : (b < 1 ? 1 : b)); }

void launch_render_mesh(const float* verts, const int* faces, long NF, const double* cams, int T, int H, int W, double znear, double zfar,
                        const unsigned char* mask, const RenderBufs& b, hipStream_t s) {
  const long n = (long)T * H * W;
  unsigned long long* cnt = b.big_count;
  hipLaunchKernelGGL(k_rnd_fill, dim3(rnd_blocks(n)), dim3(NB), 0, s, b.zbuf, n, cnt);
  hipLaunchKernelGGL(k_rnd_splat, dim3(rnd_blocks((long)T * NF)), dim3(NB), 0, s, verts, faces, NF, cams, T, H, W, znear, zfar, b.zbuf, b.big_id,
                     b.big_tile, cnt, b.big_cap);
  hipLaunchKernelGGL(k_rnd_big, dim3(b.big_cap < NMAXB ? (b.big_cap ? b.big_cap : 1) : NMAXB), dim3(NB), 0, s, verts, faces, NF, cams, H, W, znear,
                     zfar, b.zbuf, (const long long*)b.big_id, (const int*)b.big_tile, (const unsigned long long*)cnt, b.big_cap);
  hipLaunchKernelGGL(k_rnd_resolve, dim3(rnd_blocks(n)), dim3(NB), 0, s, verts, faces, cams, n, (long)H * W, (const unsigned long long*)b.zbuf, mask,
                     b.depth, b.normal, b.tri);
}
