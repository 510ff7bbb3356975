// Ground-truth normals fitted from the depth at the picked pixels (include/unigeo_hip.h, ug_prep_gt_normals, has the
// definition operation by operation; harness/normals.py's fit_normals is the host mirror).  The reference has no such loader step: where its
// authors want normals on an RGB-D dataset they fit a plane to the back-projected points (get_surface_normal_np, utils/geometry_utils.py:73-134);
// this is that fit with a masked window, an edge test and a validity mask.
// One thread per picked pixel (t, oy, ox).  It walks the (2r+1)^2 NATIVE neighbours of source pixel (row_idx[oy], col_idx[ox]) in row-major
// order, back-projects each one from the uint16 depth with prep_point - the device function k_prep_gt uses, so the points are the bits of the
// loader's cam_coord and the validity test is its `bad` rule - and keeps nine float64 sums in registers.  No atomics, no LDS: the depth is two
// bytes per neighbour and neighbouring lanes read neighbouring pixels, so a wave's window rows are a few cache lines that stay resident.
// Every float64 step is one IEEE operation in the documented order; the pragma keeps a product and a sum from being contracted into an FMA.
// Addresses: a neighbour (qy, qx) is read only after 0 <= qy < Hi and 0 <= qx < Wi was tested, from frame t < T of the chunk; the centre comes
// from the tables, which the caller validated before upload; the outputs are written at the thread's own index i < n.
#include "../common.h"
#include "prep_point.h"

#pragma clang fp contract(off)

#define NB 256       // threads per block
#define NMAXB 2048   // grid cap; the loop below strides over the rest

__global__ __launch_bounds__(NB) void k_prep_gt_normals(const GtNormalsArgs a) {
  const long plane = (long)a.Ho * a.Wo;
  const int r = a.radius;
  for (long i = (long)blockIdx.x * NB + threadIdx.x; i < a.n; i += (long)gridDim.x * NB) {
    const long t = i / plane;
    const long rem = i - t * plane;
    const int oy = (int)(rem / a.Wo), ox = (int)(rem - (long)oy * a.Wo);
    const int sy = a.row_idx[oy], sx = a.col_idx[ox];
    const double* q = a.cam + t * 20;
    const unsigned short* frame = a.depth + t * (long)a.Hi * a.Wi;
    const PrepPoint pc = prep_point(frame[(long)sy * a.Wi + sx], sx, sy, q, a.divisor, a.max_depth, a.depth_f64);
    float n32[3] = {0.f, 0.f, 0.f}, w32[3] = {0.f, 0.f, 0.f};
    bool valid = false;
    if (!pc.bad) {
      const double cx = (double)pc.c[0], cy = (double)pc.c[1], cz = (double)pc.c[2];
      const double dc = -cz;
      const double lim = a.edge * dc;
      double sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0, s1x = 0.0, s1y = 0.0, s1z = 0.0;
      int cnt = 0;
      for (int dy = -r; dy <= r; ++dy) {
        const int qy = sy + dy;
        if (qy < 0 || qy >= a.Hi) continue;
        for (int dx = -r; dx <= r; ++dx) {
          const int qx = sx + dx;
          if (qx < 0 || qx >= a.Wi) continue;
          const PrepPoint p = prep_point(frame[(long)qy * a.Wi + qx], qx, qy, q, a.divisor, a.max_depth, a.depth_f64);
          if (p.bad) continue;
          const double x = (double)p.c[0], y = (double)p.c[1], z = (double)p.c[2];
          if (a.edge_on && !(fabs(-z - dc) <= lim)) continue;
          sxx += x * x; sxy += x * y; sxz += x * z; syy += y * y; syz += y * z; szz += z * z;
          s1x += x; s1y += y; s1z += z;
          ++cnt;
        }
      }
      if (cnt >= a.min_count) {
        const double c = (double)cnt;
        const double axx = sxx / c + 1e-6, axy = sxy / c, axz = sxz / c, ayy = syy / c + 1e-6, ayz = syz / c, azz = szz / c + 1e-6;
        const double bx = s1x / c, by = s1y / c, bz = s1z / c;
        const double c00 = ayy * azz - ayz * ayz, c01 = axz * ayz - axy * azz, c02 = axy * ayz - axz * ayy;
        const double c11 = axx * azz - axz * axz, c12 = axy * axz - axx * ayz, c22 = axx * ayy - axy * axy;
        const double det = (axx * c00 + axy * c01) + axz * c02;
        double n0 = ((c00 * bx + c01 * by) + c02 * bz) / det;
        double n1 = ((c01 * bx + c11 * by) + c12 * bz) / det;
        double n2 = ((c02 * bx + c12 * by) + c22 * bz) / det;
        const double den = sqrt((n0 * n0 + n1 * n1) + n2 * n2) + 1e-6;
        n0 = n0 / den; n1 = n1 / den; n2 = n2 / den;
        if ((n0 * cx + n1 * cy) + n2 * cz > 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
        if (isfinite(n0) && isfinite(n1) && isfinite(n2)) {
          valid = true;
          n32[0] = (float)n0; n32[1] = (float)n1; n32[2] = (float)n2;
          for (int k = 0; k < 3; ++k) {
            const double* m = q + 4 + k * 3;
            w32[k] = (float)((m[0] * (double)n32[0] + m[1] * (double)n32[1]) + m[2] * (double)n32[2]);
          }
          if (a.zoomed)
            for (int k = 0; k < 3; ++k) { n32[k] = __fadd_rn(n32[k], 0.f); w32[k] = __fadd_rn(w32[k], 0.f); }
        }
      }
    }
    const long o = t * 3 * plane + rem;
    for (int k = 0; k < 3; ++k) { a.cam_normal[o + k * plane] = n32[k]; a.world_normal[o + k * plane] = w32[k]; }
    a.normal_mask[i] = valid ? 1.f : 0.f;
  }
}

void launch_prep_gt_normals(const GtNormalsArgs& a, hipStream_t s) {
  long b = (a.n + NB - 1) / NB;
  b = b > NMAXB ? NMAXB : (b < 1 ? 1 : b);
  hipLaunchKernelGGL(k_prep_gt_normals, dim3((int)b), dim3(NB), 0, s, a);
}
