// The loaders' back-projection of ONE depth pixel, shared by k_prep_gt (prep.hip) and k_prep_gt_normals (gt_normals.hip) so that the points the
// normal fit sums are the bits of the loader's cam_coord and its validity test is the loader's `bad` rule (include/unigeo_hip.h, ug_prep_gt /
// ug_prep_gt_ex).  q: the frame's camera table, fx, fy, cx, cy in q[0..3].  The float64 expression (u - cx) * depth / fx has no sum a product
// could be contracted into, so the function gives the same bits with and without `#pragma clang fp contract(off)` in the including file.
#pragma once

struct PrepPoint {
  float c[3];   // cam_coord = (x, -y, -d), OpenGL; NOT zeroed where bad
  bool bad;     // isnan(x) | isnan(y) | isnan(d) | d < 1e-3f | d > max_depth
};

__device__ __forceinline__ PrepPoint prep_point(unsigned short raw, int sx, int sy, const double* __restrict__ q, float divisor, float max_depth,
                                                int depth_f64) {
  const double dd = depth_f64 ? (double)raw / (double)divisor : (double)__fdiv_rn((float)raw, divisor);
  const float d = (float)dd;
  const float x = (float)(((double)sx - q[2]) * dd / q[0]);
  const float y = (float)(((double)sy - q[3]) * dd / q[1]);
  PrepPoint p;
  p.c[0] = x; p.c[1] = -y; p.c[2] = -d;
  p.bad = x != x || y != y || d != d || d < 1e-3f || d > max_depth;
  return p;
}
