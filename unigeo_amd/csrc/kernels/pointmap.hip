// Focal, camera poses and depth from world point maps on the device - what the reference's point-map plugins take from
// solve_depth_and_camera_from_3d_points (/root/reference/metrics/utils.py:68-160): the Weiszfeld focal of estimate_focal_knowing_depth in float64,
// and, in place of cv2.solvePnPRansac, the orthogonal (object-space) iteration of Lu, Hager and Mjolsness with a trim at a reprojection threshold.
// The arithmetic is that of the numpy mirror harness/pointmap.py, operation by operation: unfused fp64 (fp contract off), and every sum as
// per-block partials - thread t of block b adds the pixels b * 256 + t + j * gridDim * 256 for ascending j, the 256 threads are folded by halves
// in LDS - that the caller adds in block order.  No atomics, no cooperative launch, no inline assembly: the result does not depend on the
// order in which workgroups arrive.  The 3x3 inverse and the SVD of every iteration are done on the host (pcd_host.h).
#include "../common.h"
#include "eval_reduce.h"

#pragma clang fp contract(off)

__device__ __forceinline__ void pm_pixel(const PmCam& cam, long i, double& col, double& row) {
  const long r = i / cam.W;
  col = (double)(i - r * cam.W); row = (double)r;
}
// unit ray of pixel i: normalize(K^-1 (col, row, 1))
__device__ __forceinline__ void pm_ray(const PmCam& cam, long i, double* b) {
  double col, row;
  pm_pixel(cam, i, col, row);
  const double dx = (col - cam.cx) / cam.f, dy = (row - cam.cy) / cam.f;
  const double nrm = __dsqrt_rn((dx * dx + dy * dy) + 1.0);
  b[0] = dx / nrm; b[1] = dy / nrm; b[2] = 1.0 / nrm;
}
__device__ __forceinline__ void pm_load(const float* pts, long i, double* X) {
  X[0] = pts[i * 3]; X[1] = pts[i * 3 + 1]; X[2] = pts[i * 3 + 2];
}
__device__ __forceinline__ void pm_rot(const double* R, const double* X, double* p) {      // (r0 x + r1 y) + r2 z per coordinate
  for (int r = 0; r < 3; ++r) p[r] = (R[r * 3] * X[0] + R[r * 3 + 1] * X[1]) + R[r * 3 + 2] * X[2];
}
__device__ __forceinline__ double pm_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ------------------------------------------------------------------------------------------------------------- focal
// INIT: partials of sum xy.px and sum xy.xy (the closed-form start); otherwise the same two weighted by w = 1 / max(|px - f xy|, 1e-8).
// xy = (x / z, y / z) with a non-finite quotient set to 0.
template <bool INIT>
__global__ __launch_bounds__(EVAL_NT) void k_pm_focal_pass(const float* pts, long n, PmCam cam, const double* fz, double* part) {
  __shared__ double sh[EVAL_NT];
  const double f = INIT ? 0.0 : fz[0];
  double acc[2] = {0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    double X[3], col, row;
    pm_load(pts, i, X);
    pm_pixel(cam, i, col, row);
    const double u = col - cam.cx, v = row - cam.cy;
    double a = X[0] / X[2], b = X[1] / X[2];
    if (!isfinite(a)) a = 0.0;
    if (!isfinite(b)) b = 0.0;
    const double dpx = a * u + b * v, dxx = a * a + b * b;
    if (INIT) { acc[0] += dpx; acc[1] += dxx; }
    else {
      const double du = u - f * a, dv = v - f * b;
      const double dis = __dsqrt_rn(du * du + dv * dv);
      const double w = 1.0 / (dis > 1e-8 ? dis : 1e-8);
      acc[0] += w * dpx; acc[1] += w * dxx;
    }
  }
  eval_store_sums<2>(acc, sh, part);
}
// one workgroup: the partials added in block order by one thread, the next focal = mean / mean
__global__ __launch_bounds__(EVAL_NT) void k_pm_focal_reduce(const double* part, int nb, double npix, double* fz) {
  __shared__ double sh[EVAL_MAXB * 2];
  for (int i = threadIdx.x; i < nb * 2; i += EVAL_NT) sh[i] = part[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double a[2] = {0, 0};
    for (int b = 0; b < nb; ++b) { a[0] += sh[b * 2]; a[1] += sh[b * 2 + 1]; }
    fz[0] = (a[0] / npix) / (a[1] / npix);
  }
}

// ------------------------------------------------------------------------------------------------------------- poses
__global__ __launch_bounds__(EVAL_NT) void k_pm_valid(const float* pts, const unsigned char* mask, long n, unsigned char* valid) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const bool fin = isfinite(pts[i * 3]) && isfinite(pts[i * 3 + 1]) && isfinite(pts[i * 3 + 2]);
    valid[i] = fin && (!mask || mask[i] > 0);
  }
}

__global__ __launch_bounds__(EVAL_NT) void k_pm_pass0(const float* pts, const unsigned char* keep, long n, PmCam cam, double* part) {
  __shared__ double sh[EVAL_NT];
  double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    if (!keep[i]) continue;
    double X[3], b[3];
    pm_load(pts, i, X);
    pm_ray(cam, i, b);
    a[0] += 1.0;
    a[1] += b[0] * b[0]; a[2] += b[0] * b[1]; a[3] += b[0] * b[2]; a[4] += b[1] * b[1]; a[5] += b[1] * b[2]; a[6] += b[2] * b[2];
    a[7] += pm_dot(X, X);
  }
  eval_store_sums<8>(a, sh, part);
}

__global__ __launch_bounds__(EVAL_NT) void k_pm_pass1(const float* pts, const unsigned char* keep, long n, PmCam cam, PmPose pose, double* part) {
  __shared__ double sh[EVAL_NT];
  double a[3] = {0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    if (!keep[i]) continue;
    double X[3], b[3], p[3];
    pm_load(pts, i, X);
    pm_ray(cam, i, b);
    pm_rot(pose.R, X, p);
    const double bp = pm_dot(b, p);
    for (int r = 0; r < 3; ++r) a[r] += b[r] * bp - p[r];
  }
  eval_store_sums<3>(a, sh, part);
}

__global__ __launch_bounds__(EVAL_NT) void k_pm_pass2(const float* pts, const unsigned char* keep, long n, PmCam cam, PmPose pose, double* part) {
  __shared__ double sh[EVAL_NT];
  double a[17];
  for (int k = 0; k < 17; ++k) a[k] = 0;
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    if (!keep[i]) continue;
    double X[3], b[3], c[3], q[3], d[3];
    pm_load(pts, i, X);
    pm_ray(cam, i, b);
    pm_rot(pose.R, X, c);
    for (int r = 0; r < 3; ++r) c[r] = c[r] + pose.t[r];
    const double bc = pm_dot(b, c);
    for (int r = 0; r < 3; ++r) { q[r] = b[r] * bc; d[r] = c[r] - q[r]; }
    a[0] += 1.0;
    for (int r = 0; r < 3; ++r) { a[1 + r] += X[r]; a[4 + r] += q[r]; }
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) a[7 + r * 3 + k] += q[r] * X[k];
    a[16] += (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  }
  eval_store_sums<17>(a, sh, part);
}

__global__ __launch_bounds__(EVAL_NT) void k_pm_inliers(const float* pts, const unsigned char* valid, const unsigned char* keep, long n, PmCam cam,
                                                    PmPose pose, double thr2, unsigned char* keep_new, double* part) {
  __shared__ double sh[EVAL_NT];
  double a[3] = {0, 0, 0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    bool in = false;
    double e2 = 0.0;
    if (valid[i]) {
      double X[3], c[3], col, row;
      pm_load(pts, i, X);
      pm_pixel(cam, i, col, row);
      pm_rot(pose.R, X, c);
      for (int r = 0; r < 3; ++r) c[r] = c[r] + pose.t[r];
      const double du = (cam.f * (c[0] / c[2]) + cam.cx) - col, dv = (cam.f * (c[1] / c[2]) + cam.cy) - row;
      e2 = du * du + dv * dv;
      in = c[2] > 0.0 && e2 <= thr2;
    }
    keep_new[i] = in;
    if (in) { a[0] += 1.0; a[2] += e2; }
    if (in != (keep[i] != 0)) a[1] += 1.0;
  }
  eval_store_sums<3>(a, sh, part);
}

__global__ __launch_bounds__(EVAL_NT) void k_pm_depth(const float* pts, const unsigned char* valid, long n, PmPose pose, float* depth) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    float z = 0.f;
    if (valid[i]) {
      double X[3];
      pm_load(pts, i, X);
      z = (float)(((pose.R[6] * X[0] + pose.R[7] * X[1]) + pose.R[8] * X[2]) + pose.t[2]);
    }
    depth[i] = z;
  }
}

// ------------------------------------------------------------------------------------------------------------- launchers
void launch_pm_focal(const float* pts, long n, PmCam cam, int steps, double* part, double* fz, hipStream_t s) {
  const int nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_pm_focal_pass<true>, dim3(nb), dim3(EVAL_NT), 0, s, pts, n, cam, (const double*)fz, part);
  hipLaunchKernelGGL(k_pm_focal_reduce, dim3(1), dim3(EVAL_NT), 0, s, (const double*)part, nb, (double)n, fz);
  for (int it = 0; it < steps; ++it) {
    hipLaunchKernelGGL(k_pm_focal_pass<false>, dim3(nb), dim3(EVAL_NT), 0, s, pts, n, cam, (const double*)fz, part);
    hipLaunchKernelGGL(k_pm_focal_reduce, dim3(1), dim3(EVAL_NT), 0, s, (const double*)part, nb, (double)n, fz);
  }
}
void launch_pm_valid(const float* pts, const unsigned char* mask, long n, unsigned char* valid, hipStream_t s) {
  hipLaunchKernelGGL(k_pm_valid, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, pts, mask, n, valid);
}
void launch_pm_pass0(const float* pts, const unsigned char* keep, long n, PmCam cam, double* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_pm_pass0, dim3(*nb), dim3(EVAL_NT), 0, s, pts, keep, n, cam, part);
}
void launch_pm_pass1(const float* pts, const unsigned char* keep, long n, PmCam cam, PmPose pose, double* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_pm_pass1, dim3(*nb), dim3(EVAL_NT), 0, s, pts, keep, n, cam, pose, part);
}
void launch_pm_pass2(const float* pts, const unsigned char* keep, long n, PmCam cam, PmPose pose, double* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_pm_pass2, dim3(*nb), dim3(EVAL_NT), 0, s, pts, keep, n, cam, pose, part);
}
void launch_pm_inliers(const float* pts, const unsigned char* valid, const unsigned char* keep, long n, PmCam cam, PmPose pose, double thr2,
                       unsigned char* keep_new, double* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_pm_inliers, dim3(*nb), dim3(EVAL_NT), 0, s, pts, valid, keep, n, cam, pose, thr2, keep_new, part);
}
void launch_pm_depth(const float* pts, const unsigned char* valid, long n, PmPose pose, float* depth, hipStream_t s) {
  hipLaunchKernelGGL(k_pm_depth, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, pts, valid, n, pose, depth);
}
