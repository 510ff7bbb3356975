// Host half of the point-to-point ICP of ug_eval_pcd: the 3x3 singular value decomposition as a one-sided Jacobi, the
// Umeyama rotation (no scaling) from the Kabsch sums of kernels/pcd.hip, and 4x4 products; and the shape of the search grid of section 20.  Plain
// C++ with no GPU dependency: the stand-alone test programs of tests/test_pcd_cpu.py and tests/test_pcd_grid_cpu.py compile it with the host
// compiler and sanitizers.
#pragma once
#include <math.h>

namespace pcd_host {

inline double det3(const double m[3][3]) {
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// A = U diag(w) V^T, w descending, U and V orthogonal.  One-sided Jacobi (Hestenes): plane rotations from the right make the columns of
// B = A V orthogonal; their lengths are the singular values.  Columns of U that belong to a singular value below 1e-12 of the largest are
// completed to a right-handed orthonormal basis instead of being divided out of rounding noise.
inline void svd3(const double A[3][3], double U[3][3], double w[3], double V[3][3]) {
  double B[3][3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { B[r][c] = A[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double alpha = 0, beta = 0, gamma = 0;
      for (int r = 0; r < 3; ++r) { alpha += B[r][p] * B[r][p]; beta += B[r][q] * B[r][q]; gamma += B[r][p] * B[r][q]; }
      if (gamma == 0.0 || fabs(gamma) <= 1e-17 * sqrt(alpha * beta)) continue;
      rotated = true;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
      for (int r = 0; r < 3; ++r) {
        const double bp = B[r][p], bq = B[r][q];
        B[r][p] = c * bp - s * bq; B[r][q] = s * bp + c * bq;
        const double vp = V[r][p], vq = V[r][q];
        V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  for (int j = 0; j < 3; ++j) w[j] = sqrt(B[0][j] * B[0][j] + B[1][j] * B[1][j] + B[2][j] * B[2][j]);
  for (int a = 0; a < 2; ++a)                      // selection sort of the three columns, descending
    for (int b = a + 1; b < 3; ++b)
      if (w[b] > w[a]) {
        const double tw = w[a]; w[a] = w[b]; w[b] = tw;
        for (int r = 0; r < 3; ++r) {
          const double tb = B[r][a]; B[r][a] = B[r][b]; B[r][b] = tb;
          const double tv = V[r][a]; V[r][a] = V[r][b]; V[r][b] = tv;
        }
      }
  int good = 0;
  while (good < 3 && w[good] > 0.0 && w[good] > 1e-12 * w[0]) ++good;
  for (int j = 0; j < good; ++j) for (int r = 0; r < 3; ++r) U[r][j] = B[r][j] / w[j];
  if (good == 0) { for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) U[r][c] = r == c ? 1.0 : 0.0; return; }
  if (good == 1) {      // any unit vector orthogonal to the first column: cross it with the axis it is least aligned with
    int ax = 0;
    if (fabs(U[1][0]) < fabs(U[ax][0])) ax = 1;
    if (fabs(U[2][0]) < fabs(U[ax][0])) ax = 2;
    double e[3] = {0, 0, 0}; e[ax] = 1.0;
    double v[3] = {U[1][0] * e[2] - U[2][0] * e[1], U[2][0] * e[0] - U[0][0] * e[2], U[0][0] * e[1] - U[1][0] * e[0]};
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int r = 0; r < 3; ++r) U[r][1] = v[r] / len;
  }
  if (good <= 2) {
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  }
}

// R = U diag(1, 1, sign(det U det V)) V^T: the rotation closest to H = sum d s^T (Kabsch / Umeyama)
inline void rotation_from_h(const double H[3][3], double R[3][3]) {
  double U[3][3], w[3], V[3][3];
  svd3(H, U, w, V);
  const double sg = det3(U) * det3(V) >= 0 ? 1.0 : -1.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[r][c] = U[r][0] * V[c][0] + U[r][1] * V[c][1] + sg * U[r][2] * V[c][2];
}

// a[17] = n, sum s (3), sum d (3), sum d s^T (9, row = d), sum dist^2 -> the 4x4 (row-major) that moves s onto d; identity for n < 1
inline void umeyama_from_sums(const double* a, double* T) {
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
  const double n = a[0];
  if (!(n >= 1.0)) return;
  double ms[3], md[3], H[3][3], R[3][3];
  for (int r = 0; r < 3; ++r) { ms[r] = a[1 + r] / n; md[r] = a[4 + r] / n; }
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[r][c] = a[7 + r * 3 + c] / n - md[r] * ms[c];
  rotation_from_h(H, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = R[r][c];
    T[r * 4 + 3] = md[r] - (R[r][0] * ms[0] + R[r][1] * ms[1] + R[r][2] * ms[2]);
  }
}

inline void mul44(const double* A, const double* B, double* C) {      // C = A B, row-major, C distinct from A and B
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double v = 0;
      for (int k = 0; k < 4; ++k) v += A[r * 4 + k] * B[k * 4 + c];
      C[r * 4 + c] = v;
    }
}

// The uniform search grid of DESIGN.md section 20: cell edge h and cells per axis G from the bounding box of the n_in finite points
// (box = min xyz, max xyz).  An axis is thick when its extent is at least h; over the d thick axes h solves
// n_in * h^d = occ * (product of their extents), i.e. occ points per cell for a cloud that fills its box along those axes.  Starting from the
// axes of positive extent, an axis thinner than the h it gives is dropped and h is solved again (at most three times); a cloud with no thick
// axis (one point, all points equal) gets one cell.  Cells per axis are floor(extent / h) + 1, so an extent of 0 is one cell, and h grows by
// a quarter at a time until the product respects max_cells.  No point (n_in <= 0): one cell at the origin with h = 1.
inline void grid_shape(const double* box, long n_in, double occ, long max_cells, double mn[3], double* h_out, int G[3], long* cells_out) {
  for (int a = 0; a < 3; ++a) { mn[a] = 0; G[a] = 1; }
  *h_out = 1.0; *cells_out = 1;
  if (n_in <= 0) return;
  double e[3], L = 0;
  bool thick[3];
  for (int a = 0; a < 3; ++a) {
    mn[a] = box[a];
    e[a] = box[3 + a] - box[a];
    if (!(e[a] >= 0)) e[a] = 0;
    if (!(e[a] <= 1.7e308)) e[a] = 1.7e308;      // the difference of two finite coordinates may overflow
    thick[a] = e[a] > 0;
    L = e[a] > L ? e[a] : L;
  }
  double h = 0;
  for (int pass = 0; pass < 4; ++pass) {
    int d = 0;
    double lg = log(occ / (double)n_in);
    for (int a = 0; a < 3; ++a) if (thick[a]) { ++d; lg += log(e[a]); }
    if (d == 0) { h = 0; break; }
    h = exp(lg / d);
    bool dropped = false;
    for (int a = 0; a < 3; ++a) if (thick[a] && e[a] < h) { thick[a] = false; dropped = true; }
    if (!dropped) break;
  }
  if (!(h > 0)) h = L > 0 ? 2.0 * L : 1.0;
  if (!(h >= 1e-300)) h = 1e-300;                  // 1 / h stays finite
  if (!(h <= 1e300)) h = 1e300;
  for (;;) {
    double cells = 1;
    for (int a = 0; a < 3; ++a) {
      const double c = floor(e[a] / h) + 1.0;
      G[a] = c < 16777217.0 ? (int)c : 16777217;
      cells *= (double)G[a];
    }
    if (cells <= (double)max_cells) { *cells_out = (long)cells; break; }
    h *= 1.25;
  }
  *h_out = h;
}

}  // namespace pcd_host
