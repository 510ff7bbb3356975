// Point-cloud evaluation on the device - what the reference hands to Open3D and a CPU k-d tree:
//   /root/reference/metrics/eval_pcd.py:10-168 (masked selection, alignment, downsampling, ICP, normals, scores),
//   metrics/pcd_alignment.py (Regr3D_t_ScaleShiftInv: median shifts and median scales), metrics/utils.py:14-42 (accuracy / completion),
//   and the farthest-point sampling of its disabled branch (eval_pcd.py:84-93,172-193), in unfused fp32.
// Brute-force pair arithmetic in unfused fp64 (fp contract off), the arithmetic of the numpy mirror in harness/metrics.py.  Every kernel is
// deterministic: reductions are two-stage in a fixed order, target slices are combined in slice order, the only atomics are integer
// histogram counts.  No float atomics, no cooperative launch, no inline assembly.  The exact search through a uniform grid (DESIGN.md
// section 20) finds the same neighbours without visiting every pair; its atomics are integer counts and list lengths.
#include "../common.h"
#include "../pcd_host.h"
#include "eval_reduce.h"

// No contraction anywhere in this file: every product and every sum below rounds on its own, as the numpy mirror's do.  (The __dmul_rn /
// __dadd_rn intrinsics are plain operators in this toolchain and would fuse; the pragma is what keeps a * b + c two roundings.)
#pragma clang fp contract(off)

#define NN_TILE 256     // target points staged in LDS per step
#define KNN_B 128       // threads per block of the neighbour-list kernel: 128 x 32 x 12 B of lists + the tile = 51 KiB of LDS
#define KNN_MAX 32      // = UG_PCD_MAX_KNN

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------------------- masked compaction
// Order-preserving: block b owns the contiguous pixels [b * chunk, (b + 1) * chunk); counts per block, one exclusive scan, then every block
// writes its kept pixels behind its offset, 256 at a time with a block scan of the keep flags.
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned* sc, unsigned* total) {
  const int tid = threadIdx.x;
  sc[tid] = v;
  __syncthreads();
  for (int o = 1; o < EVAL_NT; o <<= 1) {
    const unsigned a = tid >= o ? sc[tid - o] : 0u;
    __syncthreads();
    sc[tid] += a;
    __syncthreads();
  }
  const unsigned incl = sc[tid];
  *total = sc[EVAL_NT - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(EVAL_NT) void k_pcd_count(const unsigned char* mask, long n, long chunk, unsigned* counts) {
  __shared__ unsigned sc[EVAL_NT];
  const long b0 = (long)blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
  unsigned cnt = 0;
  for (long i = b0 + threadIdx.x; i < b1; i += EVAL_NT) cnt += mask[i] > 0;
  unsigned total;
  block_scan_excl(cnt, sc, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one workgroup: counts[0 .. nb) -> exclusive offsets in place, counts[EVAL_MAXB] = the total
__global__ __launch_bounds__(EVAL_NT) void k_pcd_offsets(unsigned* counts, int nb) {
  __shared__ unsigned sh[EVAL_MAXB];
  for (int i = threadIdx.x; i < nb; i += EVAL_NT) sh[i] = counts[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned acc = 0;
    for (int b = 0; b < nb; ++b) { const unsigned v = sh[b]; sh[b] = acc; acc += v; }
    counts[EVAL_MAXB] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += EVAL_NT) counts[i] = sh[i];
}

__global__ __launch_bounds__(EVAL_NT) void k_pcd_scatter(const float* pred, const float* gt, const unsigned char* mask, long n, long chunk,
                                                    const unsigned* counts, float* p_out, float* g_out) {
  __shared__ unsigned sc[EVAL_NT];
  const long b0 = (long)blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
  unsigned long base = counts[blockIdx.x];
  for (long s0 = b0; s0 < b1; s0 += EVAL_NT) {      // chunk is a multiple of EVAL_NT: every thread of the block takes every step
    const long i = s0 + threadIdx.x;
    const unsigned keep = i < b1 && mask[i] > 0;
    unsigned total;
    const unsigned pos = block_scan_excl(keep, sc, &total);
    if (keep) {
      const unsigned long o = (base + pos) * 3;
      p_out[o] = pred[i * 3]; p_out[o + 1] = pred[i * 3 + 1]; p_out[o + 2] = pred[i * 3 + 2];
      g_out[o] = gt[i * 3]; g_out[o + 1] = gt[i * 3 + 1]; g_out[o + 2] = gt[i * 3 + 2];
    }
    base += total;
  }
}

// ------------------------------------------------------------------------------------------------------------- exact k-th smallest
// Radix select over the order-preserving 64-bit key (common.h: pcd_key), 8 bits per pass from the top; a float32 key fills the upper word, so
// four passes finish it.  State in device memory (unsigned words): sel[0 .. 256) the histogram of the pass, sel[256 .. 258) the key bits fixed
// so far, sel[258 .. 260) the rank still to find inside that prefix.  Counts are integers: the result does not depend on workgroup order.
template <typename T>
__global__ __launch_bounds__(EVAL_NT) void k_pcd_sel_hist(const T* v, long n, int stride, int offset, int shift, int first, const unsigned* sel,
                                                     unsigned* hist) {
  __shared__ unsigned h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const u64 prefix = ((u64)sel[257] << 32) | sel[256];
  for (long i = (long)blockIdx.x * EVAL_NT + tid; i < n; i += (long)gridDim.x * EVAL_NT) {
    const u64 key = pcd_key(v[i * stride + offset]);
    if (first || ((key ^ prefix) >> (shift + 8)) == 0) atomicAdd(&h[(unsigned)(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (h[tid]) atomicAdd(&hist[tid], h[tid]);
}

// one workgroup: the bin that holds the wanted rank, the rank inside it; the histogram is zeroed for the next pass; the last pass stores the key
__global__ __launch_bounds__(256) void k_pcd_sel_scan(unsigned* sel, int shift, int first, int last, u64 k0, u64* res, int slot) {
  __shared__ unsigned sc[256];
  const int tid = threadIdx.x;
  const unsigned cnt = sel[tid];
  const u64 k = first ? k0 : (((u64)sel[259] << 32) | sel[258]);
  const u64 prefix0 = first ? 0ull : (((u64)sel[257] << 32) | sel[256]);
  unsigned total;
  const unsigned excl = block_scan_excl(cnt, sc, &total);      // ends with a barrier: every thread has read the rank and the prefix
  sel[tid] = 0;
  if (cnt && (u64)excl <= k && k < (u64)excl + cnt) {
    const u64 prefix = prefix0 | ((u64)tid << shift), rank = k - excl;
    sel[256] = (unsigned)prefix; sel[257] = (unsigned)(prefix >> 32);
    sel[258] = (unsigned)rank; sel[259] = (unsigned)(rank >> 32);
    if (last) res[slot] = prefix;
  }
}

// ------------------------------------------------------------------------------------------------------------- alignment
// p.z -= median(p.z), g.z -= median(g.z): float32, as the reference's in-place tensor updates
__global__ __launch_bounds__(EVAL_NT) void k_pcd_shift_z(float* p, float* g, long n, const u64* res, int slot_p, int slot_g) {
  const float pz = pcd_unkey_f32(res[slot_p]), gz = pcd_unkey_f32(res[slot_g]);
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    p[i * 3 + 2] = p[i * 3 + 2] - pz;
    g[i * 3 + 2] = g[i * 3 + 2] - gz;
  }
}
// |p - c| with the float32 differences widened: the fp64 products are exact, two sums and one square root round, then once to float32
__global__ __launch_bounds__(EVAL_NT) void k_pcd_center_norm(const float* p, long n, const u64* res, int slot_c, float* norm) {
  const float cx = pcd_unkey_f32(res[slot_c]), cy = pcd_unkey_f32(res[slot_c + 1]), cz = pcd_unkey_f32(res[slot_c + 2]);
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const float fx = p[i * 3] - cx, fy = p[i * 3 + 1] - cy, fz = p[i * 3 + 2] - cz;      // float32 differences
    const double dx = fx, dy = fy, dz = fz;
    norm[i] = (float)__dsqrt_rn((dx * dx + dy * dy) + dz * dz);
  }
}
// gather the sampled points (idx NULL: all), pred *= gt_scale / pred_scale, both z += gt_shift_z; float32 clouds and their fp64 copies (p64 and
// g64 both NULL: none)
__global__ __launch_bounds__(EVAL_NT) void k_pcd_align(const float* p, const float* g, const long* idx, long ns, float ratio, float gz, float* p32,
                                                  float* g32, double* p64, double* g64) {
  for (long j = (long)blockIdx.x * EVAL_NT + threadIdx.x; j < ns; j += (long)gridDim.x * EVAL_NT) {
    const long i = idx ? idx[j] : j;
    const float px = p[i * 3] * ratio, py = p[i * 3 + 1] * ratio, pz = p[i * 3 + 2] * ratio + gz;
    const float gx = g[i * 3], gy = g[i * 3 + 1], gzz = g[i * 3 + 2] + gz;
    p32[j * 3] = px; p32[j * 3 + 1] = py; p32[j * 3 + 2] = pz;
    g32[j * 3] = gx; g32[j * 3 + 1] = gy; g32[j * 3 + 2] = gzz;
    if (!p64) continue;      // farthest-point sampling aligns every masked point and widens only what it picks
    p64[j * 3] = px; p64[j * 3 + 1] = py; p64[j * 3 + 2] = pz;
    g64[j * 3] = gx; g64[j * 3 + 1] = gy; g64[j * 3 + 2] = gzz;
  }
}

// ------------------------------------------------------------------------------------------------------------- nearest neighbour
// ((r0 x + r1 y) + r2 z) + t per coordinate, T row-major 4x4 in device memory; NULL leaves the point alone
__device__ __forceinline__ void pcd_move(const double* T, double& x, double& y, double& z) {
  if (!T) return;
  const double a = x, b = y, c = z;
  x = ((T[0] * a + T[1] * b) + T[2] * c) + T[3];
  y = ((T[4] * a + T[5] * b) + T[6] * c) + T[7];
  z = ((T[8] * a + T[9] * b) + T[10] * c) + T[11];
}
__device__ __forceinline__ double pcd_d2(double x, double y, double z, const double* t) {
  const double dx = x - t[0], dy = y - t[1], dz = z - t[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// One query per thread; blockIdx.y owns the targets [y * slice, (y + 1) * slice), staged through LDS NN_TILE at a time and read by broadcast.
// Targets are visited in index order and only a strictly smaller squared distance replaces the best: ties stay with the lowest index.
__global__ __launch_bounds__(EVAL_NT) void k_pcd_nn(const double* q, long nq, const double* t, long nt, const double* T44, long slice, int* pidx,
                                               double* pdist) {
  __shared__ double tile[NN_TILE * 3];
  const long i = (long)blockIdx.x * EVAL_NT + threadIdx.x;
  const bool live = i < nq;
  double x = 0, y = 0, z = 0;
  if (live) { x = q[i * 3]; y = q[i * 3 + 1]; z = q[i * 3 + 2]; pcd_move(T44, x, y, z); }
  const long t0 = (long)blockIdx.y * slice, t1 = t0 + slice < nt ? t0 + slice : nt;
  double best = INFINITY;
  long bi = t0;
  for (long base = t0; base < t1; base += NN_TILE) {
    const int cnt = (int)(t1 - base < NN_TILE ? t1 - base : NN_TILE);
    for (int e = threadIdx.x; e < cnt * 3; e += EVAL_NT) tile[e] = t[base * 3 + e];
    __syncthreads();
    if (live)
      for (int j = 0; j < cnt; ++j) {
        const double d2 = pcd_d2(x, y, z, tile + j * 3);
        if (d2 < best) { best = d2; bi = base + j; }
      }
    __syncthreads();
  }
  if (live) { pdist[(long)blockIdx.y * nq + i] = best; pidx[(long)blockIdx.y * nq + i] = (int)bi; }
}
// the slices in slice order, again only a strictly smaller value wins; the distance is the square root of the winner
__global__ __launch_bounds__(EVAL_NT) void k_pcd_nn_combine(const int* pidx, const double* pdist, long nq, int ny, int* idx, double* dist) {
  const long i = (long)blockIdx.x * EVAL_NT + threadIdx.x;
  if (i >= nq) return;
  double best = pdist[i];
  int bi = pidx[i];
  for (int y = 1; y < ny; ++y) {
    const double d2 = pdist[(long)y * nq + i];
    if (d2 < best) { best = d2; bi = pidx[(long)y * nq + i]; }
  }
  idx[i] = bi; dist[i] = __dsqrt_rn(best);
}

// ------------------------------------------------------------------------------------------------------------- fixed-order reductions
// Kabsch sums over the correspondences (dist < threshold): n, sum s (3), sum d (3), sum d s^T (9, row = d), sum dist^2; s = the moved query
__global__ __launch_bounds__(EVAL_NT) void k_pcd_kabsch(const double* q, const double* t, long nq, const double* T44, const int* idx, const double* dist,
                                                   double threshold, double* part) {
  __shared__ double sh[EVAL_NT];
  double a[17];
  for (int k = 0; k < 17; ++k) a[k] = 0;
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < nq; i += (long)gridDim.x * EVAL_NT) {
    const double d = dist[i];
    if (!(d < threshold)) continue;
    double s[3] = {q[i * 3], q[i * 3 + 1], q[i * 3 + 2]};
    pcd_move(T44, s[0], s[1], s[2]);
    const double* g = t + (long)idx[i] * 3;
    a[0] += 1.0;
    for (int r = 0; r < 3; ++r) { a[1 + r] += s[r]; a[4 + r] += g[r]; }
    for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) a[7 + r * 3 + cc] += g[r] * s[cc];
    a[16] += d * d;
  }
  eval_store_sums<17>(a, sh, part);
}
__global__ __launch_bounds__(EVAL_NT) void k_pcd_sum(const double* v, long n, double* part) {
  __shared__ double sh[EVAL_NT];
  double a[1] = {0};
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) a[0] += v[i];
  eval_store_sums<1>(a, sh, part);
}
// how many v[i] lie strictly below each of the nt thresholds, one pass for all of them; a NaN is not below.  Integer
// counts per workgroup -> part[b * PCD_MAX_THRESHOLDS + k], added by the caller in block order.
__global__ __launch_bounds__(EVAL_NT) void k_pcd_count_below(const double* v, long n, PcdThresholds t, unsigned* part) {
  __shared__ unsigned sh[EVAL_NT];
  unsigned c[PCD_MAX_THRESHOLDS];
#pragma unroll
  for (int k = 0; k < PCD_MAX_THRESHOLDS; ++k) c[k] = 0u;
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const double d = v[i];
#pragma unroll
    for (int k = 0; k < PCD_MAX_THRESHOLDS; ++k) c[k] += (k < t.n && d < t.tau[k]) ? 1u : 0u;
  }
#pragma unroll
  for (int k = 0; k < PCD_MAX_THRESHOLDS; ++k) {
    const unsigned r = eval_block_count(c[k], sh);
    if (threadIdx.x == 0) part[(long)blockIdx.x * PCD_MAX_THRESHOLDS + k] = r;
  }
}
__global__ __launch_bounds__(EVAL_NT) void k_pcd_move(const double* q, long n, const double* T44, double* out) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    double x = q[i * 3], y = q[i * 3 + 1], z = q[i * 3 + 2];
    pcd_move(T44, x, y, z);
    out[i * 3] = x; out[i * 3 + 1] = y; out[i * 3 + 2] = z;
  }
}
// |n_t[idx] . n_q| per query
__global__ __launch_bounds__(EVAL_NT) void k_pcd_normal_dot(const double* nq, const double* nt, const int* idx, long n, double* dot) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const double* a = nt + (long)idx[i] * 3;
    const double* b = nq + i * 3;
    dot[i] = fabs((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
  }
}

// ------------------------------------------------------------------------------------------------------------- KNN covariance normals
// The mean and the covariance of the k listed neighbours in fp64 (list order) and the cyclic Jacobi eigen-solve with a fixed number of sweeps:
// the one copy that k_pcd_knn and k_pcd_knn_grid share, so equal lists give bit-equal normals.
__device__ __forceinline__ void pcd_list_normal(const double* pts, const int (*li)[KNN_B], int tid, int k, double* out) {
  double nx = 0, ny = 0, nz = 1;
  if (k >= 3) {
    double m[3] = {0, 0, 0};
    for (int j = 0; j < k; ++j) { const double* p = pts + (long)li[j][tid] * 3; m[0] += p[0]; m[1] += p[1]; m[2] += p[2]; }
    m[0] /= k; m[1] /= k; m[2] /= k;
    double a[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int j = 0; j < k; ++j) {
      const double* p = pts + (long)li[j][tid] * 3;
      const double d[3] = {p[0] - m[0], p[1] - m[1], p[2] - m[2]};
      for (int r = 0; r < 3; ++r) for (int c = r; c < 3; ++c) a[r][c] += d[r] * d[c];
    }
    for (int r = 0; r < 3; ++r) for (int c = r; c < 3; ++c) { a[r][c] /= k; a[c][r] = a[r][c]; }
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep)
#pragma unroll
      for (int pq = 0; pq < 3; ++pq) {      // unrolled: p and q are constants, the two matrices stay in registers
        const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        for (int r = 0; r < 3; ++r) {        // A <- A J
          const double arp = a[r][p], arq = a[r][q];
          a[r][p] = cs * arp - sn * arq; a[r][q] = sn * arp + cs * arq;
        }
        for (int r = 0; r < 3; ++r) {        // A <- J^T A,  V <- V J
          const double apr = a[p][r], aqr = a[q][r];
          a[p][r] = cs * apr - sn * aqr; a[q][r] = sn * apr + cs * aqr;
          const double vrp = v[r][p], vrq = v[r][q];
          v[r][p] = cs * vrp - sn * vrq; v[r][q] = sn * vrp + cs * vrq;
        }
      }
    double em = a[0][0], ex = v[0][0], ey = v[1][0], ez = v[2][0];      // the column of the smallest eigenvalue, without a dynamic index
    if (a[1][1] < em) { em = a[1][1]; ex = v[0][1]; ey = v[1][1]; ez = v[2][1]; }
    if (a[2][2] < em) { em = a[2][2]; ex = v[0][2]; ey = v[1][2]; ez = v[2][2]; }
    const double len = sqrt(ex * ex + ey * ey + ez * ez);
    if (len > 0) { nx = ex / len; ny = ey / len; nz = ez / len; }
  }
  out[0] = nx; out[1] = ny; out[2] = nz;
}

// One query per thread.  The running top-k list, sorted by (squared distance, index), lives in LDS in a [k][thread] layout: the threads of
// a wave touch consecutive words.  Targets arrive in index order, so an equal distance goes behind the entries already there.  Then the normal
// from the list.  `list` (or NULL with nl = n) names the points to serve: the leftovers of k_pcd_knn_grid.
__global__ __launch_bounds__(KNN_B) void k_pcd_knn(const double* pts, long n, int k, const int* list, long nl, int* nbr, double* normals) {
  __shared__ double ld[KNN_MAX][KNN_B];
  __shared__ int li[KNN_MAX][KNN_B];
  __shared__ double tile[KNN_B * 3];
  const int tid = threadIdx.x;
  const long slot = (long)blockIdx.x * KNN_B + tid;      // without a list (NULL, nl = n) slot is the point itself
  const bool live = slot < nl;
  const long i = live && list ? list[slot] : slot;
  double x = 0, y = 0, z = 0;
  if (live) { x = pts[i * 3]; y = pts[i * 3 + 1]; z = pts[i * 3 + 2]; }
  int cnt = 0;
  for (long base = 0; base < n; base += KNN_B) {
    const int tc = (int)(n - base < KNN_B ? n - base : KNN_B);
    for (int e = tid; e < tc * 3; e += KNN_B) tile[e] = pts[base * 3 + e];
    __syncthreads();
    if (live)
      for (int j = 0; j < tc; ++j) {
        const double d2 = pcd_d2(x, y, z, tile + j * 3);
        if (cnt < k || d2 < ld[cnt - 1][tid]) {
          int pos = cnt < k ? cnt++ : k - 1;
          while (pos > 0 && ld[pos - 1][tid] > d2) { ld[pos][tid] = ld[pos - 1][tid]; li[pos][tid] = li[pos - 1][tid]; --pos; }
          ld[pos][tid] = d2; li[pos][tid] = (int)(base + j);
        }
      }
    __syncthreads();
  }
  if (!live) return;
  if (nbr) for (int j = 0; j < k; ++j) nbr[i * k + j] = li[j][tid];
  pcd_list_normal(pts, li, tid, k, normals + i * 3);
}

// ------------------------------------------------------------------------------------------------------------- farthest-point sampling
// DESIGN.md section 19, the arithmetic of pcd_fps_indices in harness/metrics.py.  m[j] is the smallest squared distance of point j to the points
// picked so far (+inf before the first pick, -1 for a non-finite point); every pick is the largest m, ties to the lowest index.  One launch per
// pick: launch L (L >= 1) first reduces the (best m, lowest index) pairs that the workgroups of launch L - 1 left - every workgroup on its own, in
// the same order, so all agree on the pick s - then lowers m by the distance to p[s] over its grid-stride share and leaves its own pair.  Launch 0
// only initialises m.  The pairs are double-buffered by launch parity: launch L reads slot (L - 1) & 1 and writes slot L & 1, and the stream
// orders the launches, so no workgroup reads a word that a workgroup of its own launch writes.
__device__ __forceinline__ void fps_better(float& bm, int& bi, float m, int i) {
  if (m > bm || (m == bm && i < bi)) { bm = m; bi = i; }
}
__device__ __forceinline__ void fps_block_best(float& bm, int& bi, float* sm, int* si) {
  const int tid = threadIdx.x;
  sm[tid] = bm; si[tid] = bi;
  __syncthreads();
  for (int o = EVAL_NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      float m = sm[tid]; int i = si[tid];
      fps_better(m, i, sm[tid + o], si[tid + o]);
      sm[tid] = m; si[tid] = i;
    }
    __syncthreads();
  }
  bm = sm[0]; bi = si[0];
  __syncthreads();
}
#define FPS_NONE_M (-2.f)          // below every m (m >= -1): a thread or slot without a point never wins
#define FPS_NONE_I 0x7fffffff

__global__ __launch_bounds__(EVAL_NT) void k_pcd_fps(const float* p, long n, float* m, long launch, int nprev, int last, float* pm, int* pi, long* idx,
                                                float* sel_dist) {
  __shared__ float sm[EVAL_NT];
  __shared__ int si[EVAL_NT];
  const int tid = threadIdx.x;
  const float* pm_in = pm + ((launch & 1) ^ 1) * EVAL_MAXB; const int* pi_in = pi + ((launch & 1) ^ 1) * EVAL_MAXB;
  float* pm_out = pm + (launch & 1) * EVAL_MAXB; int* pi_out = pi + (launch & 1) * EVAL_MAXB;
  float bm = FPS_NONE_M; int bi = FPS_NONE_I;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  if (launch > 0) {
    for (int b = tid; b < nprev; b += EVAL_NT) fps_better(bm, bi, pm_in[b], pi_in[b]);
    fps_block_best(bm, bi, sm, si);
    if (blockIdx.x == 0 && tid == 0) { idx[launch - 1] = bi; sel_dist[launch - 1] = bm; }
    if (last) return;
    sx = p[(long)bi * 3]; sy = p[(long)bi * 3 + 1]; sz = p[(long)bi * 3 + 2];
    bm = FPS_NONE_M; bi = FPS_NONE_I;
  }
  for (long j = (long)blockIdx.x * EVAL_NT + tid; j < n; j += (long)gridDim.x * EVAL_NT) {      // ascending j: a strictly larger m keeps the lowest index
    const float x = p[j * 3], y = p[j * 3 + 1], z = p[j * 3 + 2];
    float mj;
    if (launch == 0) {
      mj = (isfinite(x) && isfinite(y) && isfinite(z)) ? INFINITY : -1.f;
      m[j] = mj;
    } else {
      mj = m[j];
      const float dx = x - sx, dy = y - sy, dz = z - sz;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d < mj) { mj = d; m[j] = d; }      // a NaN d (a non-finite point) leaves m alone
    }
    if (mj > bm) { bm = mj; bi = (int)j; }
  }
  fps_block_best(bm, bi, sm, si);
  if (tid == 0) { pm_out[blockIdx.x] = bm; pi_out[blockIdx.x] = bi; }
}

__global__ __launch_bounds__(EVAL_NT) void k_pcd_gather(const float* src, const long* idx, long ns, float* out32, double* out64) {
  for (long j = (long)blockIdx.x * EVAL_NT + threadIdx.x; j < ns; j += (long)gridDim.x * EVAL_NT) {
    const long i = idx[j];
    const float x = src[i * 3], y = src[i * 3 + 1], z = src[i * 3 + 2];
    if (out32) { out32[j * 3] = x; out32[j * 3 + 1] = y; out32[j * 3 + 2] = z; }
    if (out64) { out64[j * 3] = x; out64[j * 3 + 1] = y; out64[j * 3 + 2] = z; }
  }
}

// ------------------------------------------------------------------------------------------------------------- exact search through a uniform grid
// DESIGN.md section 20.  A counting sort of the finite targets into cubic cells of edge h, then every query walks the cells around its own, ring
// by ring, with the arithmetic of k_pcd_nn / k_pcd_knn on every candidate.  After ring r every target not yet seen lies more than r * h away
// along some axis, so a best squared distance below ((r * h)(1 - eps))^2 is final.  What PCD_GRID_RINGS rings do not settle is appended to a
// leftover list for the brute-force kernels.  The only atomics are integer counts; the order of the points inside a cell and of the leftover list
// varies between calls, the outputs do not: every comparison is on (squared distance, original index).
struct GridDev { double mn[3], h, inv_h; int G[3]; const double* sorted; const int* orig; const unsigned* start; };
static GridDev grid_dev(const PcdGrid& g) {
  GridDev d;
  for (int a = 0; a < 3; ++a) { d.mn[a] = g.mn[a]; d.G[a] = g.G[a]; }
  d.h = g.h; d.inv_h = g.inv_h; d.sorted = g.sorted; d.orig = g.orig; d.start = g.start;
  return d;
}
__device__ __forceinline__ bool pcd_finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }
// the clamp keeps every cell index in range, whatever the coordinate: a query outside the box lands in a border cell
__device__ __forceinline__ int pcd_cell_axis(double x, double mn, double inv_h, int G) {
  const double f = floor((x - mn) * inv_h);
  return !(f >= 0.0) ? 0 : (f > (double)(G - 1) ? G - 1 : (int)f);
}

// stage 1 (final = 0): per workgroup min xyz, max xyz and the count of the finite points of t -> out[b * 7 ..]; stage 2 (final = 1, one workgroup):
// the same over the nb rows of stage 1 -> out[0 .. 7)
__global__ __launch_bounds__(EVAL_NT) void k_pcd_grid_bbox(const double* in, long n, int final, double* out) {
  __shared__ double sh[EVAL_NT];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, cnt = 0;
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    if (final) {
      for (int a = 0; a < 3; ++a) { const double l = in[i * 7 + a], h = in[i * 7 + 3 + a]; lo[a] = l < lo[a] ? l : lo[a]; hi[a] = h > hi[a] ? h : hi[a]; }
      cnt += in[i * 7 + 6];
    } else {
      const double p[3] = {in[i * 3], in[i * 3 + 1], in[i * 3 + 2]};
      if (!pcd_finite3(p[0], p[1], p[2])) continue;
      for (int a = 0; a < 3; ++a) { lo[a] = p[a] < lo[a] ? p[a] : lo[a]; hi[a] = p[a] > hi[a] ? p[a] : hi[a]; }
      cnt += 1.0;
    }
  }
  double r[7];
  for (int a = 0; a < 3; ++a) { r[a] = eval_block_reduce<1>(lo[a], sh); r[3 + a] = eval_block_reduce<2>(hi[a], sh); }
  r[6] = eval_block_reduce<0>(cnt, sh);
  if (threadIdx.x == 0) for (int k = 0; k < 7; ++k) out[(long)blockIdx.x * 7 + k] = r[k];
}

// cell of every target (-1: a non-finite coordinate, in no cell) and the integer count per cell
__global__ __launch_bounds__(EVAL_NT) void k_pcd_grid_count(const double* t, long n, GridDev g, unsigned* counts, int* cell) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const double x = t[i * 3], y = t[i * 3 + 1], z = t[i * 3 + 2];
    int c = -1;
    if (pcd_finite3(x, y, z)) {
      const int cx = pcd_cell_axis(x, g.mn[0], g.inv_h, g.G[0]), cy = pcd_cell_axis(y, g.mn[1], g.inv_h, g.G[1]),
                cz = pcd_cell_axis(z, g.mn[2], g.inv_h, g.G[2]);
      c = (cz * g.G[1] + cy) * g.G[0] + cx;
      atomicAdd(&counts[c], 1u);
    }
    cell[i] = c;
  }
}
// exclusive scan of the counts, as the masked compaction does it: workgroup b owns the cells [b * chunk, (b + 1) * chunk)
__global__ __launch_bounds__(EVAL_NT) void k_pcd_grid_scan_sums(const unsigned* counts, long cells, long chunk, unsigned* bsum) {
  __shared__ unsigned sc[EVAL_NT];
  const long b0 = (long)blockIdx.x * chunk, b1 = b0 + chunk < cells ? b0 + chunk : cells;
  unsigned cnt = 0, mx = 0;
  for (long i = b0 + threadIdx.x; i < b1; i += EVAL_NT) { const unsigned v = counts[i]; cnt += v; mx = v > mx ? v : mx; }
  unsigned total;
  block_scan_excl(cnt, sc, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
  if (mx) atomicMax(&bsum[EVAL_MAXB + 1], mx);      // the fullest cell: an integer maximum, the same in any order
}
__global__ __launch_bounds__(EVAL_NT) void k_pcd_grid_scan_cells(const unsigned* counts, long cells, long chunk, const unsigned* bsum, unsigned* start) {
  __shared__ unsigned sc[EVAL_NT];
  const long b0 = (long)blockIdx.x * chunk, b1 = b0 + chunk < cells ? b0 + chunk : cells;
  unsigned base = bsum[blockIdx.x];
  for (long s0 = b0; s0 < b1; s0 += EVAL_NT) {      // chunk is a multiple of EVAL_NT: every thread of the block takes every step
    const long i = s0 + threadIdx.x;
    const unsigned v = i < b1 ? counts[i] : 0u;
    unsigned total;
    const unsigned pos = block_scan_excl(v, sc, &total);
    if (i < b1) start[i] = base + pos;
    base += total;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) start[cells] = bsum[EVAL_MAXB];
}
// the sorted points and their original indices; counts runs down to zero, so position start + count - 1 is taken exactly once
__global__ __launch_bounds__(EVAL_NT) void k_pcd_grid_scatter(const double* t, long n, const int* cell, const unsigned* start, unsigned* counts,
                                                         double* sorted, int* orig) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < n; i += (long)gridDim.x * EVAL_NT) {
    const int c = cell[i];
    if (c < 0) continue;
    const unsigned long pos = (unsigned long)start[c] + (atomicSub(&counts[c], 1u) - 1u);
    sorted[pos * 3] = t[i * 3]; sorted[pos * 3 + 1] = t[i * 3 + 1]; sorted[pos * 3 + 2] = t[i * 3 + 2];
    orig[pos] = (int)i;
  }
}

// Ring r around cell (cx, cy, cz), clipped to the grid: visit(a, b) for every run [a, b) of sorted positions.  Cells are stored x fastest, so a
// row of the two z faces and the two y faces is one run; the rows in between contribute their two end cells.
template <class F> __device__ __forceinline__ void pcd_ring(const GridDev& g, int cx, int cy, int cz, int r, F&& visit) {
  const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < g.G[0] - 1 ? cx + r : g.G[0] - 1;
  const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < g.G[1] - 1 ? cy + r : g.G[1] - 1;
  const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < g.G[2] - 1 ? cz + r : g.G[2] - 1;
  for (int zz = z0; zz <= z1; ++zz)
    for (int yy = y0; yy <= y1; ++yy) {
      const long row = ((long)zz * g.G[1] + yy) * g.G[0];
      if (zz - cz == r || cz - zz == r || yy - cy == r || cy - yy == r) visit(g.start[row + x0], g.start[row + x1 + 1]);
      else {
        if (cx - r >= 0) visit(g.start[row + cx - r], g.start[row + cx - r + 1]);
        if (cx + r <= g.G[0] - 1) visit(g.start[row + cx + r], g.start[row + cx + r + 1]);
      }
    }
}
__device__ __forceinline__ bool pcd_ring_covers(const GridDev& g, int cx, int cy, int cz, int r) {      // rings 0 .. r hold every cell
  return cx - r <= 0 && cx + r >= g.G[0] - 1 && cy - r <= 0 && cy + r >= g.G[1] - 1 && cz - r <= 0 && cz + r >= g.G[2] - 1;
}
__device__ __forceinline__ double pcd_ring_bound2(const GridDev& g, int r) {
  const double b = ((double)r * g.h) * (1.0 - PCD_GRID_EPS);
  return b * b;
}

// One query per thread, moved by T44 as k_pcd_nn moves it.  The winner is the lexicographic minimum of (squared distance, original index): cells
// are not visited in index order.  A query is settled when a target was found and either the ring bound or the whole grid is behind it.
__global__ __launch_bounds__(EVAL_NT) void k_pcd_nn_grid(const double* q, long nq, const double* T44, GridDev g, long n_in, int* idx, double* dist,
                                                    int* left, unsigned* n_left) {
  const long i = (long)blockIdx.x * EVAL_NT + threadIdx.x;
  if (i >= nq) return;
  double x = q[i * 3], y = q[i * 3 + 1], z = q[i * 3 + 2];
  pcd_move(T44, x, y, z);
  double best = INFINITY;
  int bi = -1;
  bool settled = false;
  if (n_in > 0 && pcd_finite3(x, y, z)) {
    const int cx = pcd_cell_axis(x, g.mn[0], g.inv_h, g.G[0]), cy = pcd_cell_axis(y, g.mn[1], g.inv_h, g.G[1]),
              cz = pcd_cell_axis(z, g.mn[2], g.inv_h, g.G[2]);
    for (int r = 0; r <= PCD_GRID_RINGS && !settled; ++r) {
      pcd_ring(g, cx, cy, cz, r, [&](unsigned a, unsigned b) {
        for (unsigned p = a; p < b; ++p) {
          const double d2 = pcd_d2(x, y, z, g.sorted + (unsigned long)p * 3);
          const int j = g.orig[p];
          if (d2 < best || (d2 == best && j < bi)) { best = d2; bi = j; }
        }
      });
      const bool all = pcd_ring_covers(g, cx, cy, cz, r);
      settled = bi >= 0 && (all || best < pcd_ring_bound2(g, r));
      if (all) break;
    }
  }
  if (settled) { idx[i] = bi; dist[i] = __dsqrt_rn(best); }
  else left[atomicAdd(n_left, 1u)] = (int)i;
}

// KNN of the cloud the grid was built over (every point finite), one point per thread, lists in LDS as k_pcd_knn holds them.  Insertion is by
// (squared distance, original index).  Settled when the list is full (k = min(knn, n)) and its last entry is below the ring bound, or the whole
// grid has been seen.
__global__ __launch_bounds__(KNN_B) void k_pcd_knn_grid(const double* pts, long n, int k, GridDev g, int* nbr, double* normals, int* left,
                                                        unsigned* n_left) {
  __shared__ double ld[KNN_MAX][KNN_B];
  __shared__ int li[KNN_MAX][KNN_B];
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * KNN_B + tid;
  if (i >= n) return;      // no barrier below
  const double x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
  const int cx = pcd_cell_axis(x, g.mn[0], g.inv_h, g.G[0]), cy = pcd_cell_axis(y, g.mn[1], g.inv_h, g.G[1]),
            cz = pcd_cell_axis(z, g.mn[2], g.inv_h, g.G[2]);
  int cnt = 0;
  bool settled = false;
  for (int r = 0; r <= PCD_GRID_RINGS && !settled; ++r) {
    pcd_ring(g, cx, cy, cz, r, [&](unsigned a, unsigned b) {
      for (unsigned p = a; p < b; ++p) {
        const double d2 = pcd_d2(x, y, z, g.sorted + (unsigned long)p * 3);
        const int j = g.orig[p];
        if (cnt < k || d2 < ld[cnt - 1][tid] || (d2 == ld[cnt - 1][tid] && j < li[cnt - 1][tid])) {
          int pos = cnt < k ? cnt++ : k - 1;
          while (pos > 0 && (ld[pos - 1][tid] > d2 || (ld[pos - 1][tid] == d2 && li[pos - 1][tid] > j))) {
            ld[pos][tid] = ld[pos - 1][tid]; li[pos][tid] = li[pos - 1][tid]; --pos;
          }
          ld[pos][tid] = d2; li[pos][tid] = j;
        }
      }
    });
    const bool all = pcd_ring_covers(g, cx, cy, cz, r);
    settled = cnt == k && (all || ld[k - 1][tid] < pcd_ring_bound2(g, r));
    if (all) break;
  }
  if (!settled) { left[atomicAdd(n_left, 1u)] = (int)i; return; }
  if (nbr) for (int j = 0; j < k; ++j) nbr[i * k + j] = li[j][tid];
  pcd_list_normal(pts, li, tid, k, normals + i * 3);
}

__global__ __launch_bounds__(EVAL_NT) void k_pcd_gather64(const double* src, const int* list, long nl, double* out) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < nl; i += (long)gridDim.x * EVAL_NT) {
    const long j = list[i];
    out[i * 3] = src[j * 3]; out[i * 3 + 1] = src[j * 3 + 1]; out[i * 3 + 2] = src[j * 3 + 2];
  }
}
__global__ __launch_bounds__(EVAL_NT) void k_pcd_nn_scatter(const int* list, long nl, const int* idx_l, const double* dist_l, int* idx, double* dist) {
  for (long i = (long)blockIdx.x * EVAL_NT + threadIdx.x; i < nl; i += (long)gridDim.x * EVAL_NT) {
    const long j = list[i];
    idx[j] = idx_l[i]; dist[j] = dist_l[i];
  }
}

// ------------------------------------------------------------------------------------------------------------- launchers
void launch_pcd_compact(const float* pred, const float* gt, const unsigned char* mask, long n, unsigned* counts, float* p_out, float* g_out,
                        hipStream_t s) {
  const int nb = eval_nblocks(n);
  const long chunk = ((n + nb - 1) / nb + EVAL_NT - 1) / EVAL_NT * EVAL_NT;      // a multiple of EVAL_NT; nb * chunk >= n
  hipLaunchKernelGGL(k_pcd_count, dim3(nb), dim3(EVAL_NT), 0, s, mask, n, chunk, counts);
  hipLaunchKernelGGL(k_pcd_offsets, dim3(1), dim3(EVAL_NT), 0, s, counts, nb);
  hipLaunchKernelGGL(k_pcd_scatter, dim3(nb), dim3(EVAL_NT), 0, s, pred, gt, mask, n, chunk, counts, p_out, g_out);
}

void launch_pcd_select(const void* v, int is_f64, long n, int stride, int offset, unsigned long long k, unsigned* sel, unsigned long long* res,
                       int slot, hipStream_t s) {
  (void)hipMemsetAsync(sel, 0, PCD_SEL_WORDS * sizeof(unsigned), s);
  const int passes = is_f64 ? 8 : 4, nb = eval_nblocks(n);
  for (int p = 0; p < passes; ++p) {
    const int shift = 56 - 8 * p;
    if (is_f64) hipLaunchKernelGGL(k_pcd_sel_hist<double>, dim3(nb), dim3(EVAL_NT), 0, s, (const double*)v, n, stride, offset, shift, p == 0, sel, sel);
    else hipLaunchKernelGGL(k_pcd_sel_hist<float>, dim3(nb), dim3(EVAL_NT), 0, s, (const float*)v, n, stride, offset, shift, p == 0, sel, sel);
    hipLaunchKernelGGL(k_pcd_sel_scan, dim3(1), dim3(256), 0, s, sel, shift, p == 0, p == passes - 1, (u64)k, (u64*)res, slot);
  }
}
void launch_pcd_shift_z(float* p, float* g, long n, const unsigned long long* res, int slot_p, int slot_g, hipStream_t s) {
  hipLaunchKernelGGL(k_pcd_shift_z, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, p, g, n, (const u64*)res, slot_p, slot_g);
}
void launch_pcd_center_norm(const float* p, long n, const unsigned long long* res, int slot_c, float* norm, hipStream_t s) {
  hipLaunchKernelGGL(k_pcd_center_norm, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, p, n, (const u64*)res, slot_c, norm);
}
void launch_pcd_align(const float* p, const float* g, const long* idx, long ns, float ratio, float gz, float* p32, float* g32, double* p64, double* g64,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_pcd_align, dim3(eval_nblocks(ns)), dim3(EVAL_NT), 0, s, p, g, idx, ns, ratio, gz, p32, g32, p64, g64);
}

// how the targets are split over blockIdx.y: enough slices that about 2048 workgroups are in flight, whole tiles per slice, at most 64 slices
static long pcd_nn_slice(long nq, long nt, int* ny) {
  const long bx = (nq + EVAL_NT - 1) / EVAL_NT, tiles = (nt + NN_TILE - 1) / NN_TILE;
  long want = 2048 / (bx < 1 ? 1 : bx);
  want = want < 1 ? 1 : (want > 64 ? 64 : want);
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const long slice = (tiles + want - 1) / want * NN_TILE;
  *ny = (int)((nt + slice - 1) / slice);
  if (*ny < 1) *ny = 1;
  return slice;
}
int pcd_nn_slices(long nq, long nt) { int ny; pcd_nn_slice(nq, nt, &ny); return ny; }

void launch_pcd_nn(const double* q, long nq, const double* t, long nt, const double* T44, int* idx, double* dist, int* pidx, double* pdist,
                   hipStream_t s) {
  int ny;
  const long slice = pcd_nn_slice(nq, nt, &ny);
  const int bx = (int)((nq + EVAL_NT - 1) / EVAL_NT);
  hipLaunchKernelGGL(k_pcd_nn, dim3(bx, ny), dim3(EVAL_NT), 0, s, q, nq, t, nt, T44, slice, pidx, pdist);
  hipLaunchKernelGGL(k_pcd_nn_combine, dim3(bx), dim3(EVAL_NT), 0, s, pidx, pdist, nq, ny, idx, dist);
}
void launch_pcd_kabsch(const double* q, const double* t, long nq, const double* T44, const int* idx, const double* dist, double threshold,
                       double* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(nq);
  hipLaunchKernelGGL(k_pcd_kabsch, dim3(*nb), dim3(EVAL_NT), 0, s, q, t, nq, T44, idx, dist, threshold, part);
}
void launch_pcd_move(const double* q, long n, const double* T44, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_pcd_move, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, q, n, T44, out);
}
void launch_pcd_knn_normals(const double* pts, long n, int knn, int* nbr, double* normals, hipStream_t s) {
  const int k = (int)(n < knn ? n : knn);
  hipLaunchKernelGGL(k_pcd_knn, dim3((unsigned)((n + KNN_B - 1) / KNN_B)), dim3(KNN_B), 0, s, pts, n, k, (const int*)nullptr, n, nbr, normals);
}
void launch_pcd_normal_dot(const double* nq, const double* nt, const int* idx, long n, double* dot, hipStream_t s) {
  hipLaunchKernelGGL(k_pcd_normal_dot, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, nq, nt, idx, n, dot);
}
// k picks in k + 1 plain launches: launch 0 initialises m, launch L writes pick L - 1; the last one has nothing left to update and is one workgroup
void launch_pcd_fps(const float* p, long n, long k, float* m, float* pm, int* pi, long* idx, float* sel_dist, hipStream_t s) {
  const int nb = eval_nblocks(n);
  for (long L = 0; L <= k; ++L) {
    const int last = L == k;
    hipLaunchKernelGGL(k_pcd_fps, dim3(last ? 1 : nb), dim3(EVAL_NT), 0, s, p, n, m, L, nb, last, pm, pi, idx, sel_dist);
  }
}
void launch_pcd_gather(const float* src, const long* idx, long ns, float* out32, double* out64, hipStream_t s) {
  hipLaunchKernelGGL(k_pcd_gather, dim3(eval_nblocks(ns)), dim3(EVAL_NT), 0, s, src, idx, ns, out32, out64);
}
void launch_pcd_sum(const double* v, long n, double* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_pcd_sum, dim3(*nb), dim3(EVAL_NT), 0, s, v, n, part);
}
void launch_pcd_count_below(const double* v, long n, const PcdThresholds& t, unsigned* part, int* nb, hipStream_t s) {
  *nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_pcd_count_below, dim3(*nb), dim3(EVAL_NT), 0, s, v, n, t, part);
}

// ------------------------------------------------------------------------------------------------------------- grid launchers
void launch_pcd_grid_bbox(const double* t, long n, double* part, double* box, hipStream_t s) {
  const int nb = eval_nblocks(n);
  hipLaunchKernelGGL(k_pcd_grid_bbox, dim3(nb), dim3(EVAL_NT), 0, s, t, n, 0, part);
  hipLaunchKernelGGL(k_pcd_grid_bbox, dim3(1), dim3(EVAL_NT), 0, s, (const double*)part, (long)nb, 1, box);
}

// host: the rule for h lives in pcd_host.h (plain C++, tested under sanitizers on the host)
void pcd_grid_shape(const double* box, long n, PcdGrid* g) {
  g->n = n; g->n_in = (long)box[6];
  pcd_host::grid_shape(box, g->n_in, PCD_GRID_OCC, PCD_GRID_MAX_CELLS, g->mn, &g->h, g->G, &g->cells);
  g->inv_h = 1.0 / g->h;
}

void launch_pcd_grid_build(const double* t, long n, const PcdGrid& g, unsigned* counts, unsigned* start, unsigned* bsum, int* cell, double* sorted,
                           int* orig, hipStream_t s) {
  const GridDev d = grid_dev(g);
  (void)hipMemsetAsync(counts, 0, (size_t)g.cells * sizeof(unsigned), s);
  (void)hipMemsetAsync(bsum, 0, (EVAL_MAXB + 2) * sizeof(unsigned), s);
  hipLaunchKernelGGL(k_pcd_grid_count, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, t, n, d, counts, cell);
  const int nb = eval_nblocks(g.cells);
  const long chunk = ((g.cells + nb - 1) / nb + EVAL_NT - 1) / EVAL_NT * EVAL_NT;      // a multiple of EVAL_NT; nb * chunk >= cells
  hipLaunchKernelGGL(k_pcd_grid_scan_sums, dim3(nb), dim3(EVAL_NT), 0, s, (const unsigned*)counts, g.cells, chunk, bsum);
  hipLaunchKernelGGL(k_pcd_offsets, dim3(1), dim3(EVAL_NT), 0, s, bsum, nb);
  hipLaunchKernelGGL(k_pcd_grid_scan_cells, dim3(nb), dim3(EVAL_NT), 0, s, (const unsigned*)counts, g.cells, chunk, (const unsigned*)bsum, start);
  hipLaunchKernelGGL(k_pcd_grid_scatter, dim3(eval_nblocks(n)), dim3(EVAL_NT), 0, s, t, n, (const int*)cell, (const unsigned*)start, counts, sorted, orig);
}
void launch_pcd_nn_grid(const double* q, long nq, const double* T44, const PcdGrid& g, int* idx, double* dist, int* left, unsigned* n_left,
                        hipStream_t s) {
  (void)hipMemsetAsync(n_left, 0, sizeof(unsigned), s);
  hipLaunchKernelGGL(k_pcd_nn_grid, dim3((unsigned)((nq + EVAL_NT - 1) / EVAL_NT)), dim3(EVAL_NT), 0, s, q, nq, T44, grid_dev(g), g.n_in, idx, dist, left, n_left);
}
void launch_pcd_knn_grid(const PcdGrid& g, int knn, int* nbr, double* normals, int* left, unsigned* n_left, hipStream_t s) {
  const int k = (int)(g.n < knn ? g.n : knn);
  (void)hipMemsetAsync(n_left, 0, sizeof(unsigned), s);
  hipLaunchKernelGGL(k_pcd_knn_grid, dim3((unsigned)((g.n + KNN_B - 1) / KNN_B)), dim3(KNN_B), 0, s, g.pts, g.n, k, grid_dev(g), nbr, normals, left,
                     n_left);
}
void launch_pcd_knn_normals_list(const double* pts, long n, int knn, const int* list, long nl, int* nbr, double* normals, hipStream_t s) {
  const int k = (int)(n < knn ? n : knn);
  hipLaunchKernelGGL(k_pcd_knn, dim3((unsigned)((nl + KNN_B - 1) / KNN_B)), dim3(KNN_B), 0, s, pts, n, k, list, nl, nbr, normals);
}
void launch_pcd_gather64(const double* src, const int* list, long nl, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_pcd_gather64, dim3(eval_nblocks(nl)), dim3(EVAL_NT), 0, s, src, list, nl, out);
}
void launch_pcd_nn_scatter(const int* list, long nl, const int* idx_l, const double* dist_l, int* idx, double* dist, hipStream_t s) {
  hipLaunchKernelGGL(k_pcd_nn_scatter, dim3(eval_nblocks(nl)), dim3(EVAL_NT), 0, s, list, nl, idx_l, dist_l, idx, dist);
}
