// Private to the two extern "C" units: capi.hip (include/unigeo_hip.h, the drop-in boundary) and capi_test.hip (include/unigeo_hip_test.h,
// test / tuning entry points).  The context handle, the error funnel and the host <-> device helpers both sides use.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/unigeo_hip.h"
#include "../../include/unigeo_hip_test.h"
#include "engine.h"
#include "kernels/eval_reduce.h"   // EVAL_MAXB: the rows of every `part` buffer

using namespace ug;

struct ug_ctx { Ctx c; long l1_info[4] = {-1, -1, 0, 1}; };   // l1_info: j, k, steps, certified of the last UG_ALIGN_L1 evaluation

#define UG_TRY(ctx, ...)                                   \
  if (!(ctx)) return -1;                                   \
  try { UG_CHECK(hipSetDevice((ctx)->c.device)); __VA_ARGS__; return 0; } \
  catch (const std::exception& e) { (ctx)->c.err = e.what(); (void)hipGetLastError(); return 1; } \
  catch (...) { (ctx)->c.err = "unknown error"; return 2; }

// ------------------------------------------------------------------ host <-> device helpers
struct Scope {
  Ctx& c; size_t mk;
  explicit Scope(Ctx& c_) : c(c_), mk(c_.ws.mark()) {}
  ~Scope() { (void)hipStreamSynchronize(c.stream); c.ws.release(mk); }
};
static inline void upload16(const float* h, long n, f16* d) {   // float host -> f16 device, into d
  std::vector<f16> v((size_t)n);
  for (long i = 0; i < n; ++i) v[i] = (f16)h[i];
  UG_CHECK(hipMemcpy(d, v.data(), (size_t)n * 2, hipMemcpyHostToDevice));
}
static inline f16* up16(Ctx& c, const float* h, long n) {
  f16* d = c.ws.get<f16>(n);
  upload16(h, n, d);
  return d;
}
static inline f16* up16_opt(Ctx& c, const float* h, long n) { return h ? up16(c, h, n) : nullptr; }
static inline void down16(Ctx& c, const f16* d, float* h, long n) {
  std::vector<f16> v((size_t)n);
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(v.data(), d, (size_t)n * 2, hipMemcpyDeviceToHost));
  for (long i = 0; i < n; ++i) h[i] = (float)v[i];
}
// NCHW float host -> NHWC(+channel pad) f16 device, into d (T*H*W*Cpad elements)
static inline void upload_nchw(const float* h, int T, int C, int H, int W, int Cpad, f16* d) {
  std::vector<f16> v((size_t)T * H * W * Cpad, (f16)0.f);
  for (int t = 0; t < T; ++t)
    for (int ch = 0; ch < C; ++ch)
      for (long p = 0; p < (long)H * W; ++p) v[((size_t)t * H * W + p) * Cpad + ch] = (f16)h[((size_t)t * C + ch) * H * W + p];
  UG_CHECK(hipMemcpy(d, v.data(), v.size() * 2, hipMemcpyHostToDevice));
}
static inline f16* up_nchw(Ctx& c, const float* h, int T, int C, int H, int W, int Cpad) {
  f16* d = c.ws.get<f16>((long)T * H * W * Cpad);
  upload_nchw(h, T, C, H, W, Cpad, d);
  return d;
}
static inline void down_nchw(Ctx& c, const f16* d, float* h, int T, int C, int H, int W) {
  std::vector<f16> v((size_t)T * H * W * C);
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(v.data(), d, v.size() * 2, hipMemcpyDeviceToHost));
  for (int t = 0; t < T; ++t)
    for (int ch = 0; ch < C; ++ch)
      for (long p = 0; p < (long)H * W; ++p) h[((size_t)t * C + ch) * H * W + p] = (float)v[((size_t)t * H * W + p) * C + ch];
}

// ------------------------------------------------------------------ depth evaluation: what ug_eval_depth* (product) and ug_op_masked_median (test) share
static inline float clip_lo(float v) { return std::isnan(v) ? -INFINITY : v; }
static inline float clip_hi(float v) { return std::isnan(v) ? INFINITY : v; }
static inline float depth_bound(float v) { return (std::isnan(v) || v <= 0.f) ? NAN : v; }   // NaN: the kernels test gt > 0 only
// the option fields as the kernels take them: the depth bound of mask1, the clamps before and after the alignment
struct DepthBounds { float md, lo, hi, plo, phi; };
static inline DepthBounds depth_bounds(const ug_depth_eval_opts* o) {
  return {depth_bound(o->max_depth), clip_lo(o->pre_clip_min), clip_hi(o->pre_clip_max), clip_lo(o->post_clip_min), clip_hi(o->post_clip_max)};
}
struct DepthEvalBufs { const float* dp; float* dg; unsigned char* dm; long n; };
static inline DepthEvalBufs depth_eval_upload(Ctx& c, const float* pred, const float* gt, const unsigned char* cmask, long n) {
  DepthEvalBufs b{nullptr, nullptr, nullptr, n};
  if (pred) { float* d = c.ws.get<float>(n); UG_CHECK(hipMemcpy(d, pred, n * 4, hipMemcpyHostToDevice)); b.dp = d; }
  else { UG_REQUIRE(c.io_ready && n == (long)c.T * c.H * c.W, "no resident depth of that size"); b.dp = c.d_depth; }
  b.dg = c.ws.get<float>(n); UG_CHECK(hipMemcpy(b.dg, gt, n * 4, hipMemcpyHostToDevice));
  if (cmask) { b.dm = (unsigned char*)c.ws.alloc(n); UG_CHECK(hipMemcpy(b.dm, cmask, n, hipMemcpyHostToDevice)); }
  return b;
}
// ------------------------------------------------------------------ exact grid search: what ug_eval_pcd_ex (product) and ug_op_pcd_*_grid (test) share
struct PcdSearchStats { long settled = 0, left = 0; };
static inline unsigned pcd_fetch_u32(Ctx& c, const unsigned* d) {
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  unsigned v = 0;
  UG_CHECK(hipMemcpy(&v, d, 4, hipMemcpyDeviceToHost));
  return v;
}
// The grid over t [n,3] (device).  sorted / orig / start stay on the workspace stack until the caller's Scope ends; the sort's scratch is released here.
static inline PcdGrid pcd_grid_build(Ctx& c, const double* t, long n, long* max_cell) {
  PcdGrid g{};
  double* part = c.ws.get<double>(PCD_MAXB * 7); double* box = c.ws.get<double>(8);
  launch_pcd_grid_bbox(t, n, part, box, c.stream);
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  double hb[8];
  UG_CHECK(hipMemcpy(hb, box, sizeof(hb), hipMemcpyDeviceToHost));
  pcd_grid_shape(hb, n, &g);
  g.pts = t;
  unsigned* start = c.ws.get<unsigned>(g.cells + 1);
  double* sorted = c.ws.get<double>(n * 3); int* orig = c.ws.get<int>(n);
  g.start = start; g.sorted = sorted; g.orig = orig;
  const size_t mk = c.ws.mark();
  unsigned* counts = c.ws.get<unsigned>(g.cells); unsigned* bsum = c.ws.get<unsigned>(PCD_MAXB + 2); int* cell = c.ws.get<int>(n);
  launch_pcd_grid_build(t, n, g, counts, start, bsum, cell, sorted, orig, c.stream);
  *max_cell = (long)pcd_fetch_u32(c, bsum + PCD_MAXB + 1);
  c.ws.release(mk);
  return g;
}
// launch_pcd_nn through the grid; left [nq] ints and n_left (one word) are device scratch.  Leaves the stream idle.
static inline void pcd_nn_search_grid(Ctx& c, const double* q, long nq, const double* T44, const PcdGrid& g, int* idx, double* dist, int* left,
                                      unsigned* n_left, PcdSearchStats& st) {
  launch_pcd_nn_grid(q, nq, T44, g, idx, dist, left, n_left, c.stream);
  const long nl = (long)pcd_fetch_u32(c, n_left);
  UG_REQUIRE(nl >= 0 && nl <= nq, "leftover count out of range");
  st.settled += nq - nl; st.left += nl;
  if (nl == 0) return;
  UG_REQUIRE((double)nl * (double)g.n <= 1099511627776.0,
             "more than 2^40 point pairs in one nearest-neighbour pass over the queries the grid left: lower pcd_downsample_num");
  const size_t mk = c.ws.mark();
  const int ny = pcd_nn_slices(nl, g.n);
  double* ql = c.ws.get<double>(nl * 3); int* il = c.ws.get<int>(nl); double* dl = c.ws.get<double>(nl);
  int* pidx = c.ws.get<int>((long)ny * nl); double* pdist = c.ws.get<double>((long)ny * nl);
  launch_pcd_gather64(q, left, nl, ql, c.stream);
  launch_pcd_nn(ql, nl, g.pts, g.n, T44, il, dl, pidx, pdist, c.stream);
  launch_pcd_nn_scatter(left, nl, il, dl, idx, dist, c.stream);
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  c.ws.release(mk);
}
// launch_pcd_knn_normals of the cloud the grid was built over.  A cloud with a non-finite point goes to the brute-force kernel whole: such a point
// can enter its lists, which no cell holds.
static inline void pcd_knn_search_grid(Ctx& c, const PcdGrid& g, int knn, int* nbr, double* normals, int* left, unsigned* n_left, PcdSearchStats& st) {
  const char* cap = "more than 2^40 point pairs in one neighbour pass over the points the grid left: lower pcd_downsample_num";
  if (g.n_in < g.n) {
    UG_REQUIRE((double)g.n * (double)g.n <= 1099511627776.0, cap);
    launch_pcd_knn_normals(g.pts, g.n, knn, nbr, normals, c.stream);
    st.left += g.n;
    return;
  }
  launch_pcd_knn_grid(g, knn, nbr, normals, left, n_left, c.stream);
  const long nl = (long)pcd_fetch_u32(c, n_left);
  UG_REQUIRE(nl >= 0 && nl <= g.n, "leftover count out of range");
  st.settled += g.n - nl; st.left += nl;
  if (nl == 0) return;
  UG_REQUIRE((double)nl * (double)g.n <= 1099511627776.0, cap);
  launch_pcd_knn_normals_list(g.pts, g.n, knn, left, nl, nbr, normals, c.stream);
}

// ------------------------------------------------------------------ voxel set: what ug_eval_pcd_scores (product) and ug_op_voxel_set (test) share
// the production table: the smallest power of two >= 2 * points, at least 1024 slots - at most half full even when every point has a cell of its own
static inline long voxel_capacity(long points) {
  long cap = 1024;
  while (cap < 2 * points) cap <<= 1;
  return cap;
}
static inline size_t voxel_table_bytes(long capacity) {      // as the arena rounds the four allocations of voxel_set_run
  auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
  return r256((size_t)capacity * 8) + r256((size_t)capacity * 4) + r256(VOX_STAT_WORDS * 4) + r256((size_t)PCD_MAXB * 3 * 4);
}
// cells of a (flag 1) and b (flag 2), device float64 [n,3] each, for edge v in a table of `capacity` slots -> out6 = |A|, |B|, |A & B|, |A | B|,
// skipped points of a, of b.  A probe that ran through the whole table is an error.  Leaves the stream idle and the workspace as it found it.
static inline void voxel_set_run(Ctx& c, const double* a, long na, const double* b, long nb_, double v, long capacity, long* out6, const char* who) {
  const size_t mk = c.ws.mark();
  unsigned long long* keys = c.ws.get<unsigned long long>(capacity); unsigned* flags = c.ws.get<unsigned>(capacity);
  unsigned* stat = c.ws.get<unsigned>(VOX_STAT_WORDS); unsigned* part = c.ws.get<unsigned>((long)PCD_MAXB * 3);
  int nb = 0;
  launch_vox_fill(keys, flags, capacity, stat, c.stream);
  launch_vox_insert(a, na, v, 1u, keys, flags, capacity, stat, c.stream);
  launch_vox_insert(b, nb_, v, 2u, keys, flags, capacity, stat, c.stream);
  launch_vox_count(flags, capacity, part, &nb, c.stream);
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  unsigned hs[VOX_STAT_WORDS];
  std::vector<unsigned> hp((size_t)nb * 3);
  UG_CHECK(hipMemcpy(hs, stat, sizeof(hs), hipMemcpyDeviceToHost));
  UG_CHECK(hipMemcpy(hp.data(), part, hp.size() * 4, hipMemcpyDeviceToHost));
  c.ws.release(mk);
  if (hs[VOX_OVERFLOW])
    throw std::runtime_error(std::string(who) + ": voxel table overflow: the cells of both clouds do not fit into " + std::to_string(capacity) + " slots");
  long cnt[3] = {0, 0, 0};
  for (int i = 0; i < nb; ++i) for (int k = 0; k < 3; ++k) cnt[k] += hp[(size_t)i * 3 + k];      // block order
  out6[0] = cnt[0] + cnt[2]; out6[1] = cnt[1] + cnt[2]; out6[2] = cnt[2]; out6[3] = cnt[0] + cnt[1] + cnt[2];
  out6[4] = hs[1]; out6[5] = hs[2];
}

// the result words of launch_masked_median, once the stream is idle: how many pixels were selected, the lower medians of prediction and ground truth
static inline void read_masked_median(Ctx& c, const unsigned* sel, unsigned& count, float& mp, float& mg) {
  UG_CHECK(hipStreamSynchronize(c.stream));
  unsigned r[3];
  UG_CHECK(hipMemcpy(r, sel + SEL_COUNT, sizeof(r), hipMemcpyDeviceToHost));
  count = r[0]; memcpy(&mp, &r[1], 4); memcpy(&mg, &r[2], 4);
}

// ------------------------------------------------------------------ exact L1 alignment: what ug_eval_depth_ex (product) and ug_op_l1_fit (test) share
// t = g_j - s * (q_j * 2^(E - 36)), product and difference rounded separately
static inline double l1_shift(double s, double gj, double qj, double down) {
#pragma clang fp contract(off)
  const double x = qj * down;
  const double sx = s * x;
  return gj - sx;
}
// The host loop over the kernels of kernels/metrics.hip: dp / dg are the n device pixels; st2 = (s, t) in double, info = j, k, steps, certified
// (indices among the valid pixels in pixel order, -1 where there is none).  Leaves the stream idle.
static inline void l1_fit_device(Ctx& c, const float* dp, const float* dg, long n, float md, float lo, float hi, double* st2, long* info) {
  typedef unsigned long long u64;
  st2[0] = st2[1] = 0.0;
  info[0] = info[1] = -1; info[2] = 0; info[3] = 1;
  if (n == 0) return;
  unsigned* sel = (unsigned*)c.ws.alloc(SEL_WORDS * 4);
  unsigned* aux = c.ws.get<unsigned>(L1_AUX_WORDS);
  launch_masked_median(dp, dg, n, md, lo, hi, sel, c.stream);
  launch_l1_maxabs(dp, dg, n, md, lo, hi, aux, c.stream);
  UG_CHECK(hipGetLastError());
  unsigned cnt; float mp, mg;
  read_masked_median(c, sel, cnt, mp, mg);
  if (cnt == 0) return;
  UG_REQUIRE(cnt < (1u << 26), "l1 alignment: 2^26 valid pixels or more (the integer weights must sum below 2^63)");
  unsigned mbits;
  UG_CHECK(hipMemcpy(&mbits, aux, 4, hipMemcpyDeviceToHost));
  float m; memcpy(&m, &mbits, 4);
  UG_REQUIRE(std::isfinite(m), "l1 alignment: non-finite prediction");
  int E = 0;
  if (m > 0.f) (void)frexp((double)m, &E);      // m = f * 2^E with 0.5 <= f < 1: the smallest E with m < 2^E
  const double up = ldexp(1.0, L1_BITS - E), down = ldexp(1.0, E - L1_BITS);
  long long* qc = c.ws.get<long long>(cnt); float* gc = c.ws.get<float>(cnt);
  u64* st = c.ws.get<u64>(L1_WORDS);
  unsigned* tie_idx = c.ws.get<unsigned>(L1_MAX_TIES); long long* tie_q = c.ws.get<long long>(L1_MAX_TIES);
  launch_l1_compact(dp, dg, n, md, lo, hi, aux, up, mp, cnt, qc, gc, c.stream);
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  unsigned j0;
  UG_CHECK(hipMemcpy(&j0, aux + 1, 4, hipMemcpyDeviceToHost));
  UG_REQUIRE(j0 < cnt, "l1 alignment: the median of the prediction was not found among the valid pixels");
  long pivot = j0, j = j0, k = -1;
  int steps = 0, certified = 1;
  double S = 0.0;
  std::vector<unsigned> ti; std::vector<long long> tq; std::vector<std::pair<unsigned, long long>> tied;
  for (;;) {
    launch_l1_step(qc, gc, cnt, pivot, down, st, tie_idx, tie_q, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    u64 r[5];      // key, target, W, lowest tied index, tied count
    UG_CHECK(hipMemcpy(r, st + L1_PREFIX, sizeof(r), hipMemcpyDeviceToHost));
    if (r[2] == 0) {      // every q equals the pivot's (the first step only): s = 0, t = the lower median of gt
      st2[1] = mg; info[0] = j0;
      return;
    }
    ++steps; j = pivot; S = pcd_unkey_f64(r[0]); k = (long)r[3];
    UG_REQUIRE(r[4] >= 1 && k >= 0 && k < (long)cnt, "l1 alignment: the selected slope belongs to no point");
    if (r[4] > L1_MAX_TIES) { certified = 0; break; }
    const size_t nt = (size_t)r[4];
    ti.resize(nt); tq.resize(nt); tied.resize(nt);
    UG_CHECK(hipMemcpy(ti.data(), tie_idx, nt * 4, hipMemcpyDeviceToHost));
    UG_CHECK(hipMemcpy(tq.data(), tie_q, nt * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nt; ++i) { UG_REQUIRE(ti[i] < cnt, "l1 alignment: tied index out of range"); tied[i] = {ti[i], tq[i]}; }
    // one point per distinct q, the lowest index of each, in index order
    std::sort(tied.begin(), tied.end(), [](const auto& a, const auto& b) { return a.second != b.second ? a.second < b.second : a.first < b.first; });
    tied.erase(std::unique(tied.begin(), tied.end(), [](const auto& a, const auto& b) { return a.second == b.second; }), tied.end());
    std::sort(tied.begin(), tied.end());
    long next = -1;
    for (size_t b0 = 0; b0 < tied.size() && next < 0; b0 += L1_CHK_SLOTS) {
      const size_t nb = std::min(tied.size() - b0, (size_t)L1_CHK_SLOTS);
      UG_CHECK(hipMemsetAsync(st + L1_CHK, 0, L1_CHK_SLOTS * 3 * sizeof(u64), c.stream));
      for (size_t i = 0; i < nb; ++i) launch_l1_check(qc, gc, cnt, (long)tied[b0 + i].first, S, down, st + L1_CHK + 3 * i, c.stream);
      UG_CHECK(hipGetLastError());
      UG_CHECK(hipStreamSynchronize(c.stream));
      u64 chk[L1_CHK_SLOTS * 3];
      UG_CHECK(hipMemcpy(chk, st + L1_CHK, sizeof(chk), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < nb && next < 0; ++i) {
        const u64 B = chk[3 * i], A = chk[3 * i + 1], W = chk[3 * i + 2];
        if (B > W - B || A > W - A) next = (long)tied[b0 + i].first;
      }
    }
    if (next < 0) break;
    if (steps == L1_MAX_STEPS) { certified = 0; break; }
    pivot = next;
  }
  long long qj; float gj;
  UG_CHECK(hipMemcpy(&qj, qc + j, 8, hipMemcpyDeviceToHost));
  UG_CHECK(hipMemcpy(&gj, gc + j, 4, hipMemcpyDeviceToHost));
  st2[0] = S; st2[1] = l1_shift(S, (double)gj, (double)qj, down);
  info[0] = j; info[1] = k; info[2] = steps; info[3] = certified;
}
