// extern "C" surface of libunigeo_hip.so, test half: exactly the functions declared in include/unigeo_hip_test.h - stage- and op-level entry points
// of the parity tests (host in / host out), tuning overrides and micro-benchmarks.  The drop-in boundary is capi.hip.
#include "capi_util.h"

// ------------------------------------------------------------------ weight layouts, as the engine binds them
// W [N][K] / b [N] (b may be NULL: bp stays empty) in the engine's GEGLU row order: blocks of 16 rows = [8 value | 8 gate] (geglu_src_row, bind_geglu)
static void pack_geglu(const float* W, const float* b, int N, int K, std::vector<float>& Wp, std::vector<float>& bp) {
  Wp.resize((size_t)N * K); if (b) bp.resize(N);
  for (int v = 0; v < N; ++v) {
    const int src = geglu_src_row(v, N / 2);
    memcpy(&Wp[(size_t)v * K], &W[(size_t)src * K], (size_t)K * 4);
    if (b) bp[v] = b[src];
  }
}
// weight [O][I][taps] -> the GEMM's K order: [O][taps][I] (tap-major), or chunk-major [O][I/64][taps][64] (GemmP::kchunk, I % 64 == 0)
static std::vector<float> pack_conv_weight(const float* weight, int O, int I, int taps, bool chunk_major) {
  std::vector<float> wp((size_t)O * taps * I);
  for (int o = 0; o < O; ++o) for (int i = 0; i < I; ++i) for (int tp = 0; tp < taps; ++tp)
    wp[chunk_major ? (((size_t)o * (I / 64) + i / 64) * taps + tp) * 64 + i % 64 : ((size_t)o * taps + tp) * I + i] = weight[((size_t)o * I + i) * taps + tp];
  return wp;
}

// ------------------------------------------------------------------ GEMM parameter blocks
static GemmP blank_gemm(Ctx& c) {
  GemmP p; memset(&p, 0, sizeof(p));
  p.zero = c.zero; p.nb_inner = 1; p.c0 = 1.f;
  return p;
}
// Out[M][ldo] = A[M][K] W[N][K]^T + bias
static GemmP dense_gemm(Ctx& c, const f16* A, int M, int K, const f16* W, int N, const f16* bias, f16* Out, long ldo) {
  GemmP p = blank_gemm(c);
  p.A0 = A; p.C0 = K; p.M = M; p.N = N; p.K = K; p.W = W; p.ldw = K; p.bias = bias; p.Out = Out; p.ldo = ldo;
  return p;
}
// implicit-GEMM convolution of one / two channels-last sources [T][H][W][C0 | C1], (kt, k, k) taps, O output channels
static GemmP conv_gemm(Ctx& c, const f16* x0, int C0, const f16* x1, int C1, int T, int H, int W, int kt, int k, int stride, int pad_t, int pad_l, int ups,
                       const f16* Wt, int O, const f16* bias, f16* Out) {
  GemmP p = blank_gemm(c);
  p.conv = 1; p.A0 = x0; p.A1 = x1; p.C0 = C0; p.C1 = C1; p.T = T; p.Hi = H; p.Wi = W; p.Ho = H * ups / stride; p.Wo = W * ups / stride;
  p.ups = ups; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l; p.kt = kt; p.ky = k; p.kx = k;
  p.M = T * p.Ho * p.Wo; p.N = O; p.K = (C0 + C1) * kt * k * k; p.W = Wt; p.ldw = p.K; p.bias = bias; p.Out = Out; p.ldo = O;
  return p;
}
// the context's tuning overrides, then the planner's tile config and split-K factor (+ the split-K scratch, from c.ws)
static void plan_gemm(Ctx& c, GemmP& p) {
  gemm_apply_tune(p, c.tune);
  int cf, sp;
  gemm_plan(p, 1, &cf, &sp);
  p.cfg_p1 = cf + 1; p.splitk = sp;
  if (sp > 1) p.partial = c.ws.get<float>((long)sp * p.M * p.N);
}
// the unfused feed-forward: mid = GEGLU(X W1^T + b1) [M][4C], Out = c0 * (mid W2^T + b2) + c1 * res.  Not planned: the launcher picks the first GEMM's
// tile and split (splitk = 0), the down-projection runs unsplit.
static void ff_two_launch(Ctx& c, const f16* X, int M, int C, const f16* W1, const f16* b1, const f16* W2, const f16* b2, const f16* res, float c0, float c1,
                          f16* mid, f16* Out) {
  const int I = 4 * C;
  GemmP g1 = dense_gemm(c, X, M, C, W1, 2 * I, b1, mid, I);
  g1.flags = UG_F_GEGLU;
  gemm_apply_tune(g1, c.tune); launch_gemm(g1, 1, c.stream);
  GemmP g2 = dense_gemm(c, mid, M, I, W2, C, b2, Out, C);
  g2.c0 = c0; g2.R1 = res; g2.ldr1 = C; g2.c1 = c1; g2.splitk = 1;
  gemm_apply_tune(g2, c.tune); launch_gemm(g2, 1, c.stream);
}
static FFusedP ff_fused(Ctx& c, const f16* X, int M, int C, const f16* W1, const f16* b1, const f16* W2, const f16* b2, const f16* res, float c0, float c1, f16* Out) {
  FFusedP p; memset(&p, 0, sizeof(p));
  p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2; p.R1 = res; p.c0 = c0; p.c1 = c1; p.Out = Out; p.M = M; p.C = C; p.zero = c.zero; p.variant = c.ff_variant;
  return p;
}

// ------------------------------------------------------------------ timing
struct Event {     // destroyed on every way out of its scope, a throwing UG_CHECK included
  hipEvent_t e = nullptr;
  Event() { UG_CHECK(hipEventCreate(&e)); }
  ~Event() { (void)hipEventDestroy(e); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
};
// `warm` untimed launches, then the time of `iters` launches together, in milliseconds; launch(i) enqueues timed launch i on c.stream (warm-up: i = 0)
template <class Fn> static float time_launches_ms(Ctx& c, int warm, int iters, Fn&& launch) {
  for (int i = 0; i < warm; ++i) launch(0);
  Event e0, e1;
  UG_CHECK(hipEventRecord(e0.e, c.stream));
  for (int i = 0; i < iters; ++i) launch(i);
  UG_CHECK(hipEventRecord(e1.e, c.stream));
  UG_CHECK(hipEventSynchronize(e1.e));
  float ms = 0.f;
  UG_CHECK(hipEventElapsedTime(&ms, e0.e, e1.e));
  return ms;
}

// [px][3] float host -> [px][8] f16 device (channels 3 .. 7 zero): the VAE encoders' input
static f16* upload_rgb_pad8(Ctx& c, const float* video, long px) {
  std::vector<f16> v((size_t)px * 8, (f16)0.f);
  for (long p = 0; p < px; ++p) for (int ch = 0; ch < 3; ++ch) v[p * 8 + ch] = (f16)video[p * 3 + ch];
  f16* d = c.ws.get<f16>(px * 8);
  UG_CHECK(hipMemcpy(d, v.data(), v.size() * 2, hipMemcpyHostToDevice));
  return d;
}

extern "C" {

// ------------------------------------------------------------------ per-context switches and overrides
int ug_set_ff_fused(ug_ctx* x, int on) {
  if (!x) return -1;
  x->c.ff_fused = on & 3; x->c.lane_need.clear();   // bit 0: fused feed-forward kernel, bit 1: its pre-LayerNorm inside the kernel (a feature toggle changes the transient memory a lane task needs)
  return 0;
}
int ug_dc_set_trace(ug_ctx* x, float* host_latents, int steps) {
  if (!x) return -1;
  x->c.trace_host = host_latents; x->c.trace_steps = host_latents ? steps : 0;
  return 0;
}
int ug_profile_begin_shapes(ug_ctx* x) { UG_TRY(x, prof_begin(x->c, true)); }
int ug_tune_force(ug_ctx* x, int cfg, int split) {
  if (!x) return -1;
  if (cfg <= -100) {                                         // knob mask: ug_tune_force(ctx, -100 - knobs, 0)
    x->c.tune.knobs = (-cfg - 100) & ~4194304;
    if (x->c.cosched) x->c.tune.knobs |= 4194304;            // the co-scheduled planner rule belongs to ug_set_coscheduled alone: a forced mask neither sets nor drops it
  }
  else { x->c.tune.cfg = cfg; x->c.tune.split = split; }
  x->c.lane_need.clear();    // forced split-K / tile configs change the partial buffers a lane task needs
  return 0;
}
int ug_tune_flash(ug_ctx* x, int variant) { if (!x) return -1; x->c.flash_variant = variant; return 0; }
int ug_tune_ff(ug_ctx* x, int variant) { if (!x) return -1; x->c.ff_variant = variant; x->c.lane_need.clear(); return 0; }

// ------------------------------------------------------------------ stage level
int ug_clip_embed(ug_ctx* x, const float* frames, int T, int H, int W, float* emb_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const long px = (long)T * H * W;
    float* df = c.ws.get<float>(px * 3); float* dn = c.ws.get<float>(px * 3);
    UG_CHECK(hipMemcpy(df, frames, px * 3 * 4, hipMemcpyHostToDevice));
    UG_CHECK(hipMemsetAsync(dn, 0, px * 3 * 4, c.stream));
    f16* src = c.ws.get<f16>(px * 3); f16* vin = c.ws.get<f16>(px * 8);
    launch_prep_video(df, dn, src, vin, T, H, W, 0.f, c.stream);
    f16* e = clip_embed(c, src, T, H, W);
    down16(c, e, emb_out, (long)T * c.clip.cfg.proj);
  });
}

int ug_vae_encode(ug_ctx* x, const float* video, int T, int H, int W, float* lat_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    f16* l = vae_encode(c, upload_rgb_pad8(c, video, (long)T * H * W), T, H, W);
    down_nchw(c, l, lat_out, T, c.vae.cfg.lat, H / 8, W / 8);
  });
}

int ug_vae_decode(ug_ctx* x, const float* z, int T, int h, int w, float* frames_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    f16* dz = up_nchw(c, z, T, c.vae.cfg.lat, h, w, c.vae.cfg.lat);
    const long px = (long)T * h * 8 * w * 8;
    float* out = c.ws.get<float>(px * 3);
    vae_decode(c, dz, T, h, w, out);
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(frames_out, out, px * 3 * 4, hipMemcpyDeviceToHost));
  });
}

int ug_unet_forward(ug_ctx* x, const float* sample, int T, int h, int w, float timestep, const float* clip_emb, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const UNetCfg& g = c.unet.cfg;
    f16* dx = up_nchw(c, sample, T, g.in_ch, h, w, g.in_ch);
    f16* de = up16(c, clip_emb, (long)T * g.cross_dim);
    unet_prepare(c, T, de, &timestep, 1);
    f16* y = unet_forward(c, dx, T, h, w, 0);
    down_nchw(c, y, out, T, g.out_ch, h, w);
  });
}

// one batched UNet pass over two videos stacked [2][T] (the classifier-free-guidance pass of ug_dc_run, without the combine)
int ug_unet_forward_pair(ug_ctx* x, const float* sample_a, const float* emb_a, const float* sample_b, const float* emb_b, int T, int h, int w,
                         float timestep, float* out_a, float* out_b) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const UNetCfg& g = c.unet.cfg;
    UG_REQUIRE(sample_a && emb_a && sample_b && emb_b && out_a && out_b && T >= 1, "ug_unet_forward_pair: null buffer / no frames");
    const long ns = (long)T * h * w * g.in_ch, ne = (long)T * g.cross_dim;
    f16* dx = c.ws.get<f16>(2 * ns);
    f16* de = c.ws.get<f16>(2 * ne);
    const float* smp[2] = {sample_a, sample_b};
    const float* emb[2] = {emb_a, emb_b};
    for (int v = 0; v < 2; ++v) {     // straight into the stacked [2][T] buffers
      upload_nchw(smp[v], T, g.in_ch, h, w, g.in_ch, dx + v * ns);
      upload16(emb[v], ne, de + v * ne);
    }
    unet_prepare(c, T, de, &timestep, 1, 2);
    f16* y = unet_forward(c, dx, T, h, w, 0, 2);
    const long no = (long)T * h * w * g.out_ch;
    down_nchw(c, y, out_a, T, g.out_ch, h, w);
    down_nchw(c, y + no, out_b, T, g.out_ch, h, w);
  });
}

// ------------------------------------------------------------------ StableNormal stages
int ug_sn_unet_forward(ug_ctx* x, int which, const float* sample, const float* zimg, int B, int h, int w, float t_unet, float t_ctrl,
                       const float* prompt, const float* dino_tokens, int use_ctrl, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    SN& s = c.sn;
    UG_REQUIRE(s.bound, "StableNormal weights are not bound");
    f16* ds = up_nchw(c, sample, B, 4, h, w, 4);
    f16* dz = zimg ? up_nchw(c, zimg, B, 4, h, w, 4) : nullptr;
    f16* dp = up16(c, prompt, 77L * s.cfg.cross_dim);
    const int g = s.dino.cfg.image / s.dino.cfg.patch;
    f16* dt = dino_tokens ? up16(c, dino_tokens, (long)B * g * g * s.dino.cfg.hidden) : nullptr;
    UG_REQUIRE(!use_ctrl || dz, "ControlNet evaluation needs the image latent");
    f16* y = sn_unet_eval(c, which, ds, dz, B, h, w, t_unet, t_ctrl, dp, dt, use_ctrl);
    down_nchw(c, y, out, B, 4, h, w);
  });
}
int ug_sn_dino(ug_ctx* x, const float* images01, int B, int H, int W, float* tokens_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const long px = (long)B * H * W;
    float* df = c.ws.get<float>(px * 3);
    UG_CHECK(hipMemcpy(df, images01, px * 3 * 4, hipMemcpyHostToDevice));
    f16* src = c.ws.get<f16>(px * 3); f16* vin = c.ws.get<f16>(px * 8);
    launch_prep_video(df, df, src, vin, B, H, W, 0.f, c.stream);
    f16* t = sn_dino_tokens(c, src, B, H, W);
    const int g = c.sn.dino.cfg.image / c.sn.dino.cfg.patch;
    down16(c, t, tokens_out, (long)B * g * g * c.sn.dino.cfg.hidden);
  });
}
int ug_sn_vae_decode(ug_ctx* x, const float* z, int B, int h, int w, float* out_bhwc) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    f16* dz = up_nchw(c, z, B, 4, h, w, 4);
    f16* rgb = sn_vae_decode(c, dz, B, h, w);
    const long px = (long)B * h * 8 * w * 8;
    std::vector<f16> v((size_t)px * 8);
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(v.data(), rgb, v.size() * 2, hipMemcpyDeviceToHost));
    for (long p = 0; p < px; ++p) for (int ch = 0; ch < 3; ++ch) out_bhwc[p * 3 + ch] = (float)v[p * 8 + ch];
  });
}
int ug_sn_vae_encode(ug_ctx* x, const float* video, int B, int H, int W, float* lat_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    f16* l = vae_encode_v(c, c.sn.vae, upload_rgb_pad8(c, video, (long)B * H * W), B, H, W, false);
    down_nchw(c, l, lat_out, B, c.sn.vae.cfg.lat, H / 8, W / 8);
  });
}

// ------------------------------------------------------------------ op level
int ug_op_masked_median(ug_ctx* x, const float* pred, const float* gt, long n, float max_depth, float pre_clip_min, float pre_clip_max,
                        float* out_medians, long* out_count) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(n >= 1 && n < (1L << 32), "pixel count");
    const DepthEvalBufs d = depth_eval_upload(c, pred, gt, nullptr, n);
    unsigned* sel = (unsigned*)c.ws.alloc(SEL_WORDS * 4);
    launch_masked_median(d.dp, d.dg, n, depth_bound(max_depth), clip_lo(pre_clip_min), clip_hi(pre_clip_max), sel, c.stream);
    unsigned cnt;
    read_masked_median(c, sel, cnt, out_medians[0], out_medians[1]);
    *out_count = (long)cnt;
  });
}

int ug_op_l1_fit(ug_ctx* x, const float* pred, const float* gt, long n, const ug_depth_eval_opts* o, double* out_st, long* out_info) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(o && out_st && out_info, "opts, out_st and out_info must not be NULL");
    UG_REQUIRE(n >= 0 && n < (1L << 32), "pixel count");
    if (n == 0) { out_st[0] = out_st[1] = 0.0; out_info[0] = out_info[1] = -1; out_info[2] = 0; out_info[3] = 1; return 0; }
    UG_REQUIRE(gt != nullptr, "gt must not be NULL");
    const DepthEvalBufs d = depth_eval_upload(c, pred, gt, nullptr, n);
    l1_fit_device(c, d.dp, d.dg, n, depth_bound(o->max_depth), clip_lo(o->pre_clip_min), clip_hi(o->pre_clip_max), out_st, out_info);
  });
}

// the kernels of ug_eval_pcd one by one (kernels/pcd.hip)
int ug_op_pcd_nn(ug_ctx* x, const double* query, long nq, const double* target, long nt, const double* T44, int* idx_out, double* dist_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(query && target && idx_out && dist_out, "query, target, idx_out and dist_out must not be NULL");
    UG_REQUIRE(nq >= 1 && nt >= 1 && nq < (1L << 31) && nt < (1L << 31), "point counts must be 1 .. 2^31 - 1");
    UG_REQUIRE((double)nq * (double)nt <= 1099511627776.0, "more than 2^40 point pairs in one nearest-neighbour pass: lower pcd_downsample_num");
    double* dq = c.ws.get<double>(nq * 3); double* dt = c.ws.get<double>(nt * 3);
    UG_CHECK(hipMemcpy(dq, query, (size_t)nq * 24, hipMemcpyHostToDevice));
    UG_CHECK(hipMemcpy(dt, target, (size_t)nt * 24, hipMemcpyHostToDevice));
    double* dT = nullptr;
    if (T44) { dT = c.ws.get<double>(16); UG_CHECK(hipMemcpy(dT, T44, 128, hipMemcpyHostToDevice)); }
    const int ny = pcd_nn_slices(nq, nt);
    int* idx = c.ws.get<int>(nq); double* dist = c.ws.get<double>(nq);
    int* pidx = c.ws.get<int>((long)ny * nq); double* pdist = c.ws.get<double>((long)ny * nq);
    launch_pcd_nn(dq, nq, dt, nt, dT, idx, dist, pidx, pdist, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(idx_out, idx, (size_t)nq * 4, hipMemcpyDeviceToHost));
    UG_CHECK(hipMemcpy(dist_out, dist, (size_t)nq * 8, hipMemcpyDeviceToHost));
  });
}
int ug_op_pcd_select(ug_ctx* x, const void* values, int is_f64, long n, long k, void* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(values && out, "values and out must not be NULL");
    UG_REQUIRE(n >= 1 && n < (1L << 31) && k >= 0 && k < n, "n must be 1 .. 2^31 - 1 and k inside it");
    const size_t bytes = (size_t)n * (is_f64 ? 8 : 4);
    void* dv = c.ws.alloc(bytes); UG_CHECK(hipMemcpy(dv, values, bytes, hipMemcpyHostToDevice));
    unsigned* sel = (unsigned*)c.ws.alloc(PCD_SEL_WORDS * 4);
    unsigned long long* res = c.ws.get<unsigned long long>(1);
    launch_pcd_select(dv, is_f64, n, 1, 0, (unsigned long long)k, sel, res, 0, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    unsigned long long key;
    UG_CHECK(hipMemcpy(&key, res, 8, hipMemcpyDeviceToHost));
    if (is_f64) *(double*)out = pcd_unkey_f64(key); else *(float*)out = pcd_unkey_f32(key);
  });
}
int ug_op_pcd_knn_normals(ug_ctx* x, const double* pts, long n, int knn, int* nbr_out, double* normals_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(pts && normals_out, "pts and normals_out must not be NULL");
    UG_REQUIRE(n >= 1 && n < (1L << 31) && knn >= 1 && knn <= UG_PCD_MAX_KNN, "n must be 1 .. 2^31 - 1 and knn 1 .. UG_PCD_MAX_KNN");
    UG_REQUIRE((double)n * (double)n <= 1099511627776.0, "more than 2^40 point pairs in one neighbour pass: lower pcd_downsample_num");
    const long k = n < knn ? n : knn;
    double* dp = c.ws.get<double>(n * 3); UG_CHECK(hipMemcpy(dp, pts, (size_t)n * 24, hipMemcpyHostToDevice));
    int* nbr = nbr_out ? c.ws.get<int>(n * k) : nullptr;
    double* nrm = c.ws.get<double>(n * 3);
    launch_pcd_knn_normals(dp, n, knn, nbr, nrm, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    if (nbr_out) UG_CHECK(hipMemcpy(nbr_out, nbr, (size_t)n * k * 4, hipMemcpyDeviceToHost));
    UG_CHECK(hipMemcpy(normals_out, nrm, (size_t)n * 24, hipMemcpyDeviceToHost));
  });
}
// the two searches through the uniform grid
int ug_op_pcd_nn_grid(ug_ctx* x, const double* query, long nq, const double* target, long nt, const double* T44, int* idx_out, double* dist_out,
                      long* stats) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(query && target && idx_out && dist_out, "query, target, idx_out and dist_out must not be NULL");
    UG_REQUIRE(nq >= 1 && nt >= 1 && nq < (1L << 31) && nt < (1L << 31), "point counts must be 1 .. 2^31 - 1");
    double* dq = c.ws.get<double>(nq * 3); double* dt = c.ws.get<double>(nt * 3);
    UG_CHECK(hipMemcpy(dq, query, (size_t)nq * 24, hipMemcpyHostToDevice));
    UG_CHECK(hipMemcpy(dt, target, (size_t)nt * 24, hipMemcpyHostToDevice));
    double* dT = nullptr;
    if (T44) { dT = c.ws.get<double>(16); UG_CHECK(hipMemcpy(dT, T44, 128, hipMemcpyHostToDevice)); }
    int* idx = c.ws.get<int>(nq); double* dist = c.ws.get<double>(nq);
    int* left = c.ws.get<int>(nq); unsigned* n_left = c.ws.get<unsigned>(1);
    long cellmax = 0;
    PcdSearchStats st;
    const PcdGrid g = pcd_grid_build(c, dt, nt, &cellmax);
    pcd_nn_search_grid(c, dq, nq, dT, g, idx, dist, left, n_left, st);
    UG_CHECK(hipMemcpy(idx_out, idx, (size_t)nq * 4, hipMemcpyDeviceToHost));
    UG_CHECK(hipMemcpy(dist_out, dist, (size_t)nq * 8, hipMemcpyDeviceToHost));
    if (stats) { stats[0] = st.settled; stats[1] = st.left; stats[2] = g.cells; stats[3] = cellmax; }
  });
}
int ug_op_pcd_knn_normals_grid(ug_ctx* x, const double* pts, long n, int knn, int* nbr_out, double* normals_out, long* stats) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(pts && normals_out, "pts and normals_out must not be NULL");
    UG_REQUIRE(n >= 1 && n < (1L << 31) && knn >= 1 && knn <= UG_PCD_MAX_KNN, "n must be 1 .. 2^31 - 1 and knn 1 .. UG_PCD_MAX_KNN");
    const long k = n < knn ? n : knn;
    double* dp = c.ws.get<double>(n * 3); UG_CHECK(hipMemcpy(dp, pts, (size_t)n * 24, hipMemcpyHostToDevice));
    int* nbr = nbr_out ? c.ws.get<int>(n * k) : nullptr;
    double* nrm = c.ws.get<double>(n * 3);
    int* left = c.ws.get<int>(n); unsigned* n_left = c.ws.get<unsigned>(1);
    long cellmax = 0;
    PcdSearchStats st;
    const PcdGrid g = pcd_grid_build(c, dp, n, &cellmax);
    pcd_knn_search_grid(c, g, knn, nbr, nrm, left, n_left, st);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    if (nbr_out) UG_CHECK(hipMemcpy(nbr_out, nbr, (size_t)n * k * 4, hipMemcpyDeviceToHost));
    UG_CHECK(hipMemcpy(normals_out, nrm, (size_t)n * 24, hipMemcpyDeviceToHost));
    if (stats) { stats[0] = st.settled; stats[1] = st.left; stats[2] = g.cells; stats[3] = cellmax; }
  });
}
// the voxel set alone, in a table of a forced size
int ug_op_voxel_set(ug_ctx* x, const double* a, long na, const double* b, long nb, double voxel_size, int capacity_log2, long* out6) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(out6 && (a || na == 0) && (b || nb == 0), "out6 must not be NULL, nor a cloud with points");
    UG_REQUIRE(na >= 0 && nb >= 0 && na < (1L << 31) && nb < (1L << 31), "na and nb must be 0 .. 2^31 - 1");
    UG_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "voxel_size must be positive and finite");
    UG_REQUIRE(capacity_log2 >= 0 && capacity_log2 <= 30, "capacity_log2 must be 0 (the production rule) or 1..30");
    const long capacity = capacity_log2 ? 1L << capacity_log2 : voxel_capacity(na + nb);
    double* da = c.ws.get<double>(na * 3 + 1); double* db = c.ws.get<double>(nb * 3 + 1);
    if (na) UG_CHECK(hipMemcpy(da, a, (size_t)na * 24, hipMemcpyHostToDevice));
    if (nb) UG_CHECK(hipMemcpy(db, b, (size_t)nb * 24, hipMemcpyHostToDevice));
    voxel_set_run(c, da, na, db, nb, voxel_size, capacity, out6, "ug_op_voxel_set");
  });
}
// farthest-point sampling alone
int ug_op_pcd_fps(ug_ctx* x, const float* pts, long n, long k, long* idx_out, float* sel_dist_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(pts && idx_out && sel_dist_out, "pts, idx_out and sel_dist_out must not be NULL");
    UG_REQUIRE(n >= 1 && n < (1L << 31), "n must be 1 .. 2^31 - 1");
    UG_REQUIRE(k >= 1 && k <= n, "k must be 1 .. n");
    float* dp = c.ws.get<float>(n * 3); UG_CHECK(hipMemcpy(dp, pts, (size_t)n * 12, hipMemcpyHostToDevice));
    float* m = c.ws.get<float>(n); float* pm = c.ws.get<float>(2 * PCD_MAXB); int* pi = c.ws.get<int>(2 * PCD_MAXB);
    long* idx = c.ws.get<long>(k); float* sel = c.ws.get<float>(k);
    launch_pcd_fps(dp, n, k, m, pm, pi, idx, sel, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(idx_out, idx, (size_t)k * sizeof(long), hipMemcpyDeviceToHost));
    UG_CHECK(hipMemcpy(sel_dist_out, sel, (size_t)k * 4, hipMemcpyDeviceToHost));
  });
}

int ug_op_linear(ug_ctx* x, const float* A, int M, int K, const float* W, int N, const float* bias, const float* R1,
                 float c0, float c1, int act, int geglu, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    std::vector<float> Wp, bp;
    if (geglu) { pack_geglu(W, bias, N, K, Wp, bp); W = Wp.data(); if (bias) bias = bp.data(); }
    const int Nout = geglu ? N / 2 : N;
    f16* dA = up16(c, A, (long)M * K); f16* dW = up16(c, W, (long)N * K);
    f16* db = up16_opt(c, bias, N); f16* dR = up16_opt(c, R1, (long)M * Nout);
    f16* dO = c.ws.get<f16>((long)M * Nout);
    GemmP p = dense_gemm(c, dA, M, K, dW, N, db, dO, Nout);
    p.R1 = dR; p.ldr1 = Nout; p.c0 = c0; p.c1 = c1; p.act = act; p.flags = geglu ? UG_F_GEGLU : 0;
    plan_gemm(c, p);
    launch_gemm(p, 1, c.stream);
    down16(c, dO, out, (long)M * Nout);
  });
}

// out = c0 * FF(LayerNorm(x') * gamma + beta) + c1 * x',  x' = fp16(X + addvec[row / rows_per_vec]) (addvec may be NULL: x' = X).
// mode 0: LayerNorm launch + two GEMM launches; 1: LayerNorm launch + fused feed-forward; 2: everything inside the fused kernel.
int ug_op_ln_ff(ug_ctx* x, const float* X, int M, int C, const float* gamma, const float* beta, float eps, const float* addvec, int rows_per_vec,
                const float* W1, const float* b1, const float* W2, const float* b2, float c0, float c1, int mode, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int I = 4 * C;
    std::vector<float> w1, bb1;
    pack_geglu(W1, b1, 2 * I, C, w1, bb1);
    const int nvec = addvec ? (M + rows_per_vec - 1) / rows_per_vec : 0;
    f16* dX = up16(c, X, (long)M * C); f16* dW1 = up16(c, w1.data(), (long)2 * I * C); f16* db1 = up16(c, bb1.data(), 2 * I);
    f16* dW2 = up16(c, W2, (long)C * I); f16* db2 = up16(c, b2, C);
    f16* dg = up16(c, gamma, C); f16* dbt = up16(c, beta, C); f16* dav = addvec ? up16(c, addvec, (long)nvec * C) : nullptr;
    f16* dO = c.ws.get<f16>((long)M * C);
    if (mode == 2) {
      FFusedP p = ff_fused(c, dX, M, C, dW1, db1, dW2, db2, dX, c0, c1, dO);
      p.ln_g = dg; p.ln_b = dbt; p.ln_eps = eps; p.addvec = dav; p.rows_per_vec = rows_per_vec;
      launch_ff_fused(p, c.stream);
    } else {
      f16* t1 = c.ws.get<f16>((long)M * C); f16* xo = c.ws.get<f16>((long)M * C);
      LayerNormP l; memset(&l, 0, sizeof(l));
      l.X = dX; l.Y = t1; l.M = M; l.C = C; l.eps = eps; l.gamma = dg; l.beta = dbt; l.addvec = dav; l.rows_per_vec = rows_per_vec; l.Xout = dav ? xo : nullptr;
      launch_layernorm(l, c.stream);
      const f16* res = dav ? xo : dX;
      if (mode == 1) launch_ff_fused(ff_fused(c, t1, M, C, dW1, db1, dW2, db2, res, c0, c1, dO), c.stream);
      else ff_two_launch(c, t1, M, C, dW1, db1, dW2, db2, res, c0, c1, c.ws.get<f16>((long)M * I), dO);
    }
    down16(c, dO, out, (long)M * C);
  });
}

int ug_op_ff(ug_ctx* x, const float* X, int M, int C, const float* W1, const float* b1, const float* W2, const float* b2, const float* R1,
             float c0, float c1, int fused, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int I = 4 * C;
    std::vector<float> w1, bb1;
    pack_geglu(W1, b1, 2 * I, C, w1, bb1);
    f16* dX = up16(c, X, (long)M * C); f16* dW1 = up16(c, w1.data(), (long)2 * I * C); f16* db1 = up16(c, bb1.data(), 2 * I);
    f16* dW2 = up16(c, W2, (long)C * I); f16* db2 = up16(c, b2, C); f16* dR = up16_opt(c, R1, (long)M * C);
    f16* dO = c.ws.get<f16>((long)M * C);
    if (fused) launch_ff_fused(ff_fused(c, dX, M, C, dW1, db1, dW2, db2, dR, c0, c1, dO), c.stream);
    else ff_two_launch(c, dX, M, C, dW1, db1, dW2, db2, dR, c0, c1, c.ws.get<f16>((long)M * I), dO);
    down16(c, dO, out, (long)M * C);
  });
}

// Every launch form of the feed-forward (tests/test_ff_forms_gpu.py; the contract stands in include/unigeo_hip_test.h).  X, R1 and R2 go to the device
// with their in_guard rows and addvec with its extra vector, the kernels are told M; out_inout goes up as given and all of it comes back.
int ug_op_ff_ex(ug_ctx* x, const float* X, int M, int C, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* R1, int r1_is_x, const float* R2, float c0, float c1, float c2,
                const float* gamma, const float* beta, float eps, const float* addvec, int rows_per_vec,
                int mode, int max_wg, long in_guard, long out_guard, float* out_inout, int* info_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const bool pre = gamma != nullptr;
    UG_REQUIRE(X && W1 && b1 && W2 && out_inout && M >= 1 && C >= 1 && mode >= 0 && mode <= 3 && max_wg >= 0 && in_guard >= 0 && out_guard >= 0 && !(R1 && r1_is_x),
               "ug_op_ff_ex: arguments");
    UG_REQUIRE(!addvec || (pre && rows_per_vec >= 1), "ug_op_ff_ex: addvec belongs to the pre-norm, rows_per_vec >= 1");
    const int I = 4 * C;
    const long rows_in = M + in_guard;
    std::vector<float> w1, bb1;
    pack_geglu(W1, b1, 2 * I, C, w1, bb1);
    f16* dX = up16(c, X, rows_in * C);
    f16* dR1 = r1_is_x ? dX : up16_opt(c, R1, rows_in * C);
    f16* dR2 = up16_opt(c, R2, rows_in * C);
    f16* dW1 = up16(c, w1.data(), (long)2 * I * C); f16* db1 = up16(c, bb1.data(), 2 * I);
    f16* dW2 = up16(c, W2, (long)C * I); f16* db2 = up16_opt(c, b2, C);
    f16* dg = up16_opt(c, gamma, C); f16* dbt = up16_opt(c, beta, C);
    const long nvec = addvec ? (M + rows_per_vec - 1) / rows_per_vec + (in_guard > 0 ? 1 : 0) : 0;
    f16* dav = up16_opt(c, addvec, nvec * C);
    f16* dO = up16(c, out_inout, (M + out_guard) * C);
    int grid = 0; long m1 = 0;
    if (mode == 3) {
      UG_REQUIRE(pre && beta && r1_is_x && max_wg == 0, "ug_op_ff_ex mode 3: the engine's ln_ff takes a pre-norm, the stream as residual and its own grid");
      m1 = test_ln_ff(c, dX, M, C, dg, dbt, eps, dav, rows_per_vec, dW1, db1, dW2, db2, dR2, c0, c1, c2, dO);
      if (m1 > 0) grid = ff_fused_grid(ff_fused(c, dX, (int)m1, C, dW1, db1, dW2, db2, dX, c0, c1, dO));
    } else {
      const f16* xin = dX; const f16* res = dR1;
      if (pre && mode != 2) {   // the LayerNorm launch the in-kernel form replaces: it writes the normalised rows and the stream x'
        UG_REQUIRE(beta && (!dav || !dR1 || dR1 == dX), "ug_op_ff_ex pre-norm: beta missing / residual is not the normalised stream");
        f16* t1 = c.ws.get<f16>((long)M * C); f16* xo = dav ? c.ws.get<f16>((long)M * C) : nullptr;
        LayerNormP l; memset(&l, 0, sizeof(l));
        l.X = dX; l.Y = t1; l.M = M; l.C = C; l.eps = eps; l.gamma = dg; l.beta = dbt; l.addvec = dav; l.rows_per_vec = rows_per_vec; l.Xout = xo;
        launch_layernorm(l, c.stream);
        xin = t1;
        if (dav && dR1) res = xo;
      }
      if (mode == 0) {
        UG_REQUIRE(!R2 && max_wg == 0, "ug_op_ff_ex mode 0: the two-launch path takes one residual and has no grid cap");
        ff_two_launch(c, xin, M, C, dW1, db1, dW2, db2, res, c0, c1, c.ws.get<f16>((long)M * I), dO);
      } else {
        FFusedP p = ff_fused(c, xin, M, C, dW1, db1, dW2, db2, res, c0, c1, dO);
        p.R2 = dR2; p.c2 = c2; p.max_wg = max_wg;
        if (pre && mode == 2) { p.ln_g = dg; p.ln_b = dbt; p.ln_eps = eps; p.addvec = dav; p.rows_per_vec = rows_per_vec; }
        launch_ff_fused(p, c.stream);
        grid = ff_fused_grid(p); m1 = M;
      }
    }
    down16(c, dO, out_inout, (M + out_guard) * C);
    if (info_out) { info_out[0] = grid; info_out[1] = grid ? (int)(((m1 + 127) / 128 + grid - 1) / grid) : 0; info_out[2] = (int)m1; }
  });
}

// what is left of the workspace above the current mark, filled with 0xFF (e8m0 NaN in every scale byte): what a product launch may find there
static void poison_rest(Ctx& c) {
  void* top = c.ws.alloc(0);
  UG_CHECK(hipMemsetAsync(top, 0xFF, c.ws.capacity() - c.ws.mark(), c.stream));
}

// The quantiser launch alone (tests/test_mx8_forms_gpu.py; the contract stands in include/unigeo_hip_test.h).
int ug_op_quant_mx8_ex(ug_ctx* x, const float* xin, int M, int K, long ldx, long guard, long ld_s, unsigned char* q_inout, unsigned* s_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(xin && q_inout && s_inout && M >= 1 && K >= 1 && ldx >= K && guard >= 0, "ug_op_quant_mx8_ex: arguments");
    UG_REQUIRE(K % 128 == 0 && ldx % 8 == 0 && ld_s >= M, "ug_op_quant_mx8_ex: the launcher's rules (checked before the caller's buffers are sized by them)");
    const long rows = M + guard;
    const size_t qb = (size_t)rows * K, sb = (size_t)(K / 128) * ld_s * 4;
    f16* dX = up16(c, xin, rows * ldx);
    unsigned char* q = (unsigned char*)c.ws.alloc(qb); unsigned* s = (unsigned*)c.ws.alloc(sb);
    UG_CHECK(hipMemcpy(q, q_inout, qb, hipMemcpyHostToDevice)); UG_CHECK(hipMemcpy(s, s_inout, sb, hipMemcpyHostToDevice));
    launch_quant_mx8(dX, ldx, M, K, q, s, ld_s, c.stream);
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(q_inout, q, qb, hipMemcpyDeviceToHost)); UG_CHECK(hipMemcpy(s_inout, s, sb, hipMemcpyDeviceToHost));
  });
}

// Every epilogue form of the MX-fp8 GEMM behind the two quantiser launches (the contract stands in include/unigeo_hip_test.h).
int ug_op_linear_mx8_ex(ug_ctx* x, const float* A, int M, int K, const float* W, int N, const float* bias, const float* R1, long ldr1, const float* R2, long ldr2,
                        float c0, float c1, float c2, int act, int geglu, long ldo, long guard, int poison, float* out_inout,
                        unsigned char* a8_out, unsigned* sa_out, int* plan_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int nout = geglu ? N / 2 : N;
    UG_REQUIRE(A && W && out_inout && M >= 1 && N >= 8 && K >= 1 && guard >= 0, "op_linear_mx8: arguments");
    UG_REQUIRE(K % 128 == 0 && N % 8 == 0, "op_linear_mx8: K % 128 == 0, N % 8 == 0");
    UG_REQUIRE(!geglu || N % 128 == 0, "op_linear_mx8: GEGLU needs N % 128 == 0");
    UG_REQUIRE(ldo >= nout && (!R1 || ldr1 >= nout) && (!R2 || ldr2 >= nout), "op_linear_mx8: rows narrower than the output");
    std::vector<float> Wp, bp;
    if (geglu) { pack_geglu(W, bias, N, K, Wp, bp); W = Wp.data(); if (bias) bias = bp.data(); }
    f16* dA = up16(c, A, (long)M * K); f16* dW = up16(c, W, (long)N * K);
    f16* db = up16_opt(c, bias, N);
    f16* dR1 = up16_opt(c, R1, (long)M * ldr1); f16* dR2 = up16_opt(c, R2, (long)M * ldr2);
    f16* dO = up16(c, out_inout, (M + guard) * ldo);
    const long ld_sa = (M + 255) / 256 * 256, ld_sw = (N + 255) / 256 * 256;
    if (poison) poison_rest(c);   // the four buffers below and everything above them: rows [M, ld_sa) / [N, ld_sw) of the scale areas then hold e8m0 NaN, as in the product
    unsigned char* a8 = (unsigned char*)c.ws.alloc((size_t)M * K); unsigned char* w8 = (unsigned char*)c.ws.alloc((size_t)N * K);
    unsigned* sw = (unsigned*)c.ws.alloc((size_t)(K / 128) * ld_sw * 4); unsigned* sa = (unsigned*)c.ws.alloc((size_t)(K / 128) * ld_sa * 4);
    launch_quant_mx8(dA, K, M, K, a8, sa, ld_sa, c.stream);
    launch_quant_mx8(dW, K, N, K, w8, sw, ld_sw, c.stream);
    GemmP p = dense_gemm(c, (const f16*)a8, M, K, (const f16*)w8, N, db, dO, ldo);
    p.R1 = dR1; p.ldr1 = ldr1; p.c1 = c1; p.R2 = dR2; p.ldr2 = ldr2; p.c2 = c2; p.c0 = c0; p.act = act;
    p.flags = geglu ? UG_F_GEGLU : 0;
    p.sa = sa; p.ld_sa = ld_sa; p.sw = sw; p.ld_sw = ld_sw;
    gemm_apply_tune(p, c.tune);
    launch_gemm_mx8(p, c.stream, plan_out);
    down16(c, dO, out_inout, (M + guard) * ldo);
    if (a8_out) UG_CHECK(hipMemcpy(a8_out, a8, (size_t)M * K, hipMemcpyDeviceToHost));
    if (sa_out) UG_CHECK(hipMemcpy(sa_out, sa, (size_t)(K / 128) * ld_sa * 4, hipMemcpyDeviceToHost));
  });
}

int ug_op_linear_mx8(ug_ctx* x, const float* A, int M, int K, const float* W, int N, const float* bias, int geglu, float* out,
                     unsigned char* a8_out, unsigned* sa_out) {
  return ug_op_linear_mx8_ex(x, A, M, K, W, N, bias, nullptr, 0, nullptr, 0, 1.f, 1.f, 1.f, 0, geglu, geglu ? N / 2 : N, 0, 0, out, a8_out, sa_out, nullptr);
}

// One linear layer through the engine's quant_lin() and linear() / ln_linear() over a 0xFF-filled workspace (the contract stands in include/unigeo_hip_test.h).
int ug_op_linear_engine(ug_ctx* x, const float* A, int M, long lda, const float* W, int N, int K, const float* bias, const float* gamma, const float* beta, float eps,
                        const float* R1, long ldr1, const float* R2, long ldr2, float c0, float c1, float c2, int act, int geglu, long ldo, long guard,
                        float* out_inout, int* info_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int nout = geglu ? N / 2 : N;
    UG_REQUIRE(A && W && out_inout && M >= 1 && N >= 8 && N % 8 == 0 && K >= 8 && K % 8 == 0 && guard >= 0, "ug_op_linear_engine: arguments");
    UG_REQUIRE(lda >= K && lda % 8 == 0 && ldo >= nout && (!R1 || ldr1 >= nout) && (!R2 || ldr2 >= nout), "ug_op_linear_engine: rows narrower than the matrix");
    UG_REQUIRE(!geglu || N % 128 == 0, "ug_op_linear_engine: GEGLU needs N % 128 == 0");
    UG_REQUIRE(!gamma || (beta && lda == K), "ug_op_linear_engine: the LayerNorm takes beta and tight rows");
    std::vector<float> Wp, bp;
    if (geglu) { pack_geglu(W, bias, N, K, Wp, bp); W = Wp.data(); if (bias) bias = bp.data(); }
    f16* dA = up16(c, A, (long)M * lda); f16* dW = up16(c, W, (long)N * K); f16* db = up16_opt(c, bias, N);
    f16* dg = up16_opt(c, gamma, K); f16* dbt = up16_opt(c, beta, K);
    f16* dR1 = up16_opt(c, R1, (long)M * ldr1); f16* dR2 = up16_opt(c, R2, (long)M * ldr2);
    f16* dO = up16(c, out_inout, (M + guard) * ldo);
    poison_rest(c);
    test_linear_engine(c, dA, M, lda == K ? 0 : lda, dW, db, K, N, dg, dbt, eps, dR1, ldr1, c1, dR2, ldr2, c2, c0, act, geglu ? UG_F_GEGLU : 0, dO,
                       ldo == nout ? 0 : ldo, info_out);
    down16(c, dO, out_inout, (M + guard) * ldo);
  });
}

int ug_op_conv(ug_ctx* x, const float* x0, int C0, const float* x1, int C1, int T, int H, int W, const float* weight,
               const float* bias, int O, int kt, int k, int stride, int pad_t, int pad_l, int ups, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int I = C0 + C1, taps = kt * k * k;
    const bool kch = (I % 64 == 0) && taps > 1 && !getenv("UG_NO_KCHUNK");     // the engine's chunk-major K order (GemmP::kchunk); UG_NO_KCHUNK: tap-major weights -> general path
    const std::vector<float> wp = pack_conv_weight(weight, O, I, taps, kch);
    const long px = (long)T * H * W;
    f16* d0 = up16(c, x0, px * C0); f16* d1 = C1 ? up16(c, x1, px * C1) : nullptr;
    f16* dW = up16(c, wp.data(), (long)wp.size()); f16* db = up16_opt(c, bias, O);
    const int Ho = H * ups / stride, Wo = W * ups / stride;
    f16* dO = c.ws.get<f16>((long)T * Ho * Wo * O);
    GemmP p = conv_gemm(c, d0, C0, d1, C1, T, H, W, kt, k, stride, pad_t, pad_l, ups, dW, O, db, dO);
    p.kchunk = kch;
    plan_gemm(c, p);
    launch_gemm(p, 1, c.stream);
    down16(c, dO, out, (long)T * Ho * Wo * O);
  });
}

// conv (3x3 pad 1, or (kt,1,1) temporal) + optional residual, then GroupNorm (+SiLU) of its output two ways: statistics pass over the stored tensor
// (y_pass) and statistics from the convolution's epilogue (GemmP::stat_part -> GroupNormP::part; y_epi).  rb_out: rows per statistics block the
// launch reported (0: the planner's kernel cannot, y_epi then equals y_pass by construction).  conv_out: the convolution's output (both runs: must be bit-identical).
int ug_op_conv_gn(ug_ctx* x, const float* x0, int C0, int T, int H, int W, const float* weight, const float* bias, const float* res, int O, int kt, int k,
                  int G, float eps, int temporal, const float* gamma, const float* beta, float* conv_out, float* y_pass, float* y_epi, int* rb_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int I = C0, taps = kt * k * k;
    UG_REQUIRE(I % 64 == 0, "ug_op_conv_gn: channels must be a multiple of 64");
    const std::vector<float> wp = pack_conv_weight(weight, O, I, taps, true);
    const long M = (long)T * H * W;
    f16* d0 = up16(c, x0, M * C0); f16* dW = up16(c, wp.data(), (long)wp.size()); f16* db = up16_opt(c, bias, O);
    f16* dR = up16_opt(c, res, M * O);
    f16* dg = up16(c, gamma, O); f16* dbt = up16(c, beta, O);
    f16* o1 = c.ws.get<f16>(M * O); f16* o2 = c.ws.get<f16>(M * O); f16* y1 = c.ws.get<f16>(M * O); f16* y2 = c.ws.get<f16>(M * O);
    float2* part = (float2*)c.ws.get<float>(((M + 47) / 48) * (long)O * 2);
    int rb = 0;
    for (int pass = 0; pass < 2; ++pass) {
      GemmP p = conv_gemm(c, d0, C0, nullptr, 0, T, H, W, kt, k, 1, k / 2, k / 2, 1, dW, O, db, pass ? o2 : o1);
      p.R1 = dR; p.ldr1 = O; p.c1 = 1.f; p.kchunk = taps > 1;
      const size_t mk = c.ws.mark();
      plan_gemm(c, p);
      if (pass) { p.stat_part = part; p.stat_hw = H * W; launch_gemm(p, 1, c.stream, &rb); } else launch_gemm(p, 1, c.stream);
      c.ws.release(mk);
      GroupNormP g; memset(&g, 0, sizeof(g));
      g.X0 = pass ? o2 : o1; g.C0 = O; g.T = T; g.HW = H * W; g.G = G; g.eps = eps; g.temporal = temporal; g.silu = 1; g.gamma = dg; g.beta = dbt;
      g.Y = pass ? y2 : y1; g.ws = c.ws.get<float>((long)groupnorm_ws_floats(T, H * W, O, G));
      if (pass && rb > 0) { g.part = part; g.part_rb = rb; }
      const bool used = launch_groupnorm(g, c.stream);
      if (pass && !used) rb = 0;              // the convolution wrote partial sums but GroupNorm took its slab / small form: report "no epilogue statistics"
      c.ws.release(mk);
    }
    *rb_out = rb;
    down16(c, o1, conv_out, M * O);
    std::vector<float> tmp((size_t)M * O);
    down16(c, o2, tmp.data(), M * O);
    UG_REQUIRE(memcmp(tmp.data(), conv_out, tmp.size() * 4) == 0, "ug_op_conv_gn: the statistics epilogue changed the convolution's output");
    down16(c, y1, y_pass, M * O); down16(c, y2, y_epi, M * O);
  });
}

// GroupNorm with the launch scheme forced (GroupNormP::mode) and the launcher's decision reported.  out_inout [T*HW + guard, C] goes to the device as the
// caller gives it and all of it comes back: the rows past T*HW must return unchanged (the slab kernel drops them through its buffer descriptor).
// plan_out [4]: scheme launched, slab threads, slab VMAX (0, 0 unless scheme 4 / 6), chunks per frame (0 unless scheme 1).
int ug_op_groupnorm_ex(ug_ctx* x, const float* x0, int C0, const float* x1, int C1, int T, int HW, int G, float eps,
                       int temporal, int silu, const float* gamma, const float* beta, int mode, long guard, float* out_inout, int* plan_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(T >= 1 && HW >= 1 && G >= 1 && C0 >= 1 && C1 >= 0 && guard >= 0 && x0 && (C1 == 0 || x1) && out_inout, "groupnorm shape");
    const int C = C0 + C1; const long M = (long)T * HW;
    GroupNormP p; memset(&p, 0, sizeof(p));
    p.X0 = up16(c, x0, M * C0); p.X1 = C1 ? up16(c, x1, M * C1) : nullptr; p.C0 = C0; p.C1 = C1;
    p.T = T; p.HW = HW; p.G = G; p.eps = eps; p.temporal = temporal; p.silu = silu; p.mode = mode;
    p.gamma = up16(c, gamma, C); p.beta = up16(c, beta, C);
    f16* y = guard ? up16(c, out_inout, (M + guard) * C) : c.ws.get<f16>(M * C); p.Y = y;
    p.ws = c.ws.get<float>((long)groupnorm_ws_floats(T, HW, C, G));
    launch_groupnorm(p, c.stream);
    if (plan_out) { const GnPlan pl = groupnorm_plan(p); plan_out[0] = pl.mode; plan_out[1] = pl.nt; plan_out[2] = pl.vmax; plan_out[3] = pl.nchunk; }
    down16(c, y, out_inout, (M + guard) * C);
  });
}

int ug_op_groupnorm(ug_ctx* x, const float* x0, int C0, const float* x1, int C1, int T, int HW, int G, float eps,
                    int temporal, int silu, const float* gamma, const float* beta, float* out) {
  return ug_op_groupnorm_ex(x, x0, C0, x1, C1, T, HW, G, eps, temporal, silu, gamma, beta, 0, 0, out, nullptr);
}

// LayerNorm with the row offset of the pre-add (LayerNormP::row0), the kernel forced (form 1: ln_kernel also at C = 320 / 640 / 1280) and reported
// (*form_out: L for ln40_kernel<L>, -VPL for ln_kernel<VPL>).  out_inout [M + guard, C] goes up as given and all of it comes back.  y8_out / s8_out: the same
// launch again with the MX-fp8 output pair -> bytes [M][C] and scale dwords [C/128][round_up(M,256)] (ug_op_linear_mx8's layout; the buffer is zeroed first,
// so the dwords of rows >= M come back 0).
int ug_op_layernorm_ex(ug_ctx* x, const float* xin, int M, int C, float eps, const float* gamma, const float* beta,
                       const float* addvec, int rows_per_vec, long row0, int form, long guard, float* out_inout, float* xout,
                       unsigned char* y8_out, unsigned* s8_out, int* form_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(M >= 1 && C >= 8 && row0 >= 0 && guard >= 0 && xin && out_inout && (!addvec || rows_per_vec >= 1) && !y8_out == !s8_out, "layernorm arguments");
    LayerNormP p; memset(&p, 0, sizeof(p));
    p.X = up16(c, xin, (long)M * C); p.M = M; p.C = C; p.eps = eps; p.gamma = up16(c, gamma, C); p.beta = up16(c, beta, C);
    p.row0 = row0; p.form = form;
    f16* y = guard ? up16(c, out_inout, (M + guard) * C) : c.ws.get<f16>((long)M * C); p.Y = y;
    f16* xo = nullptr;
    if (addvec) {
      const long nv = (M + row0 + rows_per_vec - 1) / rows_per_vec;
      p.addvec = up16(c, addvec, nv * C); p.rows_per_vec = rows_per_vec;
      xo = c.ws.get<f16>((long)M * C); p.Xout = xo;
    }
    launch_layernorm(p, c.stream);
    if (form_out) *form_out = layernorm_form(p);
    down16(c, y, out_inout, (M + guard) * C);
    if (xo && xout) down16(c, xo, xout, (long)M * C);
    if (y8_out) {
      UG_REQUIRE(C % 128 == 0, "layernorm MX-fp8 output: C % 128 == 0");
      const long ld = ((long)M + 255) / 256 * 256;
      const size_t sbytes = (size_t)(C / 128) * ld * 4;
      unsigned char* y8 = (unsigned char*)c.ws.alloc((size_t)M * C); unsigned* s8 = (unsigned*)c.ws.alloc(sbytes);
      UG_CHECK(hipMemsetAsync(s8, 0, sbytes, c.stream));
      p.Y = nullptr; p.Xout = nullptr; p.Y8 = y8; p.S8 = s8; p.ld_s8 = ld;
      launch_layernorm(p, c.stream);
      UG_CHECK(hipStreamSynchronize(c.stream));
      UG_CHECK(hipMemcpy(y8_out, y8, (size_t)M * C, hipMemcpyDeviceToHost));
      UG_CHECK(hipMemcpy(s8_out, s8, sbytes, hipMemcpyDeviceToHost));
    }
  });
}

int ug_op_layernorm(ug_ctx* x, const float* xin, int M, int C, float eps, const float* gamma, const float* beta,
                    const float* addvec, int rows_per_vec, float* out, float* xout) {
  return ug_op_layernorm_ex(x, xin, M, C, eps, gamma, beta, addvec, rows_per_vec, 0, 0, 0, out, xout, nullptr, nullptr, nullptr);
}

int ug_op_flash_attn(ug_ctx* x, const float* qkv, int B, int H, int S, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int C = H * 64; const long M = (long)B * S;
    f16* d = up16(c, qkv, M * 3 * C); f16* o = c.ws.get<f16>(M * C);
    FlashP p; p.Q = d; p.K = d + C; p.V = d + 2 * C; p.ldq = p.ldk = p.ldv = 3 * C; p.O = o; p.ldo = C; p.variant = c.flash_variant;
    p.B = B; p.H = H; p.S = S; p.scale = 0.125f;
    launch_flash_attn64(p, c.stream);
    down16(c, o, out, M * C);
  });
}

int ug_op_temporal_attn(ug_ctx* x, const float* qkv, int T, int HW, int H, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int C = H * 64; const long M = (long)T * HW;
    f16* d = up16(c, qkv, M * 3 * C); f16* o = c.ws.get<f16>(M * C);
    TemporalAttnP p; p.Q = d; p.K = d + C; p.V = d + 2 * C; p.ld = 3 * C; p.O = o; p.ldo = C;
    p.T = T; p.HW = HW; p.H = H; p.scale = 0.125f;
    launch_temporal_attn64(p, c.stream);
    down16(c, o, out, M * C);
  });
}

// the launch forms of launch_flash_attn64 that ug_op_flash_attn cannot reach: Sk != 0 / kv_shared with separate row strides, K and V in one buffer.
// Everything the caller hands over goes to the device and all of out_inout comes back, so a test can poison what the kernel must not read and
// plant sentinels where it must not write.
int ug_op_flash_cross_attn(ug_ctx* x, const float* q, const float* kv, int B, int H, int S, int Sk, int kv_shared, long ldq, long ldkv, long ldo,
                           long guard, float* out_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const long C = (long)H * 64;
    UG_REQUIRE(B >= 1 && H >= 1 && S >= 1 && Sk >= 0 && guard >= 0 && q && kv && out_inout, "flash cross-attention shape");
    UG_REQUIRE(ldq >= C && ldkv >= 2 * C && ldo >= C, "flash cross-attention: rows narrower than the heads");
    UG_REQUIRE(ldq % 8 == 0 && ldkv % 8 == 0 && ldo % 4 == 0, "flash cross-attention strides");
    const long keys = Sk ? Sk : S;
    const long rows_q = (long)B * S, rows_kv = (kv_shared ? 1 : B) * keys + guard, rows_o = rows_q + guard;
    f16* dq = up16(c, q, rows_q * ldq); f16* dkv = up16(c, kv, rows_kv * ldkv); f16* o = up16(c, out_inout, rows_o * ldo);
    FlashP p; p.Q = dq; p.K = dkv; p.V = dkv + C; p.ldq = ldq; p.ldk = p.ldv = ldkv; p.O = o; p.ldo = ldo; p.variant = c.flash_variant;
    p.B = B; p.H = H; p.S = S; p.scale = 0.125f; p.Sk = Sk; p.kv_shared = kv_shared ? 1 : 0;
    launch_flash_attn64(p, c.stream);
    down16(c, o, out_inout, rows_o * ldo);
  });
}

// ug_op_temporal_attn over nv videos stacked [nv][T][HW] (TemporalAttnP::nv, grid dimension z: the guided UNet pass)
int ug_op_temporal_attn_nv(ug_ctx* x, const float* qkv, int nv, int T, int HW, int H, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(nv >= 1 && T >= 1 && HW >= 1 && H >= 1, "temporal attention shape");
    const int C = H * 64; const long M = (long)nv * T * HW;
    f16* d = up16(c, qkv, M * 3 * C); f16* o = c.ws.get<f16>(M * C);
    TemporalAttnP p; p.Q = d; p.K = d + C; p.V = d + 2 * C; p.ld = 3 * C; p.O = o; p.ldo = C;
    p.T = T; p.HW = HW; p.H = H; p.scale = 0.125f; p.nv = nv;
    launch_temporal_attn64(p, c.stream);
    down16(c, o, out, M * C);
  });
}

// The two attention paths for head dims other than 64 on packed qkv [B*S + guard, ld] (Q | K | V in columns [0, 3*H*d)) with the conventions of
// ug_op_flash_cross_attn: everything the caller hands over goes to the device as given and all of out_inout [B*S + guard, ldo] comes back.
static void attn_general_shape(int B, int S, int H, int d, long ld, long ldo, long guard, const float* qkv, const float* out) {
  UG_REQUIRE(B >= 1 && S >= 1 && H >= 1 && d >= 1 && guard >= 0 && qkv && out, "attention shape");
  UG_REQUIRE(ld >= 3L * H * d && ldo >= (long)H * d, "attention: rows narrower than the heads");
  UG_REQUIRE(ld % 8 == 0 && ldo % 4 == 0, "attention strides");
}

int ug_op_attention_generic_ex(ug_ctx* x, const float* qkv, int B, int S, int H, int d, long ld, long ldo, long guard, float* out_inout, int* plan_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    attn_general_shape(B, S, H, d, ld, ldo, guard, qkv, out_inout);
    UG_REQUIRE(d % 8 == 0, "unfused attention: head dim a multiple of 8");
    const long rows = (long)B * S + guard;
    f16* dq = up16(c, qkv, rows * ld); f16* o = up16(c, out_inout, rows * ldo);
    std::vector<int> plan;
    test_unfused_attention(c, dq, ld, B, S, H, d, o, ldo, &plan);
    down16(c, o, out_inout, rows * ldo);
    if (plan_out) for (int i = 0; i < 4; ++i) plan_out[i] = i < (int)plan.size() ? plan[i] : -1;
  });
}

int ug_op_flash_attn_dh_ex(ug_ctx* x, const float* qkv, int B, int S, int H, int d, long ld, long ldo, long guard, float* out_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    attn_general_shape(B, S, H, d, ld, ldo, guard, qkv, out_inout);
    const long C = (long)H * d, rows = (long)B * S + guard;
    f16* dq = up16(c, qkv, rows * ld); f16* o = up16(c, out_inout, rows * ldo);
    FlashP p; p.variant = c.flash_variant; p.Q = dq; p.K = dq + C; p.V = dq + 2 * C; p.ldq = p.ldk = p.ldv = ld; p.O = o; p.ldo = ldo; p.B = B; p.H = H; p.S = S;
    p.scale = 1.0f / sqrtf((float)d);
    launch_flash_attn_dh(p, d, c.stream);
    down16(c, o, out_inout, rows * ldo);
  });
}

int ug_op_attention_generic(ug_ctx* x, const float* qkv, int B, int S, int H, int d, float* out) {
  return ug_op_attention_generic_ex(x, qkv, B, S, H, d, 3L * H * d, (long)H * d, 0, out, nullptr);
}

int ug_op_flash_attn_dh(ug_ctx* x, const float* qkv, int B, int S, int H, int d, float* out) {
  return ug_op_flash_attn_dh_ex(x, qkv, B, S, H, d, 3L * H * d, (long)H * d, 0, out);
}

// One batched GEMM as unfused_attention launches its two: Out[b] = c0 * A[b] W[b]^T, batch b = (bo, bi) = (b / nb_inner, b % nb_inner) at element offsets
// bo * s?_o + bi * s?_i of A (rows of lda), W (rows of ldw) and the output (rows of ldo; float32 with out_f32, else fp16).  The buffers have the sizes the
// caller gives; that the last element every batch addresses lies inside them is checked here, on the host.
static float* up32g(Ctx& c, const float* h, long n);
static void down32g(Ctx& c, const float* d, float* h, long n);
static void batched_extent(const char* what, long rows, long ld, long cols, int batch, int nb_inner, long s_o, long s_i, long elems) {
  UG_REQUIRE(ld >= 0 && s_o >= 0 && s_i >= 0, what);
  const long last = (long)((batch - 1) / nb_inner) * s_o + (long)(std::min(batch, nb_inner) - 1) * s_i + (rows - 1) * ld + cols - 1;
  UG_REQUIRE(last < elems, what);
}

int ug_op_gemm_batched(ug_ctx* x, const float* A, long lda, long sA_o, long sA_i, const float* W, long ldw, long sW_o, long sW_i, int M, int N, int K,
                       int batch, int nb_inner, float c0, int out_f32, long ldo, long sO_o, long sO_i, long a_elems, long w_elems, long o_elems,
                       float* out_inout, int* plan_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(A && W && out_inout && M >= 1 && N >= 1 && K >= 1 && batch >= 1 && nb_inner >= 1 && batch % nb_inner == 0, "batched GEMM shape");
    UG_REQUIRE(lda <= 0x7fffffffL, "batched GEMM: lda");
    batched_extent("batched GEMM: A leaves its buffer", M, lda, K, batch, nb_inner, sA_o, sA_i, a_elems);
    batched_extent("batched GEMM: W leaves its buffer", N, ldw, K, batch, nb_inner, sW_o, sW_i, w_elems);
    batched_extent("batched GEMM: the output leaves its buffer", M, ldo, N, batch, nb_inner, sO_o, sO_i, o_elems);
    f16* dA = up16(c, A, a_elems); f16* dW = up16(c, W, w_elems);
    void* dO = out_f32 ? (void*)up32g(c, out_inout, o_elems) : (void*)up16(c, out_inout, o_elems);
    GemmP p; memset(&p, 0, sizeof(p));
    p.A0 = dA; p.C0 = (int)lda; p.M = M; p.N = N; p.K = K; p.W = dW; p.ldw = ldw; p.c0 = c0; p.Out = dO; p.ldo = ldo;
    p.flags = out_f32 ? UG_F_OUT_F32 : 0;
    p.nb_inner = nb_inner; p.sA_o = sA_o; p.sA_i = sA_i; p.sW_o = sW_o; p.sW_i = sW_i; p.sO_o = sO_o; p.sO_i = sO_i;
    std::vector<int> plan;
    test_run_gemm(c, p, batch, &plan);
    if (out_f32) down32g(c, (const float*)dO, out_inout, o_elems); else down16(c, (const f16*)dO, out_inout, o_elems);
    if (plan_out) for (int i = 0; i < 2; ++i) plan_out[i] = i < (int)plan.size() ? plan[i] : -1;
  });
}

int ug_op_euler_step(ug_ctx* x, const float* v, float* lat, long n, float sigma, float sigma_next) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    f16* dv = up16(c, v, n); f16* dl = up16(c, lat, n);
    launch_euler_step(dv, dl, n, sigma, sigma_next, c.stream);
    down16(c, dl, lat, n);
  });
}

// ---- the float32-grade VAE encoder's kernels (kernels/wide.hip; res2d_wide / vattn_wide of engine.hip): float32 in, float32 out, nothing rounded to fp16 on the way in
static float* up32(Ctx& c, const float* h, long n) {
  float* d = c.ws.get<float>(n);
  UG_CHECK(hipMemcpy(d, h, (size_t)n * 4, hipMemcpyHostToDevice));
  return d;
}
static void down32(Ctx& c, const float* d, float* h, long n) {
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(h, d, (size_t)n * 4, hipMemcpyDeviceToHost));
}
// pair tensor [M][2C] = [hi | lo] f16 device -> hi [M][C], lo [M][C] float host
static void down_pair(Ctx& c, const f16* d, float* hi, float* lo, long M, int C) {
  std::vector<f16> v((size_t)M * 2 * C);
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(v.data(), d, v.size() * 2, hipMemcpyDeviceToHost));
  for (long m = 0; m < M; ++m)
    for (int ch = 0; ch < C; ++ch) { hi[m * C + ch] = (float)v[(size_t)m * 2 * C + ch]; lo[m * C + ch] = (float)v[(size_t)m * 2 * C + C + ch]; }
}
struct BindScope {   // what a test entry binds leaves the context again on every way out: the bound copies (bind_conv, dup_conv) in c.persist, the raw tensors under `prefix`
  Ctx& c; size_t mk; std::string prefix;
  BindScope(Ctx& c_, const std::string& prefix_) : c(c_), mk(c_.persist.mark()), prefix(prefix_) {}
  ~BindScope() {
    (void)hipStreamSynchronize(c.stream); c.persist.release(mk);
    for (auto it = c.raw.begin(); it != c.raw.end();) {
      if (it->first.compare(0, prefix.size(), prefix) == 0) { (void)hipFree(it->second.dev); it = c.raw.erase(it); } else ++it;
    }
  }
};

int ug_op_split_pair(ug_ctx* x, const float* xin, long M, int C, float* hi, float* lo) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(M >= 1 && C >= 4, "ug_op_split_pair: empty tensor");
    f16* y = c.ws.get<f16>(M * 2 * C);
    launch_split_pair(up32(c, xin, M * C), y, M, C, c.stream);
    down_pair(c, y, hi, lo, M, C);
  });
}
int ug_op_gn32_pair(ug_ctx* x, const float* xin, int T, int HW, int C, int G, float eps, int silu, const float* gamma, const float* beta, float* hi, float* lo) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const long M = (long)T * HW;
    const float* dx = up32(c, xin, M * C);
    f16* dg = up16(c, gamma, C); f16* db = up16(c, beta, C);
    f16* y = c.ws.get<f16>(M * 2 * C);
    void* ws = c.ws.alloc(gn32_ws_bytes(T, HW, C, G));
    launch_gn32_pair(dx, y, T, HW, C, G, eps, silu, dg, db, ws, c.stream);
    down_pair(c, y, hi, lo, M, C);
  });
}
int ug_op_conv_wide(ug_ctx* x, const float* xin, int T, int H, int W, int C, const float* weight, const float* bias, int O, const float* res, int res_in_place,
                    int k, int stride, int pad_t, int pad_l, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c); BindScope bs(c, "op_conv_wide.");
    UG_REQUIRE(stride >= 1 && H % stride == 0 && W % stride == 0, "ug_op_conv_wide: stride must divide the frame");
    UG_REQUIRE(!res_in_place || res, "ug_op_conv_wide: res_in_place needs a residual");
    const std::string name = "op_conv_wide.conv";
    upload_raw(c, name + ".weight", 1, {O, C, k, k}, weight);
    if (bias) upload_raw(c, name + ".bias", 1, {O}, bias);
    const long Mo = (long)T * (H / stride) * (W / stride);
    const float* dx = up32(c, xin, (long)T * H * W * C);
    float* dO = c.ws.get<float>(Mo * O);
    const float* dR = nullptr;
    if (res && res_in_place) { UG_CHECK(hipMemcpy(dO, res, (size_t)Mo * O * 4, hipMemcpyHostToDevice)); dR = dO; }   // res2d_wide with a shortcut: the residual is the output buffer
    else if (res) dR = up32(c, res, Mo * O);
    test_conv_wide(c, name, bias != nullptr, dx, T, H, W, C, O, k, stride, pad_t, pad_l, dO, dR);
    finish_binding(c, "op_conv_wide.");   // both tensors were used
    down32(c, dO, out, Mo * O);
  });
}
// ---- one convolution bound on the device and launched by the engine's conv(), as every convolution of the models is (tests/test_conv_bound_gpu.py).
// The raw checkpoint-layout weight goes through bind_conv (k_permute_conv_w, k_rechunk_conv_w, k_upsample_phase_w), not through pack_conv_weight.
static Conv bind_op_conv(Ctx& c, const std::string& name, const float* weight, const float* bias, int cin, int O, int kt, int k, int upsampler) {
  UG_REQUIRE(weight && cin >= 1 && O >= 1 && k >= 1 && (kt == 1 || (kt == 3 && k == 1)), "bound conv: weight [O][cin][k][k] or [O][cin][3][1][1]");
  if (kt > 1) upload_raw(c, name + ".weight", 1, {O, cin, kt, 1, 1}, weight);
  else upload_raw(c, name + ".weight", 1, {O, cin, k, k}, weight);
  if (bias) upload_raw(c, name + ".bias", 1, {O}, bias);
  return test_bind_conv(c, name, cin, O, kt, k, bias != nullptr, upsampler != 0);
}
int ug_op_bind_conv(ug_ctx* x, const float* weight, const float* bias, int cin, int O, int kt, int k, int upsampler,
                    float* w_out, float* wphase_out, int* info_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c); BindScope bs(c, "op_bind_conv.");
    UG_REQUIRE(w_out && info_out, "ug_op_bind_conv: w_out and info_out must not be NULL");
    const Conv cv = bind_op_conv(c, "op_bind_conv.conv", weight, bias, cin, O, kt, k, upsampler);
    finish_binding(c, "op_bind_conv.");
    info_out[0] = cv.cinp; info_out[1] = cv.kchunk; info_out[2] = cv.wphase != nullptr;
    down16(c, cv.w, w_out, (long)O * kt * k * k * cv.cinp);
    if (cv.wphase && wphase_out) down16(c, cv.wphase, wphase_out, (long)4 * O * 4 * cv.cinp);
  });
}
int ug_op_conv_bound(ug_ctx* x, const float* weight, const float* bias, int cin, int O, int kt, int k, int upsampler,
                     const float* x0, int C0, const float* x1, int C1, int T, int H, int W, int stride, int pad_t, int pad_l, int ups,
                     const float* R1, float c0, float c1, int act, long ldo, long guard, float* out_inout, int* plan_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c); BindScope bs(c, "op_conv_bound.");
    UG_REQUIRE(x0 && out_inout && T >= 1 && H >= 1 && W >= 1 && guard >= 0 && C0 >= 1 && C1 >= 0 && (C1 == 0 || x1), "ug_op_conv_bound: shape");
    UG_REQUIRE((ups == 1 || ups == 2) && stride >= 1 && (H * ups) % stride == 0 && (W * ups) % stride == 0, "ug_op_conv_bound: stride must divide the frame");
    UG_REQUIRE(ldo >= O, "ug_op_conv_bound: rows narrower than the output channels");
    const Conv cv = bind_op_conv(c, "op_conv_bound.conv", weight, bias, cin, O, kt, k, upsampler);
    finish_binding(c, "op_conv_bound.");
    const long px = (long)T * H * W, rows = (long)T * (H * ups / stride) * (W * ups / stride);
    const f16* d0 = up16(c, x0, px * C0); const f16* d1 = C1 ? up16(c, x1, px * C1) : nullptr;
    if (cin % 8 != 0) {      // a source narrower than the bound weight's padded channel count: zero channels behind it, as the VAE decoder does for its latent
      UG_REQUIRE(C1 == 0 && C0 == cin, "ug_op_conv_bound: cin % 8 != 0 takes one source of cin channels");
      f16* dp = c.ws.get<f16>(px * cv.cinp);
      launch_pad_channels(d0, cin, dp, cv.cinp, px, c.stream);
      d0 = dp; C0 = cv.cinp;
    }
    UG_REQUIRE(C0 % 8 == 0 && C1 % 8 == 0 && C0 + C1 == cv.cinp, "ug_op_conv_bound: C0 + C1 must be the bound channel count, each a multiple of 8");
    const f16* dR = up16_opt(c, R1, rows * O);
    f16* dO = up16(c, out_inout, (rows + guard) * ldo);
    std::vector<int> plan;
    test_conv_bound(c, cv, d0, C0, d1, C1, T, H, W, stride, pad_t, pad_l, ups, dR, c0, c1, act, dO, ldo, &plan);
    UG_REQUIRE(plan.size() == 2 || plan.size() == 8, "ug_op_conv_bound: one launch, or the four phase launches");
    if (plan_out) { plan_out[0] = (int)plan.size() / 2; for (size_t i = 0; i < 8; ++i) plan_out[1 + i] = i < plan.size() ? plan[i] : -1; }
    down16(c, dO, out_inout, (rows + guard) * ldo);
  });
}
// ---- the epilogue operands of the graphs - bias2, R1 / c1, R2 / c2, c0, act - on the engine's linear() and conv() (tests/test_epilogue_forms_gpu.py; the
// contract stands in include/unigeo_hip_test.h)
static TestEpi upload_epi(Ctx& c, const float* bias2, int N, const float* R1, long ldr1, const float* R2, long ldr2, long rows, float c0, float c1, float c2, int act) {
  TestEpi e;
  e.bias2 = up16_opt(c, bias2, N);
  e.R1 = up16_opt(c, R1, rows * ldr1); e.ldr1 = R1 ? ldr1 : 0; e.c1 = c1;
  e.R2 = up16_opt(c, R2, rows * ldr2); e.ldr2 = R2 ? ldr2 : 0; e.c2 = c2;
  e.c0 = c0; e.act = act;
  return e;
}
int ug_op_linear_ex(ug_ctx* x, const float* A, int M, long lda, const float* W, int N, int K, const float* bias, const float* bias2,
                    const float* R1, long ldr1, const float* R2, long ldr2, float c0, float c1, float c2, int act, int geglu,
                    long ldo, long guard, float* out_inout, int* plan_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int nout = geglu ? N / 2 : N;
    UG_REQUIRE(!c.fp8_linears, "ug_op_linear_ex: the fp16 path only - the context has fp8_linears set");
    UG_REQUIRE(A && W && out_inout && M >= 1 && N >= 1 && K >= 8 && K % 8 == 0 && guard >= 0 && act >= 0 && act <= 2, "ug_op_linear_ex: arguments");
    UG_REQUIRE(lda >= K && lda % 8 == 0 && ldo >= nout && (!R1 || ldr1 >= nout) && (!R2 || ldr2 >= nout), "ug_op_linear_ex: rows narrower than the matrix");
    UG_REQUIRE(!geglu || N % 128 == 0, "ug_op_linear_ex: GEGLU needs N % 128 == 0");
    std::vector<float> Wp, bp, Wq, b2p;
    if (geglu) {     // checkpoint order [value | gate] -> the bound row order, bias2 with the rows it belongs to
      pack_geglu(W, bias, N, K, Wp, bp);
      if (bias2) { pack_geglu(W, bias2, N, K, Wq, b2p); bias2 = b2p.data(); }
      W = Wp.data(); if (bias) bias = bp.data();
    }
    f16* dA = up16(c, A, (long)M * lda); f16* dW = up16(c, W, (long)N * K); f16* db = up16_opt(c, bias, N);
    TestEpi e = upload_epi(c, bias2, N, R1, ldr1, R2, ldr2, M, c0, c1, c2, act);
    e.flags = geglu ? UG_F_GEGLU : 0;
    f16* dO = up16(c, out_inout, (M + guard) * ldo);
    std::vector<int> plan, launched;
    test_linear_epi(c, dA, M, lda == K ? 0 : lda, dW, db, K, N, e, dO, ldo == nout ? 0 : ldo, &plan, &launched);
    UG_REQUIRE(plan.size() == 2 && launched.size() == 1, "ug_op_linear_ex: one GEMM launch");
    if (plan_out) { plan_out[0] = launched[0]; plan_out[1] = plan[1]; }
    down16(c, dO, out_inout, (M + guard) * ldo);
  });
}
int ug_op_conv_epi(ug_ctx* x, const float* weight, const float* bias, int cin, int O, int kt, int k,
                   const float* x0, int C0, const float* x1, int C1, int T, int H, int W, int stride, int pad_t, int pad_l,
                   const float* bias2, const float* R1, long ldr1, const float* R2, long ldr2, float c0, float c1, float c2, int act,
                   long ldo, long guard, float* out_inout, int want_stats, float* stat_inout, int* rb_out, int* plan_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c); BindScope bs(c, "op_conv_epi.");
    UG_REQUIRE(x0 && out_inout && T >= 1 && H >= 1 && W >= 1 && guard >= 0 && C0 >= 8 && C1 >= 0 && (C1 == 0 || x1) && act >= 0 && act <= 2, "ug_op_conv_epi: shape");
    UG_REQUIRE((stride == 1 || stride == 2) && H % stride == 0 && W % stride == 0, "ug_op_conv_epi: stride 1 or 2, dividing the frame");
    UG_REQUIRE(C0 % 8 == 0 && C1 % 8 == 0 && C0 + C1 == cin, "ug_op_conv_epi: C0 + C1 must be cin, each a multiple of 8");
    UG_REQUIRE(ldo >= O && (!R1 || ldr1 >= O) && (!R2 || ldr2 >= O), "ug_op_conv_epi: rows narrower than the output channels");
    UG_REQUIRE(!want_stats || (stat_inout && rb_out), "ug_op_conv_epi: want_stats needs stat_inout and rb_out");
    const Conv cv = bind_op_conv(c, "op_conv_epi.conv", weight, bias, cin, O, kt, k, 0);
    finish_binding(c, "op_conv_epi.");
    const long px = (long)T * H * W, rows = (long)T * (H / stride) * (W / stride);
    const f16* d0 = up16(c, x0, px * C0); const f16* d1 = C1 ? up16(c, x1, px * C1) : nullptr;
    const TestEpi e = upload_epi(c, bias2, O, R1, ldr1, R2, ldr2, rows, c0, c1, c2, act);
    f16* dO = up16(c, out_inout, (rows + guard) * ldo);
    const long nstat = ((rows + 47) / 48) * (long)O * 2;     // floats: one float2 per (block of >= 48 rows, channel), as stat_alloc sizes the area
    float* dS = want_stats ? up32g(c, stat_inout, nstat) : nullptr;
    std::vector<int> plan, launched;
    const int rb = test_conv_epi(c, cv, d0, C0, d1, C1, T, H, W, stride, pad_t, pad_l, e, (float2*)dS, dO, ldo == O ? 0 : ldo, &plan, &launched);
    UG_REQUIRE(plan.size() == 2 && launched.size() == 1, "ug_op_conv_epi: one GEMM launch");
    if (plan_out) { plan_out[0] = launched[0]; plan_out[1] = plan[1]; }
    if (rb_out) *rb_out = rb;
    down16(c, dO, out_inout, (rows + guard) * ldo);
    if (want_stats) down32g(c, dS, stat_inout, nstat);
  });
}
int ug_op_attn_wide(ug_ctx* x, const float* qkv, int T, int S, int C, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const long M = (long)T * S;
    const float* dq = up32(c, qkv, M * 3 * C);
    float* dO = c.ws.get<float>(M * C);
    attn_wide_core(c, dq, T, S, C, dO);
    down32(c, dO, out, M * C);
  });
}

// ---- clip inputs made on the device (kernels/noise.hip): op-level entry points of the parity tests
int ug_op_philox_u32(ug_ctx* x, uint64_t seed, uint32_t stream, uint64_t block_offset, long nblocks, uint32_t* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(nblocks >= 1 && out, "nblocks >= 1 and an output buffer");
    uint32_t* d = c.ws.get<uint32_t>(nblocks * 4);
    launch_philox_u32(d, nblocks, seed, stream, block_offset, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(out, d, (size_t)nblocks * 16, hipMemcpyDeviceToHost));
  });
}
int ug_op_randn(ug_ctx* x, uint64_t seed, uint32_t stream, uint64_t element_offset, long n, long guard, float* inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(n >= 1 && guard >= 0 && inout, "n >= 1, guard >= 0 and a buffer of n + guard floats");
    float* d = c.ws.get<float>(n + guard);
    UG_CHECK(hipMemcpy(d, inout, (size_t)(n + guard) * 4, hipMemcpyHostToDevice));
    launch_randn(d, n, seed, stream, element_offset, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(inout, d, (size_t)(n + guard) * 4, hipMemcpyDeviceToHost));
  });
}
int ug_op_u8_to_frames(ug_ctx* x, const unsigned char* frames_tchw, int T, int H, int W, float* out_thwc) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(T >= 1 && H >= 1 && W >= 1 && ((long)H * W) % 4 == 0, "H * W must be a multiple of 4");
    const long px = (long)T * H * W;
    unsigned char* d8 = c.ws.get<unsigned char>(px * 3); float* df = c.ws.get<float>(px * 3);
    UG_CHECK(hipMemcpy(d8, frames_tchw, (size_t)px * 3, hipMemcpyHostToDevice));
    launch_u8_to_frames(d8, df, T, (long)H * W, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(out_thwc, df, (size_t)px * 12, hipMemcpyDeviceToHost));
  });
}

// ---- the pipeline glue of kernels/misc.hip one launch at a time (tests/test_glue_gpu.py).  Each entry calls the product's launch_* on the context's
// stream and nothing else; every output buffer goes to the device as the caller gives it, guard rows included, and all of it comes back.
static float* up32g(Ctx& c, const float* h, long n) {      // float32 host -> float32 device, as given
  float* d = c.ws.get<float>(n);
  UG_CHECK(hipMemcpy(d, h, (size_t)n * 4, hipMemcpyHostToDevice));
  return d;
}
static void down32g(Ctx& c, const float* d, float* h, long n) {
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(h, d, (size_t)n * 4, hipMemcpyDeviceToHost));
}
int ug_op_clip_patchify(ug_ctx* x, const float* video_m11, int T, int H, int W, int S, int P, int Kpad, int imagenet_norm, long guard, float* out_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(T >= 1 && H >= 1 && W >= 1 && S >= 1 && P >= 1 && S % P == 0 && Kpad >= 3 * P * P && guard >= 0 && video_m11 && out_inout, "clip patchify shape");
    const long rows = (long)T * (S / P) * (S / P);
    const f16* src = up16(c, video_m11, (long)T * H * W * 3);
    f16* out = up16(c, out_inout, (rows + guard) * Kpad);
    launch_clip_patchify(src, out, T, H, W, S, P, Kpad, c.stream, imagenet_norm);
    UG_CHECK(hipGetLastError());
    down16(c, out, out_inout, (rows + guard) * Kpad);
  });
}
int ug_op_prep_video(ug_ctx* x, const float* frames, const float* noise, int T, int H, int W, float aug, long guard, float* clip_src_inout, float* vae_in_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(T >= 1 && H >= 1 && W >= 1 && guard >= 0 && frames && noise && clip_src_inout && vae_in_inout, "prep video shape");
    const long px = (long)T * H * W;
    const float* df = up32g(c, frames, px * 3); const float* dn = up32g(c, noise, px * 3);
    f16* src = up16(c, clip_src_inout, (px + guard) * 3); f16* vin = up16(c, vae_in_inout, (px + guard) * 8);
    launch_prep_video(df, dn, src, vin, T, H, W, aug, c.stream);
    UG_CHECK(hipGetLastError());
    down16(c, src, clip_src_inout, (px + guard) * 3); down16(c, vin, vae_in_inout, (px + guard) * 8);
  });
}
int ug_op_init_latents(ug_ctx* x, const float* noise_tchw, int T, long hw, float sigma0, long guard, float* lat_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(T >= 1 && hw >= 1 && guard >= 0 && noise_tchw && lat_inout, "init latents shape");
    const long px = (long)T * hw;
    const float* dn = up32g(c, noise_tchw, px * 4);
    f16* lat = up16(c, lat_inout, (px + guard) * 4);
    launch_init_latents2(dn, lat, sigma0, T, hw, c.stream);
    UG_CHECK(hipGetLastError());
    down16(c, lat, lat_inout, (px + guard) * 4);
  });
}
int ug_op_unet_input(ug_ctx* x, const float* lat, const float* cond, long pixels, float den, int guided, long guard, float* x_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(pixels >= 1 && guard >= 0 && lat && cond && x_inout, "unet input shape");
    const long rows = (guided ? 2 : 1) * pixels + guard;
    const f16* dl = up16(c, lat, pixels * 4); const f16* dc = up16(c, cond, pixels * 4);
    f16* xin = up16(c, x_inout, rows * 8);
    if (guided) launch_make_unet_input_cfg(dl, dc, xin, pixels, den, c.stream);
    else launch_make_unet_input(dl, dc, xin, pixels, den, c.stream);
    UG_CHECK(hipGetLastError());
    down16(c, xin, x_inout, rows * 8);
  });
}
int ug_op_euler_step_cfg(ug_ctx* x, const float* vc, const float* vu, float g, long n, float sigma, float sigma_next, long guard, float* lat_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(n >= 1 && guard >= 0 && vc && vu && lat_inout, "guided euler step shape");
    const f16* dc = up16(c, vc, n); const f16* du = up16(c, vu, n);
    f16* dl = up16(c, lat_inout, n + guard);
    launch_euler_step_cfg(dc, du, g, dl, n, sigma, sigma_next, c.stream);
    UG_CHECK(hipGetLastError());
    down16(c, dl, lat_inout, n + guard);
  });
}
int ug_op_window_blend(ug_ctx* x, const float* prev, const float* cur, long frame_elems, int overlap, float coef, long guard,
                       float* renoised_inout, float* faded_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(frame_elems >= 1 && overlap >= 1 && guard >= 0 && prev && cur && renoised_inout && faded_inout, "window blend shape");
    const long n = frame_elems * overlap;
    const f16* dp = up16(c, prev, n); const f16* dc = up16(c, cur, n);
    f16* rn = up16(c, renoised_inout, n + guard); f16* fd = up16(c, faded_inout, n + guard);
    launch_axpby_f16(dp, 1.f, rn, coef, rn, n, c.stream);
    launch_crossfade_f16(dc, fd, frame_elems, overlap, c.stream);
    UG_CHECK(hipGetLastError());
    down16(c, rn, renoised_inout, n + guard); down16(c, fd, faded_inout, n + guard);
  });
}
int ug_op_time_conv_out(ug_ctx* x, const float* xin, const float* w, const float* b, int T, long HW, int Cs, long guard, float* out_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(T >= 1 && HW >= 1 && Cs >= 3 && guard >= 0 && xin && w && b && out_inout, "time conv out shape");
    const long px = (long)T * HW;
    const f16* dx = up16(c, xin, px * Cs); const f16* dw = up16(c, w, 27); const f16* db = up16(c, b, 3);
    float* out = up32g(c, out_inout, (px + guard) * 3);
    launch_time_conv_out(dx, dw, db, out, T, HW, Cs, c.stream);
    down32g(c, out, out_inout, (px + guard) * 3);
  });
}
int ug_op_depth_post(ug_ctx* x, const float* frames, long n, long guard, float* depth_inout, float* disp_inout, float* minmax_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(n >= 1 && guard >= 0 && frames && depth_inout && disp_inout && minmax_out, "depth post shape");
    const float* df = up32g(c, frames, n * 3);
    float* dd = up32g(c, depth_inout, n + guard); float* dx = up32g(c, disp_inout, n + guard);
    float* mm = c.ws.get<float>(2);
    launch_depth_post(df, dd, mm, n, c.stream);
    launch_disparity_from_frames(df, mm, dx, n, c.stream);
    down32g(c, dd, depth_inout, n + guard); down32g(c, dx, disp_inout, n + guard);
    unsigned u[2];
    UG_CHECK(hipMemcpy(u, mm, 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < 2; ++i) {      // the ordered-integer words back to float (ord2f of kernels/misc.hip)
      const unsigned bits = (u[i] & 0x80000000u) ? (u[i] & 0x7fffffffu) : ~u[i];
      memcpy(&minmax_out[i], &bits, 4);
    }
  });
}
int ug_op_add_grid_nearest(ug_ctx* x, const float* grid, int B, int h, int w, int g, int C, long guard, float* x_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(B >= 1 && h >= 1 && w >= 1 && g >= 1 && C >= 8 && C % 8 == 0 && guard >= 0 && grid && x_inout, "add grid shape");
    const long px = (long)B * h * w;
    const f16* dg = up16(c, grid, (long)B * g * g * C);
    f16* dx = up16(c, x_inout, (px + guard) * C);
    launch_add_grid_nearest(dx, dg, B, h, w, g, C, c.stream);
    UG_CHECK(hipGetLastError());
    down16(c, dx, x_inout, (px + guard) * C);
  });
}
int ug_op_sn_normals_out(ug_ctx* x, const float* dec, int ldd, long pixels, long guard, float* out_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(pixels >= 1 && ldd >= 3 && guard >= 0 && dec && out_inout, "normals out shape");
    const f16* dd = up16(c, dec, pixels * ldd);
    float* out = up32g(c, out_inout, (pixels + guard) * 3);
    launch_sn_normals_out(dd, ldd, out, pixels, c.stream);
    down32g(c, out, out_inout, (pixels + guard) * 3);
  });
}
int ug_op_clip_assemble(ug_ctx* x, const float* patches, const float* cls, const float* pos, int T, int np, int d, long guard, float* tok_inout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(T >= 1 && np >= 1 && d >= 1 && guard >= 0 && patches && cls && pos && tok_inout, "clip assemble shape");
    const long rows = (long)T * (np + 1);
    const f16* dp = up16(c, patches, (long)T * np * d); const f16* dc = up16(c, cls, d); const f16* dq = up16(c, pos, (long)(np + 1) * d);
    f16* tok = up16(c, tok_inout, (rows + guard) * d);
    launch_clip_assemble(dp, dc, dq, tok, T, np, d, c.stream);
    UG_CHECK(hipGetLastError());
    down16(c, tok, tok_inout, (rows + guard) * d);
  });
}

// ------------------------------------------------------------------ micro-benchmarks on device-resident pseudo-random data
int ug_bench_flash(ug_ctx* x, int B, int H, int S, int variant, int iters, float* us_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const long M = (long)B * S; const int C = H * 64;
    f16* qkv = c.ws.get<f16>(M * 3 * C); f16* o = c.ws.get<f16>(M * C);
    launch_fill_random(qkv, M * 3 * C, 7, c.stream);
    FlashP p; p.Q = qkv; p.K = qkv + C; p.V = qkv + 2 * C; p.ldq = p.ldk = p.ldv = 3 * C; p.O = o; p.ldo = C; p.B = B; p.H = H; p.S = S; p.scale = 0.125f;
    p.variant = variant;     // passed with the launch: the process default (and every other launch) is untouched
    *us_out = time_launches_ms(c, 2, iters, [&](int) { launch_flash_attn64(p, c.stream); }) * 1000.f / iters;
  });
}
int ug_bench_ff(ug_ctx* x, int M, int C, int fused, int iters, float* us_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int I = 4 * C;
    f16* dX = c.ws.get<f16>((long)M * C); f16* dW1 = c.ws.get<f16>((long)2 * I * C); f16* db1 = c.ws.get<f16>(2 * I);
    f16* dW2 = c.ws.get<f16>((long)C * I); f16* db2 = c.ws.get<f16>(C); f16* dR = c.ws.get<f16>((long)M * C);
    f16* dO = c.ws.get<f16>((long)M * C); f16* mid = c.ws.get<f16>((long)M * I);
    launch_fill_random(dX, (long)M * C, 1, c.stream); launch_fill_random(dW1, (long)2 * I * C, 2, c.stream); launch_fill_random(db1, 2 * I, 3, c.stream);
    launch_fill_random(dW2, (long)C * I, 4, c.stream); launch_fill_random(db2, C, 5, c.stream); launch_fill_random(dR, (long)M * C, 6, c.stream);
    launch_scale_f16(dW1, dW1, 0.05f, (long)2 * I * C, c.stream); launch_scale_f16(dW2, dW2, 0.03f, (long)C * I, c.stream);
    *us_out = time_launches_ms(c, 2, iters, [&](int) {
      if (fused) launch_ff_fused(ff_fused(c, dX, M, C, dW1, db1, dW2, db2, dR, 1.f, 1.f, dO), c.stream);
      else ff_two_launch(c, dX, M, C, dW1, db1, dW2, db2, dR, 1.f, 1.f, mid, dO);
    }) * 1000.f / iters;
  });
}
int ug_bench_groupnorm(ug_ctx* x, int C0, int C1, int T, int HW, int temporal, int mode, int iters, float* us_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int C = C0 + C1; const long M = (long)T * HW;
    GroupNormP p; memset(&p, 0, sizeof(p));
    f16* a0 = c.ws.get<f16>(M * C0); f16* a1 = C1 ? c.ws.get<f16>(M * C1) : nullptr;
    launch_fill_random(a0, M * C0, 1, c.stream); if (C1) launch_fill_random(a1, M * C1, 2, c.stream);
    f16* gm = c.ws.get<f16>(C); f16* bt = c.ws.get<f16>(C);
    launch_fill_random(gm, C, 3, c.stream); launch_fill_random(bt, C, 4, c.stream);
    p.X0 = a0; p.X1 = a1; p.C0 = C0; p.C1 = C1; p.T = T; p.HW = HW; p.G = 32; p.eps = 1e-5f; p.temporal = temporal; p.silu = 1;
    p.gamma = gm; p.beta = bt; p.Y = c.ws.get<f16>(M * C); p.mode = mode;
    p.ws = c.ws.get<float>((long)groupnorm_ws_floats(T, HW, C, 32));
    us_out[0] = time_launches_ms(c, 3, iters, [&](int) { launch_groupnorm(p, c.stream); }) * 1000.f / iters;
  });
}
int ug_bench_mfma_peak(ug_ctx* x, int iters, float* tflops_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    float* scratch = c.ws.get<float>(256 * 512);
    *tflops_out = bench_mfma_peak(scratch, iters > 0 ? iters : 20000, c.stream);
  });
}

// GEMM / conv microbenchmark: average ms per launch over `iters`.
int ug_bench_gemm(ug_ctx* x, int M, int N, int K, int conv, int T, int Hi, int Wi, int C0, int C1, int kt, int k,
                  int stride, int ups, int cfg, int split, int iters, float* ms_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    GemmP p = conv ? conv_gemm(c, nullptr, C0, nullptr, C1, T, Hi, Wi, kt, k, stride, k / 2, k / 2, ups, nullptr, N, nullptr, nullptr)
                   : dense_gemm(c, nullptr, M, K, nullptr, N, nullptr, nullptr, N);
    M = p.M; K = p.K;                            // conv: the im2col problem, T * Ho * Wo x (C0 + C1) * taps
    const long asz = conv ? (long)T * Hi * Wi * C0 : (long)M * K;
    // rotate through enough distinct A / output buffers to exceed the 256 MiB Infinity Cache: in the pipeline the
    // activation operand was just streamed out by the previous kernel and does not sit in cache
    const long a1sz = C1 ? (long)T * Hi * Wi * C1 : 0;
    const long per = (asz + a1sz + (long)M * N) * 2;
    int nbuf = (int)std::min<long>(16, std::max<long>(2, (600L << 20) / std::max<long>(per, 1) + 1));
    if (getenv("UG_BENCH_WARM")) nbuf = 1;
    std::vector<f16*> As(nbuf), A1s(nbuf), Os(nbuf);
    for (int i = 0; i < nbuf; ++i) {
      As[i] = c.ws.get<f16>(asz); A1s[i] = C1 ? c.ws.get<f16>(a1sz) : nullptr; Os[i] = c.ws.get<f16>((long)M * N);
      launch_fill_random(As[i], asz, 1 + i, c.stream); if (C1) launch_fill_random(A1s[i], a1sz, 100 + i, c.stream);
    }
    f16* Wt = c.ws.get<f16>((long)N * K); f16* b = c.ws.get<f16>(N);
    launch_fill_random(Wt, (long)N * K, 3, c.stream); launch_fill_random(b, N, 4, c.stream);
    p.W = Wt; p.bias = b;
    p.kchunk = (conv && kt * k * k > 1 && (C0 + C1) % 64 == 0 && !getenv("UG_NO_KCHUNK")) ? 1 : 0;   // the engine's chunk-major K order (random weights: the layout itself is immaterial)
    p.A0 = As[0]; p.A1 = A1s[0]; p.Out = Os[0];
    if (getenv("UG_BENCH_GEGLU") && !conv && N % 128 == 0) { p.flags |= UG_F_GEGLU; p.ldo = N / 2; }   // A/B aid: GEGLU epilogue
    if (getenv("UG_BENCH_R1")) { p.R1 = Os[nbuf - 1]; p.ldr1 = N; p.c1 = 1.f; }                          // A/B aid: a residual operand in the epilogue
    if (getenv("UG_BENCH_NOBIAS")) p.bias = nullptr;
    gemm_apply_tune(p, c.tune);
    int cf = cfg, sp = split;                    // forced values win over the planner's
    if (cf < 0 || sp < 1) { int c2, s2; gemm_plan(p, 1, &c2, &s2); if (cf < 0) cf = c2; if (sp < 1) sp = s2; }
    p.cfg_p1 = cf + 1; p.splitk = sp;
    if (sp > 1) p.partial = c.ws.get<float>((long)sp * M * N);
    unsigned* trace = nullptr;
    if (getenv("UG_GEMM_TRACE")) { trace = c.ws.get<unsigned>(3 * 24 * 5); UG_CHECK(hipMemsetAsync(trace, 0, 3 * 24 * 5 * 4, c.stream)); p.trace = trace; }
    const float ms = time_launches_ms(c, 2, iters, [&](int i) { p.A0 = As[i % nbuf]; p.A1 = A1s[i % nbuf]; p.Out = Os[i % nbuf]; launch_gemm(p, 1, c.stream); });
    if (trace) {   // per K-step: [MFMAs issued .. operands landed .. barrier passed .. fetch issued .. MFMAs issued]
      std::vector<unsigned> h(3 * 24 * 5);
      UG_CHECK(hipMemcpy(h.data(), trace, h.size() * 4, hipMemcpyDeviceToHost));
      for (int w = 0; w < 3; ++w) {
        if (w == 2 && h[2 * 24 * 5] == 0) break;   // only the producer / consumer kernel has a third traced wave (a fetch wave)
        printf("wave %d: step  stamp0->1   1->2   2->3   3->next0   total   (gemm_kernel: vmcnt-wait, barrier, fetch-issue, reads+MFMA;"
               " gemm_ws consumer: reads+MFMA, epilogue+lgkm, barrier, -; producer: fetch-issue, vmcnt-wait, barrier, -)\n", w * 4);
        for (int st = 0; st + 1 < 24; ++st) {
          auto at = [&](int s2, int k) { return h[(size_t)w * 24 * 5 + (size_t)s2 * 5 + k]; };
          auto d = [&](unsigned a, unsigned b) { return (b - a) & 0xFFFFF; };
          printf("        %4d  %10u  %7u  %11u  %10u  %6u\n", st + 8, d(at(st, 0), at(st, 1)), d(at(st, 1), at(st, 2)), d(at(st, 2), at(st, 3)),
                 d(at(st, 3), at(st + 1, 0)), d(at(st, 0), at(st + 1, 0)));
        }
      }
    }
    ms_out[0] = ms / iters; ms_out[1] = (float)cf; ms_out[2] = (float)sp; ms_out[3] = (float)M; ms_out[4] = (float)K;
  });
}

}  // extern "C"
