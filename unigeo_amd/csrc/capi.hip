// extern "C" surface of libunigeo_hip.so, product half: exactly the functions declared in include/unigeo_hip.h - the drop-in boundary.
// The test / tuning entry points of include/unigeo_hip_test.h live in capi_test.hip; capi_util.h holds what both units share.
#include "capi_util.h"
#include "pcd_host.h"

static std::string g_create_err;

static UNetCfg to_cfg(const ug_unet_config* g) {
  UNetCfg d; d.in_ch = g->in_channels; d.out_ch = g->out_channels; d.nlev = g->num_levels;
  for (int i = 0; i < 8; ++i) { d.boc[i] = g->block_out_channels[i]; d.heads[i] = g->num_attention_heads[i]; d.has_attn[i] = g->down_has_attn[i]; }
  d.layers = g->layers_per_block; d.cross_dim = g->cross_attention_dim; d.add_dim = g->addition_time_embed_dim;
  d.proj_in_dim = g->projection_class_embeddings_input_dim; d.groups = g->norm_groups;
  d.eps_xattn = g->eps_cross_attn_blocks; d.eps_down = g->eps_plain_down_block; d.eps_mid = g->eps_mid_block; d.eps_up = g->eps_up_blocks;
  return d;
}
static VAECfg to_cfg(const ug_vae_config* g) {
  VAECfg d; d.in_ch = g->in_channels; d.out_ch = g->out_channels; d.lat = g->latent_channels; d.nlev = g->num_levels;
  for (int i = 0; i < 8; ++i) d.boc[i] = g->block_out_channels[i];
  d.layers = g->layers_per_block; d.groups = g->norm_groups; d.scaling = g->scaling_factor;
  return d;
}
static CLIPCfg to_cfg(const ug_clip_config* g) {
  CLIPCfg d; d.hidden = g->hidden_size; d.inter = g->intermediate_size; d.layers = g->num_hidden_layers; d.heads = g->num_attention_heads;
  d.image = g->image_size; d.patch = g->patch_size; d.proj = g->projection_dim; d.eps = g->layer_norm_eps;
  return d;
}

extern "C" {

void ug_unet_config_default(ug_unet_config* o) {
  UNetCfg d; memset(o, 0, sizeof(*o));
  o->in_channels = d.in_ch; o->out_channels = d.out_ch; o->num_levels = d.nlev;
  for (int i = 0; i < 8; ++i) { o->block_out_channels[i] = d.boc[i]; o->num_attention_heads[i] = d.heads[i]; o->down_has_attn[i] = d.has_attn[i]; }
  o->layers_per_block = d.layers; o->cross_attention_dim = d.cross_dim; o->addition_time_embed_dim = d.add_dim;
  o->projection_class_embeddings_input_dim = d.proj_in_dim; o->norm_groups = d.groups;
  o->eps_cross_attn_blocks = d.eps_xattn; o->eps_plain_down_block = d.eps_down; o->eps_mid_block = d.eps_mid; o->eps_up_blocks = d.eps_up;
}
void ug_vae_config_default(ug_vae_config* o) {
  VAECfg d; memset(o, 0, sizeof(*o));
  o->in_channels = d.in_ch; o->out_channels = d.out_ch; o->latent_channels = d.lat; o->num_levels = d.nlev;
  for (int i = 0; i < 8; ++i) o->block_out_channels[i] = d.boc[i];
  o->layers_per_block = d.layers; o->norm_groups = d.groups; o->scaling_factor = d.scaling;
}
void ug_clip_config_default(ug_clip_config* o) {
  CLIPCfg d;
  o->hidden_size = d.hidden; o->intermediate_size = d.inter; o->num_hidden_layers = d.layers; o->num_attention_heads = d.heads;
  o->image_size = d.image; o->patch_size = d.patch; o->projection_dim = d.proj; o->layer_norm_eps = d.eps;
}

ug_ctx* ug_create(int device_id, size_t workspace_bytes, size_t persist_bytes) {
  ug_ctx* x = nullptr;
  try {
    int n = 0;
    UG_CHECK(hipGetDeviceCount(&n));
    UG_REQUIRE(n > 0, "no HIP device visible: the MI355X path has no CPU fallback");
    UG_REQUIRE(device_id >= 0 && device_id < n, "device id out of range");
    UG_CHECK(hipSetDevice(device_id));
    x = new ug_ctx();
    x->c.device = device_id;
    UG_CHECK(hipStreamCreateWithFlags(&x->c.stream, hipStreamNonBlocking));
    x->c.ws.init(workspace_bytes);
    x->c.persist.init(persist_bytes);
    x->c.zero = x->c.persist.get<f16>(128);
    UG_CHECK(hipMemset(x->c.zero, 0, 256));
    return x;
  } catch (const std::exception& e) {
    g_create_err = e.what();
    delete x;
    return nullptr;
  }
}
void ug_destroy(ug_ctx* x) {
  if (!x) return;
  (void)hipSetDevice(x->c.device);
  (void)hipStreamSynchronize(x->c.stream);
  for (auto& kv : x->c.raw) (void)hipFree(kv.second.dev);
  for (int i = 0; i < 2; ++i) if (x->c.pin[i]) (void)hipHostFree(x->c.pin[i]);
  if (x->c.d_pcd_pts) (void)hipFree(x->c.d_pcd_pts);
  x->c.ws.destroy(); x->c.persist.destroy();
  for (auto& l : x->c.lanes) { (void)hipStreamSynchronize(l.stream); (void)hipEventDestroy(l.done); (void)hipStreamDestroy(l.stream); }
  if (x->c.fork_ev) (void)hipEventDestroy(x->c.fork_ev);
  (void)hipStreamDestroy(x->c.stream);
  delete x;
}
const char* ug_last_error(ug_ctx* x) { return x ? x->c.err.c_str() : g_create_err.c_str(); }
size_t ug_workspace_peak(ug_ctx* x) { return x ? x->c.ws.peak() : 0; }

int ug_load_tensor(ug_ctx* x, const char* name, int dtype, int ndim, const int64_t* shape, const void* host) {
  UG_TRY(x, {
    std::vector<long> sh(shape, shape + ndim);
    upload_raw(x->c, name, dtype, sh, host);
  });
}
int ug_bind_unet(ug_ctx* x, const ug_unet_config* g) {
  UG_TRY(x, {
    const UNetCfg d = to_cfg(g);
    UG_REQUIRE(d.nlev >= 2 && d.nlev <= 8, "num_levels");
    UG_REQUIRE(d.in_ch % 8 == 0, "UNet in_channels must be a multiple of 8");
    bind_unet(x->c, d, "unet.");
    finish_binding(x->c, "unet.");
  });
}
int ug_bind_vae(ug_ctx* x, const ug_vae_config* g) {
  UG_TRY(x, {
    bind_vae(x->c, to_cfg(g), "vae.");
    finish_binding(x->c, "vae.");
  });
}
int ug_bind_clip(ug_ctx* x, const ug_clip_config* g) {
  UG_TRY(x, {
    bind_clip(x->c, to_cfg(g), "clip.");
    finish_binding(x->c, "clip.");
  });
}

int ug_dc_set_inputs(ug_ctx* x, const float* frames, int T, int H, int W, const float* nl, const float* na, const float* K) {
  UG_TRY(x, dc_set_inputs(x->c, frames, T, H, W, nl, na, K));
}
int ug_dc_set_inputs_ex(ug_ctx* x, const void* frames, int frames_format, int T, int H, int W, const float* nl, const float* na,
                        uint64_t noise_seed, const float* K) {
  UG_TRY(x, {
    UG_REQUIRE(frames_format == UG_FRAMES_F32_THWC || frames_format == UG_FRAMES_U8_TCHW, "frames_format must be UG_FRAMES_F32_THWC or UG_FRAMES_U8_TCHW");
    dc_set_inputs_ex(x->c, frames, frames_format == UG_FRAMES_U8_TCHW, T, H, W, nl, na, noise_seed, K);
  });
}
int ug_dc_get_noise(ug_ctx* x, float* nl, float* na) { UG_TRY(x, dc_get_noise(x->c, nl, na)); }
int ug_dc_run(ug_ctx* x, int steps, int chunk, int with_normals) { UG_TRY(x, dc_run(x->c, steps, chunk, with_normals)); }
int ug_dc_run_windows(ug_ctx* x, int steps, int chunk, int with_normals, int window, int overlap) {
  UG_TRY(x, dc_run(x->c, steps, chunk, with_normals, window, overlap));
}
int ug_set_coscheduled(ug_ctx* x, int on) {
  if (!x) return -1;
  x->c.cosched = on ? 1 : 0;
  if (on) x->c.tune.knobs |= 4194304; else x->c.tune.knobs &= ~4194304;      // gemm_plan: no last-round fill factor
  x->c.lane_need.clear();
  return 0;
}
int ug_set_fp8_linears(ug_ctx* x, int on) {
  if (!x) return -1;
  x->c.fp8_linears = on ? 1 : 0; x->c.lane_need.clear();
  return 0;
}
int ug_set_concurrency(ug_ctx* x, int lanes) {
  if (!x) return -1;
  x->c.concurrency = std::max(1, std::min(lanes, 8));
  return 0;
}
int ug_set_vae_encode_fp32(ug_ctx* x, int on) {
  if (!x) return -1;
  x->c.vae_encode_fp32 = on ? 1 : 0; x->c.lane_need.clear();
  return 0;
}
int ug_dc_set_guidance(ug_ctx* x, float guidance_scale) {
  UG_TRY(x, {
    UG_REQUIRE(std::isfinite(guidance_scale), "guidance_scale must be finite");
    x->c.guidance = guidance_scale;
  });
}
int ug_dc_get_outputs(ug_ctx* x, float* f, float* d, float* n) { UG_TRY(x, dc_get_outputs(x->c, f, d, n)); }

int ug_dc_device_ptrs(ug_ctx* x, void** f, void** d, void** n) {
  UG_TRY(x, {
    UG_REQUIRE(x->c.io_ready, "no resident outputs");
    if (f) *f = x->c.d_out_frames;
    if (d) *d = x->c.d_depth;
    if (n) *n = x->c.d_normals;
  });
}

int ug_profile_begin(ug_ctx* x) { UG_TRY(x, prof_begin(x->c, false)); }
const char* ug_profile_end(ug_ctx* x) {
  if (!x) return "{}";
  try { x->c.prof_json = prof_end(x->c); } catch (const std::exception& e) { x->c.err = e.what(); x->c.prof_json = "{}"; }
  return x->c.prof_json.c_str();
}

// ---------------------------------------------------------------- StableNormal (reference model/stablenormal.py:16,39)
int ug_bind_stablenormal(ug_ctx* x, const ug_unet_config* gu, const ug_vae_config* gv, const ug_clip_config* gd) {
  UG_TRY(x, {
    UG_REQUIRE(gu && gv && gd, "null config");
    UG_REQUIRE(gu->num_levels >= 2 && gu->num_levels <= 8 && gv->num_levels >= 2 && gv->num_levels <= 8, "num_levels out of range");
    CLIPCfg d = to_cfg(gd);
    d.proj = 0;                      // the DINOv2 tower has no projection head: projection_dim is ignored
    bind_sn(x->c, to_cfg(gu), to_cfg(gv), d, "sn.");      // bind_sn reads none of the SVD-only UNet fields (add_dim, proj_in_dim, eps_*)
    finish_binding(x->c, "sn.");
  });
}
int ug_sn_run(ug_ctx* x, const float* images, int B, int H, int W, const float* prompt, float yoso_t, int nsteps, const float* timesteps,
              const float* ca, const float* cb, float* normals_out) {
  UG_TRY(x, sn_run(x->c, images, B, H, W, prompt, yoso_t, nsteps, timesteps, ca, cb, normals_out));
}

int ug_normals_from_depth(ug_ctx* x, const float* depth, const float* K, int T, int H, int W, float* normals) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const long px = (long)T * H * W;
    float* dd = c.ws.get<float>(px); float* dk = c.ws.get<float>((long)T * 9); float* dn = c.ws.get<float>(px * 3);
    UG_CHECK(hipMemcpy(dd, depth, px * 4, hipMemcpyHostToDevice));
    UG_CHECK(hipMemcpy(dk, K, (size_t)T * 9 * 4, hipMemcpyHostToDevice));
    launch_normals(dd, dk, dn, T, H, W, c.stream);
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(normals, dn, px * 3 * 4, hipMemcpyDeviceToHost));
  });
}

int ug_resize_bilinear(ug_ctx* x, const float* in, int B, int Hi, int Wi, int C, int Ho, int Wo, int normalise, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(B >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1 && C >= 1 && C <= 4, "resize shape");
    const long ni = (long)B * Hi * Wi * C, no = (long)B * Ho * Wo * C;
    float* di = c.ws.get<float>(ni); float* dout = c.ws.get<float>(no);
    UG_CHECK(hipMemcpyAsync(di, in, ni * 4, hipMemcpyHostToDevice, c.stream));
    launch_resize_bilinear_aa(di, dout, B, Hi, Wi, Ho, Wo, C, normalise, c.stream);
    UG_CHECK(hipMemcpyAsync(out, dout, no * 4, hipMemcpyDeviceToHost, c.stream));
    UG_CHECK(hipStreamSynchronize(c.stream));
  });
}

}  // extern "C"

// ---------------------------------------------------------------- evaluation metrics
// the metrics kernels leave nb block partials of K doubles each on the device: wait for the stream, copy them down, sum them in block order
template <int K> static void fetch_partial_sums(Ctx& c, const double* dev, int nb, double (&out)[K]) {
  UG_CHECK(hipStreamSynchronize(c.stream));
  std::vector<double> h((size_t)nb * K);
  if (nb > 0) UG_CHECK(hipMemcpy(h.data(), dev, h.size() * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < K; ++k) out[k] = 0;
  for (int b = 0; b < nb; ++b) for (int k = 0; k < K; ++k) out[k] += h[(size_t)b * K + k];
}
// least squares of g ~ s*p + t from the normal-equation sums n, sum p, sum p^2, sum g, sum p*g:  [sum p^2, sum p; sum p, n] [s; t] = [sum pg; sum g]
static void lstsq_solve(const double* a, double& s_, double& t_) {
  const double det = a[2] * a[0] - a[1] * a[1];
  // Degenerate clips do not abort the evaluation run (the reference's np.linalg.lstsq returns the minimum-norm solution
  // and its loop continues, metrics/alignment.py:150-167): no valid pixel -> s = t = 0 and zero metrics below; rank-1
  // system (one pixel / constant prediction p = c) -> [s, t] = mean(g) / (c^2 + 1) * [c, 1].
  s_ = 0.0; t_ = 0.0;
  if (a[0] >= 1) {
    if (fabs(det) > 1e-12 * fmax(1.0, a[2] * a[0])) { s_ = (a[4] * a[0] - a[1] * a[3]) / det; t_ = (a[2] * a[3] - a[1] * a[4]) / det; }
    else { const double cm = a[1] / a[0], gm = a[3] / a[0]; s_ = cm * gm / (cm * cm + 1.0); t_ = gm / (cm * cm + 1.0); }
  }
}
// host half of the least-squares alignment (waits for the stream), after a fit launch left its nb partial sums in `part`
static void fetch_lstsq(Ctx& c, const double* part, int nb, double& s_, double& t_) {
  double a[5];
  fetch_partial_sums(c, part, nb, a);
  lstsq_solve(a, s_, t_);
}
// the least-squares alignment of the pre-clipped prediction against fit_g on its mask1: launch, fetch, solve (part: EVAL_MAXB * 5 doubles)
static void fit_lstsq(Ctx& c, const DepthEvalBufs& d, const float* fit_g, const DepthBounds& b, double* part, double& s_, double& t_) {
  int nb = 0;
  launch_depth_fit(d.dp, fit_g, d.n, b.md, b.lo, b.hi, part, &nb, c.stream);
  fetch_lstsq(c, part, nb, s_, t_);
}
// host half of the metrics pass, after launch_depth_metrics / launch_radius_metrics (waits for the stream): out[11] as include/unigeo_hip.h documents it
static void fetch_depth_metrics(Ctx& c, const double* part, int nb, double s_, double t_, double* out) {
  double m[9];
  fetch_partial_sums(c, part, nb, m);
  const double cnt = m[0];
  if (cnt > 0) {
    out[0] = m[1] / cnt; out[1] = m[2] / cnt; out[2] = sqrt(m[3] / cnt); out[3] = sqrt(m[4] / cnt);
    for (int k = 0; k < 4; ++k) out[4 + k] = m[5 + k] / cnt;
  } else { for (int k = 0; k < 8; ++k) out[k] = 0; }
  out[8] = cnt; out[9] = s_; out[10] = t_;
}

// the camera table of k_world_radius / k_world_points on the device: per frame fx, fy, cx, cy, R row-major, t, widened from float32
static const double* upload_cam_table(Ctx& c, const float* cam2world, const float* K, int T) {
  std::vector<double> tab((size_t)T * 16);
  for (int f = 0; f < T; ++f) {
    const float* k = K + (size_t)f * 9; const float* p = cam2world + (size_t)f * 16; double* q = tab.data() + (size_t)f * 16;
    q[0] = k[0]; q[1] = k[4]; q[2] = k[2]; q[3] = k[5];
    for (int r = 0; r < 3; ++r) { for (int j = 0; j < 3; ++j) q[4 + r * 3 + j] = p[r * 4 + j]; q[13 + r] = p[r * 4 + 3]; }
  }
  double* dcam = c.ws.get<double>((long)T * 16); UG_CHECK(hipMemcpy(dcam, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  return dcam;
}
// what ug_eval_depth_global and ug_pcd_world_points share once their own pointers are checked: the shape checks (fewer than pixel_cap pixels), the
// uploads (gt_radius may be NULL), the camera table and the first fit (s, t) of the depth; part holds EVAL_MAXB * 9 doubles for the launches that follow
struct WorldFit { long n; DepthBounds b; DepthEvalBufs d; float* dgr; const double* dcam; double* part; double s, t; };
static WorldFit world_first_fit(Ctx& c, const float* pred, const float* gt, const float* gt_radius, const unsigned char* cmask, const float* cam2world,
                                const float* K, int T, int H, int W, const ug_depth_eval_opts* o, long pixel_cap) {
  UG_REQUIRE(T > 0 && H > 0 && W > 0, "T, H and W must be positive");
  WorldFit f{};
  f.n = (long)T * H * W;
  UG_REQUIRE(f.n < pixel_cap, "pixel count");
  UG_REQUIRE(pred || (c.io_ready && T == c.T && H == c.H && W == c.W), "no resident depth of that shape");
  f.b = depth_bounds(o);
  f.d = depth_eval_upload(c, pred, gt, cmask, f.n);
  if (gt_radius) { f.dgr = c.ws.get<float>(f.n); UG_CHECK(hipMemcpy(f.dgr, gt_radius, f.n * 4, hipMemcpyHostToDevice)); }
  f.dcam = upload_cam_table(c, cam2world, K, T);
  f.part = c.ws.get<double>(EVAL_MAXB * 9);
  fit_lstsq(c, f.d, f.d.dg, f.b, f.part, f.s, f.t);
  return f;
}

// ---------------------------------------------------------------- point-cloud evaluation (kernels/pcd.hip)
// mean and np.median of n doubles on the device: a fixed-order sum, and the one or two middle order statistics by exact selection
static void pcd_mean_median(Ctx& c, const double* v, long n, unsigned* sel, unsigned long long* res, double* part, double& mean, double& med) {
  int nb = 0;
  launch_pcd_sum(v, n, part, &nb, c.stream);
  launch_pcd_select(v, 1, n, 1, 0, (unsigned long long)((n - 1) / 2), sel, res, 0, c.stream);
  launch_pcd_select(v, 1, n, 1, 0, (unsigned long long)(n / 2), sel, res, 1, c.stream);
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  double s[1];
  fetch_partial_sums(c, part, nb, s);
  unsigned long long k[2];
  UG_CHECK(hipMemcpy(k, res, sizeof(k), hipMemcpyDeviceToHost));
  mean = s[0] / (double)n;
  med = (pcd_unkey_f64(k[0]) + pcd_unkey_f64(k[1])) / 2.0;
}

// ug_eval_pcd, ug_eval_pcd_fps and ug_eval_pcd_ex: one pipeline.  `fps` replaces the index list by farthest-point sampling of each aligned cloud
// (DESIGN.md section 19); `grid` sends every search through a uniform grid over its target cloud and issues no other
// launch differently.
static void eval_pcd_run(Ctx& c, const float* pred_pts, const float* gt_pts, const unsigned char* mask, long n, const long* sample_idx, long n_sample,
                         bool fps, bool grid, const ug_pcd_opts* o, double* out, float* pred_cloud_out, float* gt_cloud_out, long* pred_idx_out,
                         long* gt_idx_out, long* search_stats, const ug_pcd_score_opts* so = nullptr, long* score_counts = nullptr,
                         long* voxel_counts = nullptr) {
  if (search_stats) for (int k = 0; k < 8; ++k) search_stats[k] = 0;
  UG_REQUIRE(o && gt_pts && mask && out, "options, gt_pts, mask and out32 must not be NULL");
  UG_REQUIRE(n > 0 && n < (1L << 31), "n_pixels must be positive and below 2^31");
  UG_REQUIRE(o->knn >= 1 && o->knn <= UG_PCD_MAX_KNN, "knn must be 1..UG_PCD_MAX_KNN");
  UG_REQUIRE(o->threshold > 0.f && o->max_iteration >= 0, "threshold must be positive and max_iteration not negative");
  UG_REQUIRE(pred_pts || (c.d_pcd_pts && c.pcd_pixels == n), "no resident world points of that size (ug_pcd_world_points first)");
  UG_REQUIRE(!sample_idx || n_sample > 0, "n_sample must be positive when sample_idx is given");
  const float* dp = c.d_pcd_pts;
  if (pred_pts) { float* d = c.ws.get<float>(n * 3); UG_CHECK(hipMemcpy(d, pred_pts, (size_t)n * 12, hipMemcpyHostToDevice)); dp = d; }
  float* dg = c.ws.get<float>(n * 3); UG_CHECK(hipMemcpy(dg, gt_pts, (size_t)n * 12, hipMemcpyHostToDevice));
  unsigned char* dm = (unsigned char*)c.ws.alloc(n); UG_CHECK(hipMemcpy(dm, mask, n, hipMemcpyHostToDevice));
  unsigned* counts = (unsigned*)c.ws.alloc((PCD_MAXB + 1) * 4);
  float* P = c.ws.get<float>(n * 3); float* G = c.ws.get<float>(n * 3);
  launch_pcd_compact(dp, dg, dm, n, counts, P, G, c.stream);
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  unsigned m32 = 0;
  UG_CHECK(hipMemcpy(&m32, counts + PCD_MAXB, 4, hipMemcpyDeviceToHost));
  const long m = m32;
  for (int k = 0; k < 32; ++k) out[k] = NAN;
  out[8] = 0; out[9] = 0; out[10] = 0; out[11] = 0;
  double Tm[16];
  for (int i = 0; i < 16; ++i) Tm[i] = (i % 5 == 0) ? 1.0 : 0.0;
  memcpy(out + 12, Tm, sizeof(Tm));
  if (m == 0) return;      // empty mask: NaN metrics, like the mean over an empty selection
  const bool sample = fps && n_sample > 0 && n_sample < m;      // otherwise farthest-point sampling takes every point: no sampling at all
  const long ns = (sample_idx || sample) ? n_sample : m;
  if (sample_idx) for (long j = 0; j < ns; ++j) UG_REQUIRE(sample_idx[j] >= 0 && sample_idx[j] < m, "a sample index lies outside the masked points");
  UG_REQUIRE(grid || (double)ns * (double)ns <= 1099511627776.0,      // with the grid the cap counts the leftover queries of every pass
             "more than 2^40 point pairs in one nearest-neighbour pass: lower pcd_downsample_num");

  // alignment: median shifts along z, then per cloud the median centre and the median distance from it (all exact selections)
  unsigned* sel = (unsigned*)c.ws.alloc(PCD_SEL_WORDS * 4);
  unsigned long long* res = c.ws.get<unsigned long long>(16);
  const unsigned long long kmed = (unsigned long long)((m - 1) / 2);
  launch_pcd_select(P, 0, m, 3, 2, kmed, sel, res, 0, c.stream);
  launch_pcd_select(G, 0, m, 3, 2, kmed, sel, res, 1, c.stream);
  launch_pcd_shift_z(P, G, m, res, 0, 1, c.stream);
  float* norm = c.ws.get<float>(m);
  for (int a = 0; a < 2; ++a) {
    const float* X = a ? G : P;
    for (int k = 0; k < 3; ++k) launch_pcd_select(X, 0, m, 3, k, kmed, sel, res, 2 + a * 3 + k, c.stream);
    launch_pcd_center_norm(X, m, res, 2 + a * 3, norm, c.stream);
    launch_pcd_select(norm, 0, m, 1, 0, kmed, sel, res, 8 + a, c.stream);
  }
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  unsigned long long hres[10];
  UG_CHECK(hipMemcpy(hres, res, sizeof(hres), hipMemcpyDeviceToHost));
  const float pz = pcd_unkey_f32(hres[0]), gz = pcd_unkey_f32(hres[1]), gs = pcd_unkey_f32(hres[9]);
  const float ps = std::min(std::max(pcd_unkey_f32(hres[8]), 1e-3f), 1e3f);
  const float ratio = gs / ps;
  out[28] = ps; out[29] = gs; out[30] = pz; out[31] = gz; out[8] = (double)ns;

  long* didx = nullptr;
  if (sample_idx) { didx = c.ws.get<long>(ns); UG_CHECK(hipMemcpy(didx, sample_idx, (size_t)ns * sizeof(long), hipMemcpyHostToDevice)); }
  float* p32 = c.ws.get<float>(ns * 3); float* g32 = c.ws.get<float>(ns * 3);
  double* p64 = c.ws.get<double>(ns * 3); double* g64 = c.ws.get<double>(ns * 3);
  long* fidx[2] = {nullptr, nullptr};
  if (sample) {      // align every masked point in place (each thread reads its own point before it writes it), then pick from each cloud on its own
    launch_pcd_align(P, G, nullptr, m, ratio, gz, P, G, nullptr, nullptr, c.stream);
    float* fm = c.ws.get<float>(m); float* fpm = c.ws.get<float>(2 * PCD_MAXB); int* fpi = c.ws.get<int>(2 * PCD_MAXB);
    float* fsel = c.ws.get<float>(ns);
    for (int a = 0; a < 2; ++a) {
      fidx[a] = c.ws.get<long>(ns);
      launch_pcd_fps(a ? G : P, m, ns, fm, fpm, fpi, fidx[a], fsel, c.stream);
      launch_pcd_gather(a ? G : P, fidx[a], ns, a ? g32 : p32, a ? g64 : p64, c.stream);
    }
  } else launch_pcd_align(P, G, didx, ns, ratio, gz, p32, g32, p64, g64, c.stream);
  UG_CHECK(hipGetLastError());
  UG_CHECK(hipStreamSynchronize(c.stream));
  long* const idx_out[2] = {pred_idx_out, gt_idx_out};
  for (int a = 0; a < 2; ++a) {
    if (!idx_out[a]) continue;
    if (sample) UG_CHECK(hipMemcpy(idx_out[a], fidx[a], (size_t)ns * sizeof(long), hipMemcpyDeviceToHost));
    else for (long j = 0; j < ns; ++j) idx_out[a][j] = sample_idx ? sample_idx[j] : j;
  }
  if (pred_cloud_out) UG_CHECK(hipMemcpy(pred_cloud_out, p32, (size_t)ns * 12, hipMemcpyDeviceToHost));
  if (gt_cloud_out) UG_CHECK(hipMemcpy(gt_cloud_out, g32, (size_t)ns * 12, hipMemcpyDeviceToHost));

  // point-to-point ICP from the identity: the pair search and the Kabsch sums on the device, the 3x3 SVD here
  const int ny = pcd_nn_slices(ns, ns);
  int* idx = c.ws.get<int>(ns); double* dist = c.ws.get<double>(ns);
  int* pidx = nullptr; double* pdist = nullptr;
  if (!grid) { pidx = c.ws.get<int>((long)ny * ns); pdist = c.ws.get<double>((long)ny * ns); }
  PcdGrid gridG{}, gridP{};      // over g64, built once for the ICP, the accuracy pass and its own KNN; over the moved prediction, built after the ICP
  PcdSearchStats st;
  long cellmax[2] = {0, 0};
  int* left = nullptr; unsigned* n_left = nullptr;
  if (grid) {
    left = c.ws.get<int>(ns); n_left = c.ws.get<unsigned>(1);
    gridG = pcd_grid_build(c, g64, ns, &cellmax[0]);
  }
  double* dT = c.ws.get<double>(16);
  double* part = c.ws.get<double>(PCD_MAXB * 17);
  double sums[17];
  const double thr = (double)o->threshold;
  auto evaluate = [&](double& fit, double& rmse) {      // the stream is idle whenever dT is rewritten: every evaluation ends with a fetch
    UG_CHECK(hipMemcpy(dT, Tm, sizeof(Tm), hipMemcpyHostToDevice));
    int nb = 0;
    if (grid) pcd_nn_search_grid(c, p64, ns, dT, gridG, idx, dist, left, n_left, st);
    else launch_pcd_nn(p64, ns, g64, ns, dT, idx, dist, pidx, pdist, c.stream);
    launch_pcd_kabsch(p64, g64, ns, dT, idx, dist, thr, part, &nb, c.stream);
    UG_CHECK(hipGetLastError());
    fetch_partial_sums(c, part, nb, sums);
    fit = sums[0] / (double)ns;
    rmse = sums[0] > 0 ? sqrt(sums[16] / sums[0]) : 0.0;
  };
  double fit = 0, rmse = 0;
  evaluate(fit, rmse);
  int it = 0;
  while (it < o->max_iteration) {
    double U[16], Tn[16];
    pcd_host::umeyama_from_sums(sums, U);
    pcd_host::mul44(U, Tm, Tn);
    memcpy(Tm, Tn, sizeof(Tm));
    const double pf = fit, pr = rmse;
    evaluate(fit, rmse);
    ++it;
    if (fabs(pf - fit) < 1e-6 && fabs(pr - rmse) < 1e-6) break;
  }
  out[9] = it; out[10] = fit; out[11] = rmse;
  memcpy(out + 12, Tm, sizeof(Tm));

  // the moved prediction, normals of both clouds, nearest neighbours both ways, scores
  double* moved = c.ws.get<double>(ns * 3);
  double* nP = c.ws.get<double>(ns * 3); double* nG = c.ws.get<double>(ns * 3);
  int* idx2 = c.ws.get<int>(ns); double* dist2 = c.ws.get<double>(ns);
  double* dot1 = c.ws.get<double>(ns); double* dot2 = c.ws.get<double>(ns);
  launch_pcd_move(p64, ns, dT, moved, c.stream);      // dT holds the final transformation: the last evaluation uploaded it
  if (grid) {
    gridP = pcd_grid_build(c, moved, ns, &cellmax[1]);
    pcd_knn_search_grid(c, gridP, o->knn, nullptr, nP, left, n_left, st);
    pcd_knn_search_grid(c, gridG, o->knn, nullptr, nG, left, n_left, st);
    pcd_nn_search_grid(c, moved, ns, nullptr, gridG, idx, dist, left, n_left, st);      // accuracy: prediction -> ground truth
    launch_pcd_normal_dot(nP, nG, idx, ns, dot1, c.stream);
    pcd_nn_search_grid(c, g64, ns, nullptr, gridP, idx2, dist2, left, n_left, st);      // completion: ground truth -> prediction
    launch_pcd_normal_dot(nG, nP, idx2, ns, dot2, c.stream);
  } else {
    launch_pcd_knn_normals(moved, ns, o->knn, nullptr, nP, c.stream);
    launch_pcd_knn_normals(g64, ns, o->knn, nullptr, nG, c.stream);
    launch_pcd_nn(moved, ns, g64, ns, nullptr, idx, dist, pidx, pdist, c.stream);       // accuracy: prediction -> ground truth
    launch_pcd_normal_dot(nP, nG, idx, ns, dot1, c.stream);
    launch_pcd_nn(g64, ns, moved, ns, nullptr, idx2, dist2, pidx, pdist, c.stream);     // completion: ground truth -> prediction
    launch_pcd_normal_dot(nG, nP, idx2, ns, dot2, c.stream);
  }
  UG_CHECK(hipGetLastError());
  pcd_mean_median(c, dist, ns, sel, res, part, out[0], out[4]);
  pcd_mean_median(c, dist2, ns, sel, res, part, out[1], out[5]);
  pcd_mean_median(c, dot1, ns, sel, res, part, out[2], out[6]);
  pcd_mean_median(c, dot2, ns, sel, res, part, out[3], out[7]);
  if (grid && search_stats) {
    search_stats[0] = st.settled; search_stats[1] = st.left;
    search_stats[2] = gridG.cells; search_stats[3] = cellmax[0]; search_stats[4] = gridP.cells; search_stats[5] = cellmax[1];
    search_stats[6] = (long)c.ws.peak();
  }

  // counts below the thresholds over the two distance arrays just averaged, and the voxel sets of the two clouds behind them
  if (so && so->n_thresholds > 0) {
    PcdThresholds t;
    t.n = so->n_thresholds;
    for (int k = 0; k < PCD_MAX_THRESHOLDS; ++k) t.tau[k] = k < t.n ? so->thresholds[k] : 0.0;
    unsigned* cpart = c.ws.get<unsigned>((long)PCD_MAXB * PCD_MAX_THRESHOLDS);
    std::vector<unsigned> hp;
    for (int a = 0; a < 2; ++a) {      // 0: accuracy distances -> precision, 1: completion distances -> recall
      int nb = 0;
      launch_pcd_count_below(a ? dist2 : dist, ns, t, cpart, &nb, c.stream);
      UG_CHECK(hipGetLastError());
      UG_CHECK(hipStreamSynchronize(c.stream));
      hp.resize((size_t)nb * PCD_MAX_THRESHOLDS);
      UG_CHECK(hipMemcpy(hp.data(), cpart, hp.size() * 4, hipMemcpyDeviceToHost));
      for (int k = 0; k < t.n; ++k) {
        long cnt = 0;
        for (int b = 0; b < nb; ++b) cnt += hp[(size_t)b * PCD_MAX_THRESHOLDS + k];      // block order
        score_counts[2 * k + a] = cnt;
      }
    }
  }
  if (so)
    for (int k = 0; k < so->n_voxel_sizes; ++k)
      voxel_set_run(c, moved, ns, g64, ns, so->voxel_sizes[k], voxel_capacity(2 * ns), voxel_counts + 6 * k, "ug_eval_pcd_scores");
}

// What eval_pcd_run takes from the workspace for n pixels of which m are masked in and ns are evaluated, allocation by allocation as the arena
// rounds them, the count partials and the voxel table of section 32 included.  Exact for the brute-force search; with the grid the cell tables
// (they depend on the extent of the clouds) and the scratch of the leftover queries are not in the figure.
static size_t pcd_scores_request(long n, long m, long ns, bool host_pred, bool has_idx, bool sample, bool grid, int n_thr, int n_vox) {
  auto r = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t need = (host_pred ? r((size_t)n * 12) : 0) + r((size_t)n * 12) + r((size_t)n) + r((PCD_MAXB + 1) * 4) + 2 * r((size_t)n * 12);
  if (m == 0) return need;
  need += r(PCD_SEL_WORDS * 4) + r(16 * 8) + r((size_t)m * 4);
  if (has_idx) need += r((size_t)ns * 8);
  need += 2 * r((size_t)ns * 12) + 2 * r((size_t)ns * 24);
  if (sample) need += r((size_t)m * 4) + 2 * r(2 * PCD_MAXB * 4) + r((size_t)ns * 4) + 2 * r((size_t)ns * 8);
  need += r((size_t)ns * 4) + r((size_t)ns * 8);
  if (grid) need += r((size_t)ns * 4) + r(4) + 2 * (r((size_t)PCD_MAXB * 7 * 8) + r(64) + r((size_t)ns * 24) + r((size_t)ns * 4));
  else { const size_t ny = (size_t)pcd_nn_slices(ns, ns); need += r(ny * ns * 4) + r(ny * ns * 8); }
  need += r(16 * 8) + r((size_t)PCD_MAXB * 17 * 8);
  need += 3 * r((size_t)ns * 24) + r((size_t)ns * 4) + 3 * r((size_t)ns * 8);
  if (n_thr > 0) need += r((size_t)PCD_MAXB * PCD_MAX_THRESHOLDS * 4);
  if (n_vox > 0) need += voxel_table_bytes(voxel_capacity(2 * ns));
  return need;
}

// ---------------------------------------------------------------- clip preparation helpers (ug_prep_*)
static const size_t PREP_CHUNK_BYTES = (size_t)96 << 20;      // device bytes one chunk of frames may take: the workspace does not grow with T
static int prep_chunk_frames(int T, size_t per_frame) {
  const size_t f = PREP_CHUNK_BYTES / (per_frame ? per_frame : 1);
  return (int)std::min<size_t>((size_t)T, std::max<size_t>(f, 1));
}
// [n_out][K] tap table -> tap-major [K][n_out] on the device, after checking every index against the source length
static void prep_upload_taps(Ctx& c, const int* idx, const double* w, int n_out, int K, int n_in, const int** didx, const double** dw) {
  std::vector<int> ti((size_t)n_out * K); std::vector<double> tw((size_t)n_out * K);
  for (int o = 0; o < n_out; ++o)
    for (int k = 0; k < K; ++k) {
      const int s = idx[(size_t)o * K + k];
      UG_REQUIRE(s >= 0 && s < n_in, "a tap index lies outside the source");
      ti[(size_t)k * n_out + o] = s; tw[(size_t)k * n_out + o] = w[(size_t)o * K + k];
    }
  int* di = c.ws.get<int>((long)n_out * K); double* dwt = c.ws.get<double>((long)n_out * K);
  UG_CHECK(hipMemcpy(di, ti.data(), ti.size() * 4, hipMemcpyHostToDevice));
  UG_CHECK(hipMemcpy(dwt, tw.data(), tw.size() * 8, hipMemcpyHostToDevice));
  *didx = di; *dw = dwt;
}

// ug_eval_depth, ug_eval_depth_ex and ug_eval_depth_ex2 (DESIGN.md sections 13, 23, 24): one path, the callers resolve their options into `b`.
// disparity: the prediction (NULL: the resident disparity of the last run, made here from the resident frames and min-max) is fitted against
// gfit = mask1 ? 1 / (gt + 1e-8f) : 0 by the same fit kernels with the depth bound off, and the metric kernel inverts the aligned disparity;
// floor_ = NaN: no floor.
static void eval_depth_modes(ug_ctx* x, const float* pred, const float* gt, const unsigned char* cmask, long n, int alignment, const DepthBounds& b,
                             bool disparity, float floor_, double* out, float* emap_out) {
  Ctx& c = x->c;
  UG_REQUIRE(alignment >= UG_ALIGN_LSTSQ && alignment <= UG_ALIGN_L1, "unknown depth alignment (UG_ALIGN_LSTSQ / MEDIAN / SCALE / METRIC / L1)");
  UG_REQUIRE(n >= 0 && n < (1L << 32), "pixel count");
  if (disparity && !pred) UG_REQUIRE(c.io_ready && c.out_ready && n == (long)c.T * c.H * c.W, "no resident disparity of that size (run a clip first)");
  DepthEvalBufs d = depth_eval_upload(c, pred, gt, cmask, n);
  const float* fit_g = d.dg;      // the target of the fit and its bounds
  DepthBounds fb = b;
  if (disparity) {
    if (!pred) {
      float* dx = c.ws.get<float>(n);
      launch_disparity_from_frames(c.d_out_frames, c.d_mm, dx, n, c.stream);
      d.dp = dx;
    }
    float* gfit = c.ws.get<float>(n);
    launch_disp_target(d.dg, n, b.md, gfit, c.stream);
    fit_g = gfit; fb.md = NAN;
  }
  double* part = c.ws.get<double>(EVAL_MAXB * 9);
  double s_ = 0.0, t_ = 0.0;
  if (alignment == UG_ALIGN_LSTSQ) fit_lstsq(c, d, fit_g, fb, part, s_, t_);
  else if (alignment == UG_ALIGN_MEDIAN) {
    unsigned* sel = (unsigned*)c.ws.alloc(SEL_WORDS * 4);
    launch_masked_median(d.dp, fit_g, n, fb.md, fb.lo, fb.hi, sel, c.stream);
    unsigned cnt; float mp, mg;
    read_masked_median(c, sel, cnt, mp, mg);
    if (cnt > 0) { const float sf = mg / mp; s_ = sf; }
  } else if (alignment == UG_ALIGN_SCALE) {
    double* wz = c.ws.get<double>(2);
    launch_weiszfeld_scale(d.dp, fit_g, n, fb.md, fb.lo, fb.hi, 10, wz, part, c.stream);
    UG_CHECK(hipStreamSynchronize(c.stream));
    double r[2];
    UG_CHECK(hipMemcpy(r, wz, sizeof(r), hipMemcpyDeviceToHost));
    if (r[1] >= 1) s_ = r[0] < 1e-3 ? 1e-3 : r[0];
  } else if (alignment == UG_ALIGN_L1) {
    double st[2];
    l1_fit_device(c, d.dp, fit_g, n, fb.md, fb.lo, fb.hi, st, x->l1_info);
    s_ = (float)st[0]; t_ = (float)st[1];      // rounded once to float32, as least squares returns them
  } else s_ = 1.0;
  float* dmap = emap_out ? c.ws.get<float>(n) : nullptr;
  int nb = 0;
  launch_depth_metrics(d.dp, d.dg, d.dm, n, b.md, b.lo, b.hi, b.plo, b.phi, floor_, (float)s_, (float)t_, part, dmap, &nb, c.stream,
                       alignment == UG_ALIGN_L1, disparity);
  fetch_depth_metrics(c, part, nb, s_, t_, out);
  if (emap_out) UG_CHECK(hipMemcpy(emap_out, dmap, n * 4, hipMemcpyDeviceToHost));
}

extern "C" {

int ug_eval_depth(ug_ctx* x, const float* pred, const float* gt, const unsigned char* cmask, long n, float max_depth, double* out) {
  UG_TRY(x, {
    Scope sc(x->c);
    ug_depth_eval_opts o;
    ug_depth_eval_opts_default(&o);
    DepthBounds b = depth_bounds(&o);
    b.md = max_depth > 0.f ? max_depth : 0.f;      // this entry point tests gt < max_depth: a NaN or non-positive bound selects no pixel
    eval_depth_modes(x, pred, gt, cmask, n, o.alignment, b, false, NAN, out, nullptr);
  });
}

void ug_depth_eval_opts_default(ug_depth_eval_opts* o) {
  o->alignment = UG_ALIGN_LSTSQ; o->max_depth = 80.f;
  o->pre_clip_min = o->pre_clip_max = o->post_clip_min = o->post_clip_max = NAN;
}

int ug_eval_depth_ex(ug_ctx* x, const float* pred, const float* gt, const unsigned char* cmask, long n, const ug_depth_eval_opts* o,
                     double* out, float* emap_out) {
  UG_TRY(x, {
    Scope sc(x->c);
    UG_REQUIRE(o != nullptr, "options must not be NULL");
    eval_depth_modes(x, pred, gt, cmask, n, o->alignment, depth_bounds(o), false, NAN, out, emap_out);
  });
}

void ug_depth_eval_opts2_default(ug_depth_eval_opts2* o) {
  ug_depth_eval_opts_default(&o->base);
  o->flags = 0u; o->disp_clip_min = NAN;
}

int ug_eval_depth_ex2(ug_ctx* x, const float* pred, const float* gt, const unsigned char* cmask, long n, const ug_depth_eval_opts2* o,
                      double* out, float* emap_out) {
  UG_TRY(x, {
    Scope sc(x->c);
    UG_REQUIRE(o != nullptr, "options must not be NULL");
    UG_REQUIRE((o->flags & ~(unsigned)UG_DEPTH_ALIGN_DISPARITY) == 0u, "unknown flag bit (UG_DEPTH_ALIGN_DISPARITY)");
    const bool disparity = (o->flags & UG_DEPTH_ALIGN_DISPARITY) != 0u;
    const float fl = o->disp_clip_min;
    UG_REQUIRE(std::isnan(fl) || (fl > 0.f && std::isfinite(fl)), "disp_clip_min must be finite and positive (NaN: off)");
    UG_REQUIRE(std::isnan(fl) || disparity, "disp_clip_min needs UG_DEPTH_ALIGN_DISPARITY");
    eval_depth_modes(x, pred, gt, cmask, n, o->base.alignment, depth_bounds(&o->base), disparity, fl, out, emap_out);
  });
}

int ug_dc_get_disparity(ug_ctx* x, float* disp_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(disp_out != nullptr, "disp_out must not be NULL");
    UG_REQUIRE(c.io_ready && c.out_ready, "no resident disparity (run a clip first)");
    const long px = (long)c.T * c.H * c.W;
    float* dx = c.ws.get<float>(px);
    launch_disparity_from_frames(c.d_out_frames, c.d_mm, dx, px, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(disp_out, dx, px * 4, hipMemcpyDeviceToHost));
  });
}

int ug_eval_depth_l1_info(ug_ctx* x, long* out_info) {
  UG_TRY(x, {
    UG_REQUIRE(out_info != nullptr, "out_info must not be NULL");
    for (int i = 0; i < 4; ++i) out_info[i] = x->l1_info[i];
  });
}

int ug_eval_depth_global(ug_ctx* x, const float* pred, const float* gt, const float* gt_radius, const float* cam2world, const float* K,
                         const unsigned char* cmask, int T, int H, int W, const ug_depth_eval_opts* o, double* out, float* rmap_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(o != nullptr, "options must not be NULL");
    UG_REQUIRE(o->alignment == UG_ALIGN_LSTSQ, "depth alignment in global coordinates must be UG_ALIGN_LSTSQ (the reference asserts least squares)");
    UG_REQUIRE(gt && gt_radius && cam2world && K && out, "gt_depth, gt_radius, cam2world, intrinsics and out13 must not be NULL");
    const WorldFit f = world_first_fit(c, pred, gt, gt_radius, cmask, cam2world, K, T, H, W, o, 1L << 32);
    const long n = f.n;
    float* dr = c.ws.get<float>(n);
    int nb = 0;
    double sr = 0.0, tr = 0.0;
    launch_world_radius(f.d.dp, f.d.dg, f.dgr, f.dcam, n, H, W, f.b.md, f.b.plo, f.b.phi, (float)f.s, (float)f.t, dr, f.part, &nb, c.stream);
    fetch_lstsq(c, f.part, nb, sr, tr);
    float* dmap = rmap_out ? c.ws.get<float>(n) : nullptr;
    launch_radius_metrics(dr, f.d.dg, f.dgr, f.d.dm, n, f.b.md, (float)sr, (float)tr, f.part, dmap, &nb, c.stream);
    fetch_depth_metrics(c, f.part, nb, sr, tr, out);
    out[11] = f.s; out[12] = f.t;
    if (rmap_out) UG_CHECK(hipMemcpy(rmap_out, dmap, n * 4, hipMemcpyDeviceToHost));
  });
}

// ---------------------------------------------------------------- temporal alignment error (kernels/temporal.hip)
void ug_tae_opts_default(ug_tae_opts* o) {
  if (!o) return;
  o->s = 1.f; o->t = 0.f; o->flags = 0u;
  o->disp_clip_min = o->post_clip_min = o->post_clip_max = NAN;
  o->max_depth = 80.f; o->stride = 1;
}

int ug_eval_tae(ug_ctx* x, const float* pred, const float* gt, const unsigned char* cmask, const float* K, const double* rel, int T, int H, int W,
                const ug_tae_opts* o, double* out4, double* pair_out, float* warp_out, float* err_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(o != nullptr, "options must not be NULL");
    UG_REQUIRE(gt && K && rel && out4, "gt_depth, intrinsics, rel and out4 must not be NULL");
    UG_REQUIRE(T > 0 && H > 0 && W > 0, "T, H and W must be positive");
    UG_REQUIRE(o->stride >= 1, "stride must be at least 1");
    UG_REQUIRE((o->flags & ~(unsigned)UG_DEPTH_ALIGN_DISPARITY) == 0u, "unknown flag bit (UG_DEPTH_ALIGN_DISPARITY)");
    const bool disparity = (o->flags & UG_DEPTH_ALIGN_DISPARITY) != 0u;
    const float fl = o->disp_clip_min;
    UG_REQUIRE(std::isnan(fl) || (fl > 0.f && std::isfinite(fl)), "disp_clip_min must be finite and positive (NaN: off)");
    UG_REQUIRE(std::isnan(fl) || disparity, "disp_clip_min needs UG_DEPTH_ALIGN_DISPARITY");
    if (!pred) {
      UG_REQUIRE(c.io_ready && T == c.T && H == c.H && W == c.W, "no resident depth of that shape");
      if (disparity) UG_REQUIRE(c.out_ready, "no resident disparity of that shape (run a clip first)");
    }
    const long plane = (long)H * W;
    const long P = T > o->stride ? 2L * (T - o->stride) : 0;
    UG_REQUIRE((double)P * (double)plane < 2147483648.0, "2^31 or more pair-pixels (2 * (T - stride) * H * W)");
    if (P == 0) { out4[0] = NAN; out4[1] = out4[2] = out4[3] = 0.0; return 0; }
    const long n = (long)T * plane, np_ = P * plane;
    const int nbs = eval_nblocks(plane);
    // the whole request is sized before the first allocation, so that a workspace too small is reported with the bytes the call needs
    auto r256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t need = r256((size_t)n * 4) + r256((size_t)T * 36) + r256((size_t)P * 96) + r256((size_t)np_ * 4) + r256((size_t)P * nbs * 16);
    if (pred || disparity) need += r256((size_t)n * 4);
    if (cmask) need += r256((size_t)n);
    if (warp_out) need += r256((size_t)np_ * 4);
    if (err_out) need += r256((size_t)np_ * 4);
    const size_t room = c.ws.capacity() - c.ws.mark();
    if (need > room)
      throw std::runtime_error("ug_eval_tae: the workspace is too small: this call needs " + std::to_string(need) + " bytes of it and " +
                               std::to_string(room) + " are free (raise workspace_bytes in ug_create)");
    DepthEvalBufs d{c.d_depth, nullptr, nullptr, n};
    if (pred || disparity) {
      float* dx = c.ws.get<float>(n);
      if (pred) UG_CHECK(hipMemcpy(dx, pred, n * 4, hipMemcpyHostToDevice));
      else launch_disparity_from_frames(c.d_out_frames, c.d_mm, dx, n, c.stream);
      d.dp = dx;
    }
    d.dg = c.ws.get<float>(n); UG_CHECK(hipMemcpy(d.dg, gt, n * 4, hipMemcpyHostToDevice));
    if (cmask) { d.dm = (unsigned char*)c.ws.alloc(n); UG_CHECK(hipMemcpy(d.dm, cmask, n, hipMemcpyHostToDevice)); }
    float* dk = c.ws.get<float>((long)T * 9); UG_CHECK(hipMemcpy(dk, K, (size_t)T * 36, hipMemcpyHostToDevice));
    double* drel = c.ws.get<double>(P * 12); UG_CHECK(hipMemcpy(drel, rel, (size_t)P * 96, hipMemcpyHostToDevice));
    unsigned* zbuf = c.ws.get<unsigned>(np_);
    double* part = c.ws.get<double>(P * nbs * 2);
    float* dwarp = warp_out ? c.ws.get<float>(np_) : nullptr;
    float* derr = err_out ? c.ws.get<float>(np_) : nullptr;
    TaeArgs a;
    a.s = o->s; a.t = o->t; a.floor_ = fl; a.plo = clip_lo(o->post_clip_min); a.phi = clip_hi(o->post_clip_max);
    a.md = depth_bound(o->max_depth); a.disparity = disparity ? 1 : 0; a.stride = o->stride;
    int nb = 0;
    launch_tae(d.dp, d.dg, d.dm, dk, drel, (int)P, H, W, a, zbuf, part, dwarp, derr, &nb, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    std::vector<double> hp((size_t)P * nb * 2);
    UG_CHECK(hipMemcpy(hp.data(), part, hp.size() * 8, hipMemcpyDeviceToHost));
    double tot = 0.0, pixels = 0.0; long scored = 0;
    for (long p = 0; p < P; ++p) {
      double sum = 0.0, cnt = 0.0;
      for (int b = 0; b < nb; ++b) { sum += hp[((size_t)p * nb + b) * 2]; cnt += hp[((size_t)p * nb + b) * 2 + 1]; }      // block order
      const double v = cnt > 0 ? sum / cnt : (double)NAN;
      if (cnt > 0) { tot += v; ++scored; pixels += cnt; }
      if (pair_out) { pair_out[p * 2] = v; pair_out[p * 2 + 1] = cnt; }
    }
    out4[0] = scored > 0 ? tot / (double)scored : (double)NAN; out4[1] = (double)scored; out4[2] = (double)P; out4[3] = pixels;
    if (warp_out) UG_CHECK(hipMemcpy(warp_out, dwarp, (size_t)np_ * 4, hipMemcpyDeviceToHost));
    if (err_out) UG_CHECK(hipMemcpy(err_out, derr, (size_t)np_ * 4, hipMemcpyDeviceToHost));
  });
}

void ug_pcd_opts_default(ug_pcd_opts* o) { o->threshold = 0.1f; o->max_iteration = 30; o->knn = 30; }

int ug_pcd_world_points(ug_ctx* x, const float* pred, const float* gt, const float* cam2world, const float* K, int T, int H, int W,
                        const ug_depth_eval_opts* o, float* out_fit, float* out_pts) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(o != nullptr, "options must not be NULL");
    UG_REQUIRE(o->alignment == UG_ALIGN_LSTSQ, "the world points align the depth with UG_ALIGN_LSTSQ (as ug_eval_depth_global)");
    UG_REQUIRE(gt && cam2world && K && out_fit, "gt_depth, cam2world, intrinsics and out_fit2 must not be NULL");
    const WorldFit f = world_first_fit(c, pred, gt, nullptr, nullptr, cam2world, K, T, H, W, o, 1L << 31);
    const long n = f.n;
    c.pcd_pixels = 0;
    if (c.pcd_cap < n) {
      if (c.d_pcd_pts) { (void)hipFree(c.d_pcd_pts); c.d_pcd_pts = nullptr; c.pcd_cap = 0; }
      UG_CHECK(hipMalloc((void**)&c.d_pcd_pts, (size_t)n * 12));
      c.pcd_cap = n;
    }
    launch_world_points(f.d.dp, f.dcam, n, H, W, f.b.plo, f.b.phi, (float)f.s, (float)f.t, c.d_pcd_pts, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    c.pcd_pixels = n;
    out_fit[0] = (float)f.s; out_fit[1] = (float)f.t;
    if (out_pts) UG_CHECK(hipMemcpy(out_pts, c.d_pcd_pts, (size_t)n * 12, hipMemcpyDeviceToHost));
  });
}

int ug_eval_pcd(ug_ctx* x, const float* pred_pts, const float* gt_pts, const unsigned char* mask, long n, const long* sample_idx, long n_sample,
                const ug_pcd_opts* o, double* out, float* pred_cloud_out, float* gt_cloud_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    eval_pcd_run(c, pred_pts, gt_pts, mask, n, sample_idx, n_sample, false, false, o, out, pred_cloud_out, gt_cloud_out, nullptr, nullptr, nullptr);
  });
}

int ug_eval_pcd_fps(ug_ctx* x, const float* pred_pts, const float* gt_pts, const unsigned char* mask, long n, long n_sample, const ug_pcd_opts* o,
                    double* out, float* pred_cloud_out, float* gt_cloud_out, long* pred_idx_out, long* gt_idx_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    eval_pcd_run(c, pred_pts, gt_pts, mask, n, nullptr, n_sample, true, false, o, out, pred_cloud_out, gt_cloud_out, pred_idx_out, gt_idx_out, nullptr);
  });
}
int ug_eval_pcd_ex(ug_ctx* x, const float* pred_pts, const float* gt_pts, const unsigned char* mask, long n, const long* sample_idx, long n_sample,
                   const ug_pcd_opts* o, int flags, double* out, float* pred_cloud_out, float* gt_cloud_out, long* pred_idx_out, long* gt_idx_out,
                   long* search_stats) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const unsigned unknown = (unsigned)flags & ~(unsigned)(UG_PCD_FPS | UG_PCD_SEARCH_GRID);
    if (unknown) {
      char hex[16]; snprintf(hex, sizeof hex, "0x%x", unknown);
      throw std::runtime_error(std::string("ug_eval_pcd_ex: unknown flag bits ") + hex + " (UG_PCD_FPS | UG_PCD_SEARCH_GRID)");
    }
    const bool fps = (flags & UG_PCD_FPS) != 0;
    UG_REQUIRE(!fps || !sample_idx, "UG_PCD_FPS picks the points itself: sample_idx must be NULL");
    eval_pcd_run(c, pred_pts, gt_pts, mask, n, sample_idx, n_sample, fps, (flags & UG_PCD_SEARCH_GRID) != 0, o, out, pred_cloud_out, gt_cloud_out,
                 pred_idx_out, gt_idx_out, search_stats);
  });
}
void ug_pcd_score_opts_default(ug_pcd_score_opts* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
}
int ug_eval_pcd_scores(ug_ctx* x, const float* pred_pts, const float* gt_pts, const unsigned char* mask, long n, const long* sample_idx, long n_sample,
                       const ug_pcd_opts* o, int flags, double* out, float* pred_cloud_out, float* gt_cloud_out, long* pred_idx_out, long* gt_idx_out,
                       long* search_stats, const ug_pcd_score_opts* so, long* score_counts, long* voxel_counts) {
  if (!so || (so->n_thresholds == 0 && so->n_voxel_sizes == 0))
    return ug_eval_pcd_ex(x, pred_pts, gt_pts, mask, n, sample_idx, n_sample, o, flags, out, pred_cloud_out, gt_cloud_out, pred_idx_out, gt_idx_out,
                          search_stats);
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(so->n_thresholds >= 0 && so->n_thresholds <= PCD_MAX_THRESHOLDS, "n_thresholds must be 0..8");
    UG_REQUIRE(so->n_voxel_sizes >= 0 && so->n_voxel_sizes <= PCD_MAX_VOXEL_SIZES, "n_voxel_sizes must be 0..4");
    for (int k = 0; k < so->n_thresholds; ++k)
      UG_REQUIRE(so->thresholds[k] > 0.0 && std::isfinite(so->thresholds[k]), "every threshold must be positive and finite");
    for (int k = 0; k < so->n_voxel_sizes; ++k)
      UG_REQUIRE(so->voxel_sizes[k] > 0.0 && std::isfinite(so->voxel_sizes[k]), "every voxel size must be positive and finite");
    UG_REQUIRE(so->n_thresholds == 0 || score_counts, "score_counts must not be NULL when thresholds are given");
    UG_REQUIRE(so->n_voxel_sizes == 0 || voxel_counts, "voxel_counts must not be NULL when voxel sizes are given");
    const unsigned unknown = (unsigned)flags & ~(unsigned)(UG_PCD_FPS | UG_PCD_SEARCH_GRID);
    if (unknown) {
      char hex[16]; snprintf(hex, sizeof hex, "0x%x", unknown);
      throw std::runtime_error(std::string("ug_eval_pcd_scores: unknown flag bits ") + hex + " (UG_PCD_FPS | UG_PCD_SEARCH_GRID)");
    }
    const bool fps = (flags & UG_PCD_FPS) != 0, grid = (flags & UG_PCD_SEARCH_GRID) != 0;
    UG_REQUIRE(!fps || !sample_idx, "UG_PCD_FPS picks the points itself: sample_idx must be NULL");
    UG_REQUIRE(mask && n > 0 && n < (1L << 31), "mask must not be NULL and n_pixels must be positive and below 2^31");
    for (int k = 0; k < 2 * so->n_thresholds; ++k) score_counts[k] = 0;      // what an empty mask returns
    for (int k = 0; k < 6 * so->n_voxel_sizes; ++k) voxel_counts[k] = 0;
    // the whole request is sized before the first allocation, so that a workspace too small is reported with the bytes the call needs
    long m = 0;
    for (long i = 0; i < n; ++i) m += mask[i] > 0;
    const bool sample = fps && n_sample > 0 && n_sample < m;
    const long ns = (sample_idx || sample) ? n_sample : m;
    UG_REQUIRE(ns >= 0 && ns < (1L << 31), "n_sample out of range");
    const size_t need = pcd_scores_request(n, m, ns, pred_pts != nullptr, sample_idx != nullptr, sample, grid, so->n_thresholds, so->n_voxel_sizes);
    const size_t room = c.ws.capacity() - c.ws.mark();
    if (need > room)
      throw std::runtime_error("ug_eval_pcd_scores: the workspace is too small: this call needs " + std::to_string(need) + " bytes of it and " +
                               std::to_string(room) + " are free (raise workspace_bytes in ug_create)");
    eval_pcd_run(c, pred_pts, gt_pts, mask, n, sample_idx, n_sample, fps, grid, o, out, pred_cloud_out, gt_cloud_out, pred_idx_out, gt_idx_out,
                 search_stats, so, score_counts, voxel_counts);
  });
}

// ---------------------------------------------------------------- focal, poses and depth from point maps (kernels/pointmap.hip)
void ug_pointmap_opts_default(ug_pointmap_opts* o) { o->reproj_px = 8.0; o->max_iter = 300; o->max_rounds = 5; }

int ug_pointmap_focal(ug_ctx* x, const float* pts0, int H, int W, double cx, double cy, double* focal_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(pts0 && focal_out, "pts0 and focal_out must not be NULL");
    UG_REQUIRE(H > 0 && W > 0, "H and W must be positive");
    const long n = (long)H * W;
    UG_REQUIRE(n < (1L << 31), "pixel count");
    float* d = c.ws.get<float>(n * 3); UG_CHECK(hipMemcpy(d, pts0, (size_t)n * 12, hipMemcpyHostToDevice));
    double* part = c.ws.get<double>(PM_MAXB * 2); double* fz = c.ws.get<double>(1);
    launch_pm_focal(d, n, PmCam{0.0, cx, cy, W}, 10, part, fz, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    double f = 0;
    UG_CHECK(hipMemcpy(&f, fz, 8, hipMemcpyDeviceToHost));
    *focal_out = f > 0.0 ? f : 0.0;      // clip(min = 0); a NaN (no usable pixel) comes out as 0
  });
}

// inverse of a 3x3 by the adjugate, as _inv3 of harness/pointmap.py
static void pm_inv3(const double m[3][3], double o[3][3]) {
  const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const double det = (m[0][0] * c00 + m[0][1] * c01) + m[0][2] * c02;
  const double adj[3][3] = {{c00, m[0][2] * m[2][1] - m[0][1] * m[2][2], m[0][1] * m[1][2] - m[0][2] * m[1][1]},
                            {c01, m[0][0] * m[2][2] - m[0][2] * m[2][0], m[0][2] * m[1][0] - m[0][0] * m[1][2]},
                            {c02, m[0][1] * m[2][0] - m[0][0] * m[2][1], m[0][0] * m[1][1] - m[0][1] * m[1][0]}};
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) o[r][k] = adj[r][k] / det;
}

// One fit of the orthogonal iteration over the pixels of `keep`, from pose.R; leaves (R, t) consistent and returns the iterations it took.
static int pm_fit(Ctx& c, const float* pts, const unsigned char* keep, long n, const PmCam& cam, PmPose& pose, int max_iter, double* part) {
  int nb = 0;
  double s0[8];
  launch_pm_pass0(pts, keep, n, cam, part, &nb, c.stream);
  UG_CHECK(hipGetLastError());
  fetch_partial_sums(c, part, nb, s0);
  const double cnt = s0[0];
  const double M[3][3] = {{1.0 - s0[1] / cnt, 0.0 - s0[2] / cnt, 0.0 - s0[3] / cnt},
                          {0.0 - s0[2] / cnt, 1.0 - s0[4] / cnt, 0.0 - s0[5] / cnt},
                          {0.0 - s0[3] / cnt, 0.0 - s0[5] / cnt, 1.0 - s0[6] / cnt}};
  double Mi[3][3];
  pm_inv3(M, Mi);
  const double floor = (1e-6 * 0x1p-48) * s0[7];      // a millionth of the float32 rounding of the input, sum (2^-24 |X|)^2
  double prev = -1.0;
  int it = 1;
  for (;; ++it) {
    double sg[3], s[17];
    launch_pm_pass1(pts, keep, n, cam, pose, part, &nb, c.stream);
    UG_CHECK(hipGetLastError());
    fetch_partial_sums(c, part, nb, sg);
    for (int r = 0; r < 3; ++r) pose.t[r] = ((Mi[r][0] * sg[0] + Mi[r][1] * sg[1]) + Mi[r][2] * sg[2]) / cnt;
    launch_pm_pass2(pts, keep, n, cam, pose, part, &nb, c.stream);
    UG_CHECK(hipGetLastError());
    fetch_partial_sums(c, part, nb, s);
    const double err = s[16];
    UG_REQUIRE(err == err, "the object-space error is NaN");
    if (err <= floor || (prev >= 0.0 && fabs(prev - err) <= std::max(1e-12 * prev, floor)) || it == max_iter) break;
    double T44[16];
    pcd_host::umeyama_from_sums(s, T44);      // s = n, sum X, sum q, sum q X^T: the rotation of the centred X onto the centred q
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) pose.R[r * 3 + k] = T44[r * 4 + k];
    prev = err;
  }
  return it;
}

int ug_pointmap_poses(ug_ctx* x, const float* pts, const unsigned char* mask, int T, int H, int W, double focal, double cx, double cy,
                      const ug_pointmap_opts* o, double* ext_out, float* depth_out, double* stats_out, unsigned char* inliers_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(pts && o, "pts and options must not be NULL");
    UG_REQUIRE(ext_out && depth_out && stats_out, "extrinsics_out, depth_out and frame_stats_out must not be NULL");
    UG_REQUIRE(T > 0 && H > 0 && W > 0, "T, H and W must be positive");
    const long n = (long)H * W;
    UG_REQUIRE(n < (1L << 31), "pixel count");
    UG_REQUIRE(focal > 0.0 && std::isfinite(focal) && std::isfinite(cx) && std::isfinite(cy), "the focal must be positive and finite");
    UG_REQUIRE(o->reproj_px > 0.0 && o->max_iter >= 1 && o->max_rounds >= 0, "reproj_px must be positive, max_iter >= 1 and max_rounds >= 0");
    float* dp = c.ws.get<float>(n * 3);
    unsigned char* dm = mask ? (unsigned char*)c.ws.alloc(n) : nullptr;
    unsigned char* valid = (unsigned char*)c.ws.alloc(n);
    unsigned char* kbuf[2] = {(unsigned char*)c.ws.alloc(n), (unsigned char*)c.ws.alloc(n)};
    float* dd = c.ws.get<float>(n);
    double* part = c.ws.get<double>(PM_MAXB * 17);
    const PmCam cam{focal, cx, cy, W};
    const double thr2 = o->reproj_px * o->reproj_px;
    PmPose pose;
    for (int i = 0; i < 9; ++i) pose.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) pose.t[i] = 0.0;
    for (int f = 0; f < T; ++f) {
      UG_CHECK(hipMemcpy(dp, pts + (size_t)f * n * 3, (size_t)n * 12, hipMemcpyHostToDevice));
      if (mask) UG_CHECK(hipMemcpy(dm, mask + (size_t)f * n, n, hipMemcpyHostToDevice));
      launch_pm_valid(dp, dm, n, valid, c.stream);
      const unsigned char* keep = valid;      // the first fit takes every valid pixel; their count is the first of the pass-0 sums
      int nb = 0;
      double s0[8];
      launch_pm_pass0(dp, valid, n, cam, part, &nb, c.stream);
      UG_CHECK(hipGetLastError());
      fetch_partial_sums(c, part, nb, s0);
      if (s0[0] < 4.0) {
        char msg[96]; snprintf(msg, sizeof msg, "ug_pointmap_poses: frame %d has %ld valid pixels; a pose needs at least 4", f, (long)s0[0]);
        throw std::runtime_error(msg);
      }
      int iters = 0;
      double in3[3] = {0, 0, 0};
      unsigned char* fresh = kbuf[0];
      for (int rnd = 0;; ++rnd) {
        iters += pm_fit(c, dp, keep, n, cam, pose, o->max_iter, part);
        launch_pm_inliers(dp, valid, keep, n, cam, pose, thr2, fresh, part, &nb, c.stream);
        UG_CHECK(hipGetLastError());
        fetch_partial_sums(c, part, nb, in3);
        if (in3[1] == 0.0 || rnd == o->max_rounds || in3[0] < 4.0) break;
        keep = fresh;
        fresh = fresh == kbuf[0] ? kbuf[1] : kbuf[0];
      }
      launch_pm_depth(dp, valid, n, pose, dd, c.stream);
      UG_CHECK(hipGetLastError());
      UG_CHECK(hipStreamSynchronize(c.stream));
      UG_CHECK(hipMemcpy(depth_out + (size_t)f * n, dd, (size_t)n * 4, hipMemcpyDeviceToHost));
      if (inliers_out) UG_CHECK(hipMemcpy(inliers_out + (size_t)f * n, fresh, n, hipMemcpyDeviceToHost));
      double* E = ext_out + (size_t)f * 16;
      for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) E[r * 4 + k] = pose.R[r * 3 + k]; E[r * 4 + 3] = pose.t[r]; }
      E[12] = 0; E[13] = 0; E[14] = 0; E[15] = 1;
      stats_out[f * 3] = in3[0]; stats_out[f * 3 + 1] = (double)iters; stats_out[f * 3 + 2] = in3[0] > 0 ? sqrt(in3[2] / in3[0]) : NAN;
    }
  });
}

int ug_eval_normal(ug_ctx* x, const float* pred, const float* gt, const unsigned char* mask, long n, double* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const float* dp;
    if (pred) { float* d = c.ws.get<float>(n * 3); UG_CHECK(hipMemcpy(d, pred, n * 12, hipMemcpyHostToDevice)); dp = d; }
    else { UG_REQUIRE(c.io_ready && n == (long)c.T * c.H * c.W, "no resident normals of that size"); dp = c.d_normals; }
    float* dg = c.ws.get<float>(n * 3); UG_CHECK(hipMemcpy(dg, gt, n * 12, hipMemcpyHostToDevice));
    unsigned char* dm = nullptr;
    if (mask) { dm = (unsigned char*)c.ws.alloc(n); UG_CHECK(hipMemcpy(dm, mask, n, hipMemcpyHostToDevice)); }
    float* err = c.ws.get<float>(n);
    double* part = c.ws.get<double>(EVAL_MAXB * 8);
    unsigned* hist = (unsigned*)c.ws.alloc(4097 * 4);
    UG_CHECK(hipMemsetAsync(hist, 0, 4097 * 4, c.stream));
    int nb = 0;
    launch_normal_err(dp, dg, dm, n, err, part, hist, &nb, c.stream);
    double m[8];
    fetch_partial_sums(c, part, nb, m);
    std::vector<unsigned> hh(4096);
    UG_CHECK(hipMemcpy(hh.data(), hist, 4096 * 4, hipMemcpyDeviceToHost));
    const long cnt = (long)m[0];
    if (cnt <= 0) {   // empty mask: NaN metrics like the reference's mean over an empty selection; MetricsManager skips NaN
      for (int k = 0; k < 8; ++k) out[k] = NAN;
      return 0;
    }
    // torch.median = lower median = element (cnt-1)/2 of the sorted errors: find its bin, then sort that bin only
    const long kth = (cnt - 1) / 2;
    long acc = 0; int bin = 0;
    for (; bin < 4096; ++bin) { if (acc + hh[bin] > kth) break; acc += hh[bin]; }
    const unsigned cap = hh[bin];
    float* binv = c.ws.get<float>(cap);
    unsigned* cntd = hist + 4096;
    launch_collect_bin(err, n, bin, binv, cntd, cap, c.stream);
    UG_CHECK(hipStreamSynchronize(c.stream));
    std::vector<float> bv(cap);
    UG_CHECK(hipMemcpy(bv.data(), binv, (size_t)cap * 4, hipMemcpyDeviceToHost));
    std::sort(bv.begin(), bv.end());
    out[0] = m[1] / cnt; out[1] = bv[kth - acc]; out[2] = sqrt(m[2] / cnt);
    for (int k = 0; k < 5; ++k) out[3 + k] = 100.0 * m[3 + k] / cnt;
  });
}

// ---------------------------------------------------------------- visualisation panels (kernels/vis.hip)
int ug_vis_depth_range(ug_ctx* x, const float* depth, long n, float* out2) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(out2 != nullptr, "out2 must not be NULL");
    UG_REQUIRE(n >= 0, "n must not be negative");
    UG_REQUIRE(depth || (c.io_ready && n == (long)c.T * c.H * c.W), "no resident depth of that size");
    out2[0] = out2[1] = 0.f;
    if (n == 0) return 0;
    const float* dd = c.d_depth;
    if (depth) { float* d = c.ws.get<float>(n); UG_CHECK(hipMemcpy(d, depth, (size_t)n * 4, hipMemcpyHostToDevice)); dd = d; }
    float* part = c.ws.get<float>(2 * 1024 + 2);
    launch_vis_range(dd, n, part, part + 2 * 1024, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(out2, part + 2 * 1024, 8, hipMemcpyDeviceToHost));
  });
}

int ug_vis_panels(ug_ctx* x, const float* depth, const float* normals, const float* rgbs, int rgb_mode, int T, int H, int W, float vmin, float vmax,
                  const float* lut, const float* cbar, int Wc, unsigned char* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(lut && out, "lut_256x3 and panels_out must not be NULL");
    UG_REQUIRE(T > 0 && H > 0 && W > 0, "T, H and W must be positive");
    UG_REQUIRE(Wc >= 0 && !(cbar && Wc == 0), "Wc must not be negative, and positive when a colour bar is given");
    UG_REQUIRE(rgb_mode == UG_VIS_RGB_NONE || rgb_mode == UG_VIS_RGB_HOST || rgb_mode == UG_VIS_RGB_RESIDENT,
               "unknown rgb_mode (UG_VIS_RGB_NONE / HOST / RESIDENT)");
    UG_REQUIRE(rgb_mode != UG_VIS_RGB_HOST || rgbs, "rgbs must not be NULL with UG_VIS_RGB_HOST");
    const long rows = (long)T * H;
    const long Wp = (rgb_mode != UG_VIS_RGB_NONE ? (long)W : 0) + 2L * W + (cbar ? 5L + Wc : 0);
    UG_REQUIRE(rows < (1L << 31) && rows * Wp * 3 < (1L << 31), "the panels must stay below 2^31 bytes");
    const bool same = c.io_ready && T == c.T && H == c.H && W == c.W;
    UG_REQUIRE(depth || same, "no resident depth of that shape");
    UG_REQUIRE(normals || (same && c.normals_ready), "no resident normals of that shape (the last run must have had with_normals = 1)");
    UG_REQUIRE(rgb_mode != UG_VIS_RGB_RESIDENT || same, "no resident input frames of that shape");
    const long px = rows * W;
    auto up = [&](const float* h, long n) { float* d = c.ws.get<float>(n); UG_CHECK(hipMemcpyAsync(d, h, (size_t)n * 4, hipMemcpyHostToDevice, c.stream)); return (const float*)d; };
    const float* dd = depth ? up(depth, px) : c.d_depth;
    const float* dn = normals ? up(normals, px * 3) : c.d_normals;
    const float* dr = rgb_mode == UG_VIS_RGB_HOST ? up(rgbs, px * 3) : (rgb_mode == UG_VIS_RGB_RESIDENT ? c.d_frames : nullptr);
    const float* dl = up(lut, 768);
    const float* dc = cbar ? up(cbar, (long)H * Wc * 3) : nullptr;
    const size_t bytes = (size_t)(rows * Wp * 3);
    unsigned char* dout = (unsigned char*)c.ws.alloc(bytes);
    launch_vis_panel(dr, dn, dd, dl, dc, dout, T, H, W, Wc, vmin, vmax, c.stream);
    UG_CHECK(hipGetLastError());
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
  });
}

// ---------------------------------------------------------------- ScanNet++ clip preparation (kernels/prep.hip)
int ug_prep_resize_frames(ug_ctx* x, const unsigned char* frames, int T, int Hi, int Wi, int Ho, int Wo, const int* row_idx, const double* row_w,
                          int Kr, const int* col_idx, const double* col_w, int Kc, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(frames && row_idx && row_w && col_idx && col_w && out, "frames, the four tap tables and out must not be NULL");
    UG_REQUIRE(T > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && Kr > 0 && Kc > 0, "T, the sizes and the tap counts must be positive");
    UG_REQUIRE((long)T * 3 * Ho * Wo < (1L << 31), "the output must stay below 2^31 elements");
    UG_REQUIRE((long)Ho * Kr < (1L << 31) && (long)Wo * Kc < (1L << 31), "tap table size");
    const int* dri; const double* drw; const int* dci; const double* dcw;
    prep_upload_taps(c, row_idx, row_w, Ho, Kr, Hi, &dri, &drw);
    prep_upload_taps(c, col_idx, col_w, Wo, Kc, Wi, &dci, &dcw);
    const size_t in_f = (size_t)Hi * Wi * 3, mid_f = (size_t)3 * Ho * Wi, out_f = (size_t)3 * Ho * Wo;
    const int Tc = prep_chunk_frames(T, in_f + mid_f * 8 + out_f * 4);
    unsigned char* din = (unsigned char*)c.ws.alloc(in_f * Tc);
    double* dmid = c.ws.get<double>((long)(mid_f * Tc));
    float* dout = c.ws.get<float>((long)(out_f * Tc));
    for (int t0 = 0; t0 < T; t0 += Tc) {
      const int tc = std::min(Tc, T - t0);
      UG_CHECK(hipMemcpy(din, frames + in_f * t0, in_f * tc, hipMemcpyHostToDevice));
      launch_prep_resize(din, dri, drw, Kr, dci, dcw, Kc, tc, Hi, Wi, Ho, Wo, dmid, dout, c.stream);
      UG_CHECK(hipGetLastError());
      UG_CHECK(hipStreamSynchronize(c.stream));
      UG_CHECK(hipMemcpy(out + out_f * t0, dout, out_f * tc * 4, hipMemcpyDeviceToHost));
    }
  });
}

// What ug_prep_gt_ex and ug_prep_gt_normals share: the pick tables, checked against the source size before anything is uploaded, and the
// per-frame camera table (20 doubles: fx, fy, cx, cy, M33 row-major, t3, 4 unused) on the device
static void prep_upload_cameras(Ctx& c, const float* K, const float* M, int T, const int* row_idx, int Ho, int Hi, const int* col_idx, int Wo, int Wi,
                                double** dcam, int** dri, int** dci) {
  for (int i = 0; i < Ho; ++i) UG_REQUIRE(row_idx[i] >= 0 && row_idx[i] < Hi, "a row index lies outside the source");
  for (int i = 0; i < Wo; ++i) UG_REQUIRE(col_idx[i] >= 0 && col_idx[i] < Wi, "a column index lies outside the source");
  std::vector<double> tab((size_t)T * 20, 0.0);
  for (int f = 0; f < T; ++f) {
    const float* k = K + (size_t)f * 9; const float* m = M + (size_t)f * 16; double* q = tab.data() + (size_t)f * 20;
    q[0] = k[0]; q[1] = k[4]; q[2] = k[2]; q[3] = k[5];
    for (int r = 0; r < 3; ++r) { for (int j = 0; j < 3; ++j) q[4 + r * 3 + j] = m[r * 4 + j]; q[13 + r] = m[r * 4 + 3]; }
  }
  *dcam = c.ws.get<double>((long)T * 20); UG_CHECK(hipMemcpy(*dcam, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  *dri = c.ws.get<int>(Ho); UG_CHECK(hipMemcpy(*dri, row_idx, (size_t)Ho * 4, hipMemcpyHostToDevice));
  *dci = c.ws.get<int>(Wo); UG_CHECK(hipMemcpy(*dci, col_idx, (size_t)Wo * 4, hipMemcpyHostToDevice));
}

int ug_prep_gt_ex(ug_ctx* x, const unsigned short* depth, float depth_divisor, const unsigned char* normals, const float* K, const float* M, int T,
                  int Hi, int Wi, const int* row_idx, int Ho, const int* col_idx, int Wo, float max_depth, float* cam_normal, float* cam_coord,
                  float* world_normal, float* world_coord, float* mask, unsigned flags) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const unsigned unknown = flags & ~(unsigned)(UG_PREP_DEPTH_F64 | UG_PREP_ZOOMED);
    if (unknown) {
      char hex[16]; snprintf(hex, sizeof hex, "0x%x", unknown);
      throw std::runtime_error(std::string("ug_prep_gt_ex: unknown flag bits ") + hex + " (UG_PREP_DEPTH_F64 | UG_PREP_ZOOMED)");
    }
    UG_REQUIRE(depth && K && M && row_idx && col_idx, "depth, intrinsics, cam2key, row_idx and col_idx must not be NULL");
    UG_REQUIRE(cam_coord && world_coord && mask, "cam_coord, world_coord and mask must not be NULL");
    UG_REQUIRE(!normals || (cam_normal && world_normal), "cam_normal and world_normal must not be NULL when normals are given");
    UG_REQUIRE(T > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "T and the sizes must be positive");
    UG_REQUIRE((long)T * 3 * Ho * Wo < (1L << 31), "the outputs must stay below 2^31 elements");
    double* dcam; int* dri; int* dci;
    prep_upload_cameras(c, K, M, T, row_idx, Ho, Hi, col_idx, Wo, Wi, &dcam, &dri, &dci);
    const size_t src_f = (size_t)Hi * Wi, px_f = (size_t)Ho * Wo;
    const int Tc = prep_chunk_frames(T, src_f * (normals ? 5 : 2) + px_f * 13 * 4);
    unsigned short* dd = (unsigned short*)c.ws.alloc(src_f * 2 * Tc);
    unsigned char* dn = normals ? (unsigned char*)c.ws.alloc(src_f * 3 * Tc) : nullptr;
    float* o_cn = cam_normal ? c.ws.get<float>((long)(px_f * 3 * Tc)) : nullptr;
    float* o_wn = world_normal ? c.ws.get<float>((long)(px_f * 3 * Tc)) : nullptr;
    float* o_cc = c.ws.get<float>((long)(px_f * 3 * Tc));
    float* o_wc = c.ws.get<float>((long)(px_f * 3 * Tc));
    float* o_m = c.ws.get<float>((long)(px_f * Tc));
    for (int t0 = 0; t0 < T; t0 += Tc) {
      const int tc = std::min(Tc, T - t0);
      UG_CHECK(hipMemcpy(dd, depth + src_f * t0, src_f * 2 * tc, hipMemcpyHostToDevice));
      if (normals) { UG_CHECK(hipMemcpy(dn, normals + src_f * 3 * t0, src_f * 3 * tc, hipMemcpyHostToDevice)); }
      launch_prep_gt(dd, dn, dcam + (size_t)t0 * 20, dri, dci, tc, Hi, Wi, Ho, Wo, depth_divisor, max_depth, (flags & UG_PREP_DEPTH_F64) != 0,
                     (flags & UG_PREP_ZOOMED) != 0, o_cn, o_wn, o_cc, o_wc, o_m, c.stream);
      UG_CHECK(hipGetLastError());
      UG_CHECK(hipStreamSynchronize(c.stream));
      const size_t n3 = px_f * 3 * tc * 4, off3 = px_f * 3 * t0;
      if (cam_normal) { UG_CHECK(hipMemcpy(cam_normal + off3, o_cn, n3, hipMemcpyDeviceToHost)); }
      if (world_normal) { UG_CHECK(hipMemcpy(world_normal + off3, o_wn, n3, hipMemcpyDeviceToHost)); }
      UG_CHECK(hipMemcpy(cam_coord + off3, o_cc, n3, hipMemcpyDeviceToHost));
      UG_CHECK(hipMemcpy(world_coord + off3, o_wc, n3, hipMemcpyDeviceToHost));
      UG_CHECK(hipMemcpy(mask + px_f * t0, o_m, px_f * tc * 4, hipMemcpyDeviceToHost));
    }
  });
}

int ug_prep_gt(ug_ctx* x, const unsigned short* depth, float depth_divisor, const unsigned char* normals, const float* K, const float* M, int T,
               int Hi, int Wi, const int* row_idx, int Ho, const int* col_idx, int Wo, float max_depth, float* cam_normal, float* cam_coord,
               float* world_normal, float* world_coord, float* mask) {
  return ug_prep_gt_ex(x, depth, depth_divisor, normals, K, M, T, Hi, Wi, row_idx, Ho, col_idx, Wo, max_depth, cam_normal, cam_coord, world_normal,
                       world_coord, mask, (Ho != Hi || Wo != Wi) ? UG_PREP_ZOOMED : 0);
}

// ---------------------------------------------------------------- normals fitted from the depth (kernels/gt_normals.hip)
void ug_gt_normals_opts_default(ug_gt_normals_opts* o) {
  if (!o) return;
  o->radius = 2; o->edge = 0.05; o->min_count = 0;      // radius 2 = the reference's patch_size 5; edge and the majority count are design choices
}

int ug_prep_gt_normals(ug_ctx* x, const unsigned short* depth, float depth_divisor, const float* K, const float* M, int T, int Hi, int Wi,
                       const int* row_idx, int Ho, const int* col_idx, int Wo, float max_depth, const ug_gt_normals_opts* opts, float* cam_normal,
                       float* world_normal, float* normal_mask, unsigned flags) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    ug_gt_normals_opts o;
    if (opts) o = *opts; else ug_gt_normals_opts_default(&o);
    const unsigned unknown = flags & ~(unsigned)(UG_PREP_DEPTH_F64 | UG_PREP_ZOOMED);
    if (unknown) {
      char hex[16]; snprintf(hex, sizeof hex, "0x%x", unknown);
      throw std::runtime_error(std::string("ug_prep_gt_normals: unknown flag bits ") + hex + " (UG_PREP_DEPTH_F64 | UG_PREP_ZOOMED)");
    }
    UG_REQUIRE(depth && K && M && row_idx && col_idx, "depth, intrinsics, cam2key, row_idx and col_idx must not be NULL");
    UG_REQUIRE(cam_normal && world_normal && normal_mask, "cam_normal, world_normal and normal_mask must not be NULL");
    UG_REQUIRE(T > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "T and the sizes must be positive");
    UG_REQUIRE(o.radius >= 1 && o.radius <= 8, "radius must lie in 1..8");
    UG_REQUIRE(o.edge == o.edge, "edge must not be NaN (negative: the edge test is off)");
    UG_REQUIRE(o.min_count >= 0, "min_count must not be negative (0: the majority of the window)");
    UG_REQUIRE((long)T * 3 * Ho * Wo < (1L << 31), "the outputs must stay below 2^31 elements");
    double* dcam; int* dri; int* dci;
    prep_upload_cameras(c, K, M, T, row_idx, Ho, Hi, col_idx, Wo, Wi, &dcam, &dri, &dci);
    const size_t src_f = (size_t)Hi * Wi, px_f = (size_t)Ho * Wo;
    const int Tc = prep_chunk_frames(T, src_f * 2 + px_f * 7 * 4);
    unsigned short* dd = (unsigned short*)c.ws.alloc(src_f * 2 * Tc);
    float* o_cn = c.ws.get<float>((long)(px_f * 3 * Tc));
    float* o_wn = c.ws.get<float>((long)(px_f * 3 * Tc));
    float* o_m = c.ws.get<float>((long)(px_f * Tc));
    GtNormalsArgs a;
    a.row_idx = dri; a.col_idx = dci; a.cam_normal = o_cn; a.world_normal = o_wn; a.normal_mask = o_m;
    a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.zoomed = (flags & UG_PREP_ZOOMED) != 0; a.depth_f64 = (flags & UG_PREP_DEPTH_F64) != 0;
    a.divisor = depth_divisor; a.max_depth = max_depth; a.radius = o.radius;
    a.min_count = o.min_count > 0 ? o.min_count : (2 * o.radius + 1) * (2 * o.radius + 1) / 2 + 1;
    a.edge_on = o.edge >= 0; a.edge = o.edge;
    for (int t0 = 0; t0 < T; t0 += Tc) {
      const int tc = std::min(Tc, T - t0);
      UG_CHECK(hipMemcpy(dd, depth + src_f * t0, src_f * 2 * tc, hipMemcpyHostToDevice));
      a.depth = dd; a.cam = dcam + (size_t)t0 * 20; a.n = (long)px_f * tc;
      ProfRec r; r.name = "gt_normals"; r.flops = 0; r.bytes = (double)src_f * tc * 2 + (double)px_f * tc * 28;      // under ug_profile_begin only
      if (c.prof_on) { UG_CHECK(hipEventCreate(&r.e0)); UG_CHECK(hipEventCreate(&r.e1)); UG_CHECK(hipEventRecord(r.e0, c.stream)); }
      launch_prep_gt_normals(a, c.stream);
      if (c.prof_on) { UG_CHECK(hipEventRecord(r.e1, c.stream)); c.prof.push_back(r); }
      UG_CHECK(hipGetLastError());
      UG_CHECK(hipStreamSynchronize(c.stream));
      const size_t n3 = px_f * 3 * tc * 4, off3 = px_f * 3 * t0;
      UG_CHECK(hipMemcpy(cam_normal + off3, o_cn, n3, hipMemcpyDeviceToHost));
      UG_CHECK(hipMemcpy(world_normal + off3, o_wn, n3, hipMemcpyDeviceToHost));
      UG_CHECK(hipMemcpy(normal_mask + px_f * t0, o_m, px_f * tc * 4, hipMemcpyDeviceToHost));
    }
  });
}

// ---------------------------------------------------------------- 7-Scenes depth registration (kernels/register.hip)
// Depth focal length from the 7-Scenes page, colour focal length and the depth-to-colour transform from the Kinect calibration the reference's
// dataset/sevenScenes/preprocess.py cites: https://projet.liris.cnrs.fr/voir/activities-dataset/kinect-calibration.html
void ug_register_opts_default(ug_register_opts* o) {
  if (!o) return;
  static const double m[12] = {9.9996518012567637e-01,  2.6765126468950343e-03, -7.9041012313000904e-03, -2.5558943178152542e-02,
                               -2.7409311281316700e-03, 9.9996302803027592e-01, -8.1504520778013286e-03, 1.0109636268061706e-04,
                               7.8819942130445332e-03,  8.1718328771890631e-03, 9.9993554558014031e-01,  2.0318321729487039e-03};
  o->src_focal = 585.0; o->dst_focal = 525.0;
  memcpy(o->src2dst, m, sizeof(m));
  o->divisor = 1000.f; o->max_valid = 100.f; o->flags = 0;
}

int ug_prep_register_depth(ug_ctx* x, const unsigned short* depth, int T, int H, int W, const ug_register_opts* opts, unsigned short* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    ug_register_opts o;
    if (opts) o = *opts; else ug_register_opts_default(&o);
    const unsigned unknown = o.flags & ~(unsigned)UG_REG_DROP_SENTINEL;
    if (unknown) {
      char hex[16]; snprintf(hex, sizeof hex, "0x%x", unknown);
      throw std::runtime_error(std::string("ug_prep_register_depth: unknown flag bits ") + hex + " (UG_REG_DROP_SENTINEL)");
    }
    UG_REQUIRE(depth && out, "depth_u16 and out must not be NULL");
    UG_REQUIRE(T > 0 && H > 0 && W > 0, "T, H and W must be positive");
    UG_REQUIRE((long)T * H * W < (1L << 31), "T * H * W must stay below 2^31");
    UG_REQUIRE(std::isfinite(o.src_focal) && o.src_focal > 0 && std::isfinite(o.dst_focal) && o.dst_focal > 0, "src_focal and dst_focal must be finite and positive");
    UG_REQUIRE(std::isfinite(o.divisor) && o.divisor > 0 && std::isfinite(o.max_valid) && o.max_valid > 0, "divisor and max_valid must be finite and positive");
    RegArgs a;
    a.src_focal = o.src_focal; a.dst_focal = o.dst_focal; a.divisor = o.divisor; a.max_valid = o.max_valid;
    a.drop_sentinel = (o.flags & UG_REG_DROP_SENTINEL) != 0;
    for (int i = 0; i < 12; ++i) { UG_REQUIRE(std::isfinite(o.src2dst[i]), "src2dst must be finite"); a.m[i] = o.src2dst[i]; }
    const size_t px_f = (size_t)H * W;
    const int Tc = prep_chunk_frames(T, px_f * 8);             // per pixel: 2 bytes in, a 4-byte z-buffer word, 2 bytes out
    unsigned short* dd = (unsigned short*)c.ws.alloc(px_f * 2 * Tc);
    unsigned* dz = c.ws.get<unsigned>((long)(px_f * Tc));
    unsigned short* dout = (unsigned short*)c.ws.alloc(px_f * 2 * Tc);
    for (int t0 = 0; t0 < T; t0 += Tc) {
      const int tc = std::min(Tc, T - t0);
      UG_CHECK(hipMemcpy(dd, depth + px_f * t0, px_f * 2 * tc, hipMemcpyHostToDevice));
      ProfRec r; r.name = "register_depth"; r.flops = 0; r.bytes = (double)px_f * tc * 12;    // fill 4, splat 2 + 4, finalize 4 + 2; under ug_profile_begin only
      if (c.prof_on) { UG_CHECK(hipEventCreate(&r.e0)); UG_CHECK(hipEventCreate(&r.e1)); UG_CHECK(hipEventRecord(r.e0, c.stream)); }
      launch_register_depth(dd, tc, H, W, a, dz, dout, c.stream);
      if (c.prof_on) { UG_CHECK(hipEventRecord(r.e1, c.stream)); c.prof.push_back(r); }
      UG_CHECK(hipGetLastError());
      UG_CHECK(hipStreamSynchronize(c.stream));
      UG_CHECK(hipMemcpy(out + px_f * t0, dout, px_f * 2 * tc, hipMemcpyDeviceToHost));
    }
  });
}

// ---------------------------------------------------------------- ScanNet++ mesh renderer (kernels/render.hip)
void ug_render_opts_default(ug_render_opts* o) {
  if (!o) return;
  o->znear = 0.05; o->zfar = 20.0; o->flags = 0;      // preprocess_scannetpp_imu.py:340-341
}

int ug_prep_render_mesh(ug_ctx* x, const float* verts, long NV, const int* faces, long NF, const double* world2cam, const double* K, int T, int H,
                        int W, const unsigned char* mask, const ug_render_opts* opts, unsigned short* depth_mm, unsigned char* normal,
                        int* tri_index) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    ug_render_opts o;
    if (opts) o = *opts; else ug_render_opts_default(&o);
    if (o.flags) {
      char hex[16]; snprintf(hex, sizeof hex, "0x%x", o.flags);
      throw std::runtime_error(std::string("ug_prep_render_mesh: unknown flag bits ") + hex + " (none is defined)");
    }
    UG_REQUIRE(verts && faces && world2cam && K && depth_mm && normal, "verts, faces, world2cam, K, depth_mm and normal must not be NULL");
    UG_REQUIRE(NV > 0 && NF > 0 && T > 0 && H > 0 && W > 0, "NV, NF, T, H and W must be positive");
    UG_REQUIRE(NF < (1L << 31) && NV < (1L << 31), "NF and NV must stay below 2^31");
    UG_REQUIRE((long)T * H * W < (1L << 31), "T * H * W must stay below 2^31");
    UG_REQUIRE(std::isfinite(o.znear) && o.znear > 0, "znear must be finite and positive");
    UG_REQUIRE(std::isfinite(o.zfar) && o.zfar > o.znear, "zfar must be finite and larger than znear");
    UG_REQUIRE(o.zfar <= 65.535, "zfar must not exceed 65.535: depth_mm holds 16 bits of millimetres");
    for (long i = 0; i < (long)T * 12; ++i) UG_REQUIRE(std::isfinite(world2cam[i]), "world2cam must be finite");
    for (long i = 0; i < (long)T * 4; ++i) UG_REQUIRE(std::isfinite(K[i]), "K (fx, fy, cx, cy) must be finite");
    for (int t = 0; t < T; ++t) UG_REQUIRE(K[4 * t] > 0 && K[4 * t + 1] > 0, "fx and fy must be positive");
    for (long i = 0; i < NV * 3; ++i) UG_REQUIRE(std::isfinite(verts[i]), "a vertex is not finite");
    for (long i = 0; i < NF * 3; ++i) UG_REQUIRE(faces[i] >= 0 && faces[i] < NV, "a face index lies outside 0..NV-1");
    std::vector<double> tab((size_t)T * 16);
    for (int t = 0; t < T; ++t) {
      memcpy(tab.data() + (size_t)t * 16, world2cam + (size_t)t * 12, 12 * sizeof(double));
      memcpy(tab.data() + (size_t)t * 16 + 12, K + (size_t)t * 4, 4 * sizeof(double));
    }
    float* dv = c.ws.get<float>(NV * 3); UG_CHECK(hipMemcpy(dv, verts, (size_t)NV * 12, hipMemcpyHostToDevice));      // the mesh: once per call
    int* df = c.ws.get<int>(NF * 3); UG_CHECK(hipMemcpy(df, faces, (size_t)NF * 12, hipMemcpyHostToDevice));
    double* dcam = c.ws.get<double>((long)T * 16); UG_CHECK(hipMemcpy(dcam, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    const size_t px_f = (size_t)H * W;
    const int Tc = prep_chunk_frames(T, px_f * 18);      // per pixel: an 8-byte z-buffer word, 2 + 3 + 4 bytes out, 1 byte of mask
    const size_t px_c = px_f * Tc;
    RenderBufs b;
    b.big_cap = 2u << 20;      // entries of the large-box list, 12 bytes each; a box that finds it full is walked by its own thread
    b.zbuf = (unsigned long long*)c.ws.alloc(px_c * 8);
    b.big_id = (long long*)c.ws.alloc((size_t)b.big_cap * 8);
    b.big_tile = c.ws.get<int>((long)b.big_cap);
    b.big_count = (unsigned long long*)c.ws.alloc(8);
    b.depth = (unsigned short*)c.ws.alloc(px_c * 2);
    b.normal = (unsigned char*)c.ws.alloc(px_c * 3);
    b.tri = tri_index ? c.ws.get<int>((long)px_c) : nullptr;
    unsigned char* dm = mask ? (unsigned char*)c.ws.alloc(px_c) : nullptr;
    for (int t0 = 0; t0 < T; t0 += Tc) {
      const int tc = std::min(Tc, T - t0);
      if (mask) { UG_CHECK(hipMemcpy(dm, mask + px_f * t0, px_f * tc, hipMemcpyHostToDevice)); }
      ProfRec r; r.name = "render_mesh"; r.flops = 0; r.bytes = (double)px_f * tc * 25;      // fill 8, resolve 8 + 9 per pixel; the splat's traffic depends on the view
      if (c.prof_on) { UG_CHECK(hipEventCreate(&r.e0)); UG_CHECK(hipEventCreate(&r.e1)); UG_CHECK(hipEventRecord(r.e0, c.stream)); }
      launch_render_mesh(dv, df, NF, dcam + (size_t)t0 * 16, tc, H, W, o.znear, o.zfar, dm, b, c.stream);
      if (c.prof_on) { UG_CHECK(hipEventRecord(r.e1, c.stream)); c.prof.push_back(r); }
      UG_CHECK(hipGetLastError());
      UG_CHECK(hipStreamSynchronize(c.stream));
      UG_CHECK(hipMemcpy(depth_mm + px_f * t0, b.depth, px_f * 2 * tc, hipMemcpyDeviceToHost));
      UG_CHECK(hipMemcpy(normal + px_f * 3 * t0, b.normal, px_f * 3 * tc, hipMemcpyDeviceToHost));
      if (tri_index) { UG_CHECK(hipMemcpy(tri_index + px_f * t0, b.tri, px_f * 4 * tc, hipMemcpyDeviceToHost)); }
    }
  });
}

}  // extern "C"
