// extern "C" surface of libunigeo_hip.so (declared in include/unigeo_hip.h - the drop-in boundary - and include/unigeo_hip_test.h - test / tuning entry points).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/unigeo_hip.h"
#include "../../include/unigeo_hip_test.h"
#include "engine.h"

using namespace ug;

struct ug_ctx { Ctx c; };
static std::string g_create_err;

#define UG_TRY(ctx, ...)                                   \
  if (!(ctx)) return -1;                                   \
  try { UG_CHECK(hipSetDevice((ctx)->c.device)); __VA_ARGS__; return 0; } \
  catch (const std::exception& e) { (ctx)->c.err = e.what(); (void)hipGetLastError(); return 1; } \
  catch (...) { (ctx)->c.err = "unknown error"; return 2; }

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
    UG_CHECK(hipSetDevice(x->c.device));
    std::vector<long> sh(shape, shape + ndim);
    upload_raw(x->c, name, dtype, sh, host);
  });
}
int ug_bind_unet(ug_ctx* x, const ug_unet_config* g) {
  UG_TRY(x, {
    UNetCfg d; d.in_ch = g->in_channels; d.out_ch = g->out_channels; d.nlev = g->num_levels;
    UG_REQUIRE(d.nlev >= 2 && d.nlev <= 8, "num_levels");
    for (int i = 0; i < 8; ++i) { d.boc[i] = g->block_out_channels[i]; d.heads[i] = g->num_attention_heads[i]; d.has_attn[i] = g->down_has_attn[i]; }
    d.layers = g->layers_per_block; d.cross_dim = g->cross_attention_dim; d.add_dim = g->addition_time_embed_dim;
    d.proj_in_dim = g->projection_class_embeddings_input_dim; d.groups = g->norm_groups;
    d.eps_xattn = g->eps_cross_attn_blocks; d.eps_down = g->eps_plain_down_block; d.eps_mid = g->eps_mid_block; d.eps_up = g->eps_up_blocks;
    UG_REQUIRE(d.in_ch % 8 == 0, "UNet in_channels must be a multiple of 8");
    bind_unet(x->c, d, "unet.");
    finish_binding(x->c, "unet.");
  });
}
int ug_bind_vae(ug_ctx* x, const ug_vae_config* g) {
  UG_TRY(x, {
    VAECfg d; d.in_ch = g->in_channels; d.out_ch = g->out_channels; d.lat = g->latent_channels; d.nlev = g->num_levels;
    for (int i = 0; i < 8; ++i) d.boc[i] = g->block_out_channels[i];
    d.layers = g->layers_per_block; d.groups = g->norm_groups; d.scaling = g->scaling_factor;
    bind_vae(x->c, d, "vae.");
    finish_binding(x->c, "vae.");
  });
}
int ug_bind_clip(ug_ctx* x, const ug_clip_config* g) {
  UG_TRY(x, {
    CLIPCfg d; d.hidden = g->hidden_size; d.inter = g->intermediate_size; d.layers = g->num_hidden_layers; d.heads = g->num_attention_heads;
    d.image = g->image_size; d.patch = g->patch_size; d.proj = g->projection_dim; d.eps = g->layer_norm_eps;
    bind_clip(x->c, d, "clip.");
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
int ug_set_ff_fused(ug_ctx* x, int on) {
  if (!x) return -1;
  x->c.ff_fused = on & 3; x->c.lane_need.clear();   // bit 0: fused feed-forward kernel, bit 1: its pre-LayerNorm inside the kernel (a feature toggle changes the transient memory a lane task needs)
  return 0;
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
int ug_dc_set_trace(ug_ctx* x, float* host_latents, int steps) {
  if (!x) return -1;
  x->c.trace_host = host_latents; x->c.trace_steps = host_latents ? steps : 0;
  return 0;
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
int ug_profile_begin_shapes(ug_ctx* x) { UG_TRY(x, prof_begin(x->c, true)); }
const char* ug_profile_end(ug_ctx* x) {
  if (!x) return "{}";
  try { x->c.prof_json = prof_end(x->c); } catch (const std::exception& e) { x->c.err = e.what(); x->c.prof_json = "{}"; }
  return x->c.prof_json.c_str();
}

}  // extern "C"

// ------------------------------------------------------------------ host <-> device helpers (test entry points)
namespace {
struct Scope {
  Ctx& c; size_t mk;
  explicit Scope(Ctx& c_) : c(c_), mk(c_.ws.mark()) {}
  ~Scope() { (void)hipStreamSynchronize(c.stream); c.ws.release(mk); }
};
void upload16(const float* h, long n, f16* d) {   // float host -> f16 device, into d
  std::vector<f16> v((size_t)n);
  for (long i = 0; i < n; ++i) v[i] = (f16)h[i];
  UG_CHECK(hipMemcpy(d, v.data(), (size_t)n * 2, hipMemcpyHostToDevice));
}
f16* up16(Ctx& c, const float* h, long n) {
  f16* d = c.ws.get<f16>(n);
  upload16(h, n, d);
  return d;
}
f16* up16_opt(Ctx& c, const float* h, long n) { return h ? up16(c, h, n) : nullptr; }
void down16(Ctx& c, const f16* d, float* h, long n) {
  std::vector<f16> v((size_t)n);
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(v.data(), d, (size_t)n * 2, hipMemcpyDeviceToHost));
  for (long i = 0; i < n; ++i) h[i] = (float)v[i];
}
// NCHW float host -> NHWC(+channel pad) f16 device, into d (T*H*W*Cpad elements)
void upload_nchw(const float* h, int T, int C, int H, int W, int Cpad, f16* d) {
  std::vector<f16> v((size_t)T * H * W * Cpad, (f16)0.f);
  for (int t = 0; t < T; ++t)
    for (int ch = 0; ch < C; ++ch)
      for (long p = 0; p < (long)H * W; ++p) v[((size_t)t * H * W + p) * Cpad + ch] = (f16)h[((size_t)t * C + ch) * H * W + p];
  UG_CHECK(hipMemcpy(d, v.data(), v.size() * 2, hipMemcpyHostToDevice));
}
f16* up_nchw(Ctx& c, const float* h, int T, int C, int H, int W, int Cpad) {
  f16* d = c.ws.get<f16>((long)T * H * W * Cpad);
  upload_nchw(h, T, C, H, W, Cpad, d);
  return d;
}
void down_nchw(Ctx& c, const f16* d, float* h, int T, int C, int H, int W) {
  std::vector<f16> v((size_t)T * H * W * C);
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(v.data(), d, v.size() * 2, hipMemcpyDeviceToHost));
  for (int t = 0; t < T; ++t)
    for (int ch = 0; ch < C; ++ch)
      for (long p = 0; p < (long)H * W; ++p) h[((size_t)t * C + ch) * H * W + p] = (float)v[((size_t)t * H * W + p) * C + ch];
}
}  // namespace

namespace ug {
// exposed from engine.hip for the op-level tests
void test_unfused_attention(Ctx& c, const f16* qkv, long ld, int B, int S, int H, int d, f16* out, long ldo);
}

extern "C" {

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
    const long px = (long)T * H * W;
    std::vector<f16> v((size_t)px * 8, (f16)0.f);
    for (long p = 0; p < px; ++p) for (int ch = 0; ch < 3; ++ch) v[p * 8 + ch] = (f16)video[p * 3 + ch];
    f16* d = c.ws.get<f16>(px * 8);
    UG_CHECK(hipMemcpy(d, v.data(), v.size() * 2, hipMemcpyHostToDevice));
    f16* l = vae_encode(c, d, T, H, W);
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

// ---------------------------------------------------------------- StableNormal (reference model/stablenormal.py:16,39)
static UNetCfg sd_cfg_from(const ug_unet_config* g) {
  UNetCfg u; u.in_ch = g->in_channels; u.out_ch = g->out_channels; u.nlev = g->num_levels;
  for (int i = 0; i < 8; ++i) { u.boc[i] = g->block_out_channels[i]; u.heads[i] = g->num_attention_heads[i]; u.has_attn[i] = g->down_has_attn[i]; }
  u.layers = g->layers_per_block; u.cross_dim = g->cross_attention_dim; u.groups = g->norm_groups;
  return u;
}
int ug_bind_stablenormal(ug_ctx* x, const ug_unet_config* gu, const ug_vae_config* gv, const ug_clip_config* gd) {
  UG_TRY(x, {
    UG_REQUIRE(gu && gv && gd, "null config");
    UG_REQUIRE(gu->num_levels >= 2 && gu->num_levels <= 8 && gv->num_levels >= 2 && gv->num_levels <= 8, "num_levels out of range");
    VAECfg v; v.in_ch = gv->in_channels; v.out_ch = gv->out_channels; v.lat = gv->latent_channels; v.nlev = gv->num_levels;
    for (int i = 0; i < 8; ++i) v.boc[i] = gv->block_out_channels[i];
    v.layers = gv->layers_per_block; v.groups = gv->norm_groups; v.scaling = gv->scaling_factor;
    CLIPCfg d; d.hidden = gd->hidden_size; d.inter = gd->intermediate_size; d.layers = gd->num_hidden_layers; d.heads = gd->num_attention_heads;
    d.image = gd->image_size; d.patch = gd->patch_size; d.proj = 0; d.eps = gd->layer_norm_eps;
    bind_sn(x->c, sd_cfg_from(gu), v, d, "sn.");
    finish_binding(x->c, "sn.");
  });
}
int ug_sn_run(ug_ctx* x, const float* images, int B, int H, int W, const float* prompt, float yoso_t, int nsteps, const float* timesteps,
              const float* ca, const float* cb, float* normals_out) {
  UG_TRY(x, sn_run(x->c, images, B, H, W, prompt, yoso_t, nsteps, timesteps, ca, cb, normals_out));
}
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
    const long px = (long)B * H * W;
    std::vector<f16> v((size_t)px * 8, (f16)0.f);
    for (long p = 0; p < px; ++p) for (int ch = 0; ch < 3; ++ch) v[p * 8 + ch] = (f16)video[p * 3 + ch];
    f16* d = c.ws.get<f16>(px * 8);
    UG_CHECK(hipMemcpy(d, v.data(), v.size() * 2, hipMemcpyHostToDevice));
    f16* l = vae_encode_v(c, c.sn.vae, d, B, H, W, false);
    down_nchw(c, l, lat_out, B, c.sn.vae.cfg.lat, H / 8, W / 8);
  });
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
static void depth_metrics_out(const double* m, double s_, double t_, double* out) {
  const double cnt = m[0];
  if (cnt > 0) {
    out[0] = m[1] / cnt; out[1] = m[2] / cnt; out[2] = sqrt(m[3] / cnt); out[3] = sqrt(m[4] / cnt);
    for (int k = 0; k < 4; ++k) out[4 + k] = m[5 + k] / cnt;
  } else { for (int k = 0; k < 8; ++k) out[k] = 0; }
  out[8] = cnt; out[9] = s_; out[10] = t_;
}
struct DepthEvalBufs { const float* dp; float* dg; unsigned char* dm; };
static DepthEvalBufs depth_eval_upload(Ctx& c, const float* pred, const float* gt, const unsigned char* cmask, long n) {
  DepthEvalBufs b{nullptr, nullptr, nullptr};
  if (pred) { float* d = c.ws.get<float>(n); UG_CHECK(hipMemcpy(d, pred, n * 4, hipMemcpyHostToDevice)); b.dp = d; }
  else { UG_REQUIRE(c.io_ready && n == (long)c.T * c.H * c.W, "no resident depth of that size"); b.dp = c.d_depth; }
  b.dg = c.ws.get<float>(n); UG_CHECK(hipMemcpy(b.dg, gt, n * 4, hipMemcpyHostToDevice));
  if (cmask) { b.dm = (unsigned char*)c.ws.alloc(n); UG_CHECK(hipMemcpy(b.dm, cmask, n, hipMemcpyHostToDevice)); }
  return b;
}
static void eval_depth_lstsq(Ctx& c, const float* pred, const float* gt, const unsigned char* cmask, long n, float max_depth, double* out) {
  const DepthEvalBufs d = depth_eval_upload(c, pred, gt, cmask, n);
  double* part = c.ws.get<double>(1024 * 9);
  std::vector<double> h(1024 * 9);
  int nb = 0;
  launch_depth_fit(d.dp, d.dg, n, max_depth, part, &nb, c.stream);
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(h.data(), part, (size_t)nb * 5 * 8, hipMemcpyDeviceToHost));
  double a[5] = {0, 0, 0, 0, 0};
  for (int b = 0; b < nb; ++b) for (int k = 0; k < 5; ++k) a[k] += h[b * 5 + k];
  double s_, t_;
  lstsq_solve(a, s_, t_);
  launch_depth_metrics(d.dp, d.dg, d.dm, n, max_depth, (float)s_, (float)t_, part, &nb, c.stream);
  UG_CHECK(hipStreamSynchronize(c.stream));
  UG_CHECK(hipMemcpy(h.data(), part, (size_t)nb * 9 * 8, hipMemcpyDeviceToHost));
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < nb; ++b) for (int k = 0; k < 9; ++k) m[k] += h[b * 9 + k];
  depth_metrics_out(m, s_, t_, out);
}

int ug_eval_depth(ug_ctx* x, const float* pred, const float* gt, const unsigned char* cmask, long n, float max_depth, double* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    eval_depth_lstsq(c, pred, gt, cmask, n, max_depth, out);
  });
}

void ug_depth_eval_opts_default(ug_depth_eval_opts* o) {
  o->alignment = UG_ALIGN_LSTSQ; o->max_depth = 80.f;
  o->pre_clip_min = o->pre_clip_max = o->post_clip_min = o->post_clip_max = NAN;
}
static inline float clip_lo(float v) { return std::isnan(v) ? -INFINITY : v; }
static inline float clip_hi(float v) { return std::isnan(v) ? INFINITY : v; }
static inline float depth_bound(float v) { return (std::isnan(v) || v <= 0.f) ? NAN : v; }   // NaN: the kernels test gt > 0 only

int ug_eval_depth_ex(ug_ctx* x, const float* pred, const float* gt, const unsigned char* cmask, long n, const ug_depth_eval_opts* o,
                     double* out, float* emap_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(o != nullptr, "options must not be NULL");
    UG_REQUIRE(o->alignment >= UG_ALIGN_LSTSQ && o->alignment <= UG_ALIGN_METRIC, "unknown depth alignment (UG_ALIGN_LSTSQ / MEDIAN / SCALE / METRIC)");
    UG_REQUIRE(n >= 0 && n < (1L << 32), "pixel count");
    const bool clips = !std::isnan(o->pre_clip_min) || !std::isnan(o->pre_clip_max) || !std::isnan(o->post_clip_min) || !std::isnan(o->post_clip_max);
    if (o->alignment == UG_ALIGN_LSTSQ && !clips && !emap_out && o->max_depth > 0.f) {   // what ug_eval_depth computes: its launches, its bits
      eval_depth_lstsq(c, pred, gt, cmask, n, o->max_depth, out);
      return 0;
    }
    const float md = depth_bound(o->max_depth);
    const float lo = clip_lo(o->pre_clip_min), hi = clip_hi(o->pre_clip_max), plo = clip_lo(o->post_clip_min), phi = clip_hi(o->post_clip_max);
    const DepthEvalBufs d = depth_eval_upload(c, pred, gt, cmask, n);
    double* part = c.ws.get<double>(1024 * 9);
    std::vector<double> h(1024 * 9);
    int nb = 0;
    double s_ = 0.0, t_ = 0.0;
    if (o->alignment == UG_ALIGN_LSTSQ) {
      launch_depth_fit_ex(d.dp, d.dg, n, md, lo, hi, part, &nb, c.stream);
      UG_CHECK(hipStreamSynchronize(c.stream));
      UG_CHECK(hipMemcpy(h.data(), part, (size_t)nb * 5 * 8, hipMemcpyDeviceToHost));
      double a[5] = {0, 0, 0, 0, 0};
      for (int b = 0; b < nb; ++b) for (int k = 0; k < 5; ++k) a[k] += h[b * 5 + k];
      lstsq_solve(a, s_, t_);
    } else if (o->alignment == UG_ALIGN_MEDIAN) {
      unsigned* sel = (unsigned*)c.ws.alloc(SEL_WORDS * 4);
      launch_masked_median(d.dp, d.dg, n, md, lo, hi, sel, c.stream);
      UG_CHECK(hipStreamSynchronize(c.stream));
      unsigned r[3];
      UG_CHECK(hipMemcpy(r, sel + SEL_COUNT, sizeof(r), hipMemcpyDeviceToHost));
      float mp, mg; memcpy(&mp, &r[1], 4); memcpy(&mg, &r[2], 4);
      if (r[0] > 0) { const float sf = mg / mp; s_ = sf; }
    } else if (o->alignment == UG_ALIGN_SCALE) {
      double* wz = c.ws.get<double>(2);
      launch_weiszfeld_scale(d.dp, d.dg, n, md, lo, hi, 10, wz, part, c.stream);
      UG_CHECK(hipStreamSynchronize(c.stream));
      double r[2];
      UG_CHECK(hipMemcpy(r, wz, sizeof(r), hipMemcpyDeviceToHost));
      if (r[1] >= 1) s_ = r[0] < 1e-3 ? 1e-3 : r[0];
    } else s_ = 1.0;
    float* dmap = emap_out ? c.ws.get<float>(n) : nullptr;
    launch_depth_metrics_ex(d.dp, d.dg, d.dm, n, md, lo, hi, plo, phi, (float)s_, (float)t_, part, dmap, &nb, c.stream);
    UG_CHECK(hipStreamSynchronize(c.stream));
    UG_CHECK(hipMemcpy(h.data(), part, (size_t)nb * 9 * 8, hipMemcpyDeviceToHost));
    if (emap_out) UG_CHECK(hipMemcpy(emap_out, dmap, n * 4, hipMemcpyDeviceToHost));
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nb; ++b) for (int k = 0; k < 9; ++k) m[k] += h[b * 9 + k];
    depth_metrics_out(m, s_, t_, out);
  });
}

int ug_op_masked_median(ug_ctx* x, const float* pred, const float* gt, long n, float max_depth, float pre_clip_min, float pre_clip_max,
                        float* out_medians, long* out_count) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(n >= 1 && n < (1L << 32), "pixel count");
    const DepthEvalBufs d = depth_eval_upload(c, pred, gt, nullptr, n);
    unsigned* sel = (unsigned*)c.ws.alloc(SEL_WORDS * 4);
    launch_masked_median(d.dp, d.dg, n, depth_bound(max_depth), clip_lo(pre_clip_min), clip_hi(pre_clip_max), sel, c.stream);
    UG_CHECK(hipStreamSynchronize(c.stream));
    unsigned r[3];
    UG_CHECK(hipMemcpy(r, sel + SEL_COUNT, sizeof(r), hipMemcpyDeviceToHost));
    *out_count = (long)r[0];
    memcpy(out_medians, &r[1], 8);
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
    double* part = c.ws.get<double>(1024 * 8);
    unsigned* hist = (unsigned*)c.ws.alloc(4097 * 4);
    UG_CHECK(hipMemsetAsync(hist, 0, 4097 * 4, c.stream));
    int nb = 0;
    launch_normal_err(dp, dg, dm, n, err, part, hist, &nb, c.stream);
    UG_CHECK(hipStreamSynchronize(c.stream));
    std::vector<double> h((size_t)nb * 8);
    std::vector<unsigned> hh(4096);
    UG_CHECK(hipMemcpy(h.data(), part, (size_t)nb * 8 * 8, hipMemcpyDeviceToHost));
    UG_CHECK(hipMemcpy(hh.data(), hist, 4096 * 4, hipMemcpyDeviceToHost));
    double m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nb; ++b) for (int k = 0; k < 8; ++k) m[k] += h[b * 8 + k];
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

int ug_op_linear(ug_ctx* x, const float* A, int M, int K, const float* W, int N, const float* bias, const float* R1,
                 float c0, float c1, int act, int geglu, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    std::vector<float> Wp, bp;
    const float* Wu = W; const float* bu = bias;
    if (geglu) {   // same row interleave as bind_geglu
      const int inner = N / 2;
      Wp.resize((size_t)N * K); if (bias) bp.resize(N);
      for (int v = 0; v < N; ++v) {
        const int blk = v / 16, wv = v % 16;
        const int src = wv < 8 ? blk * 8 + wv : inner + blk * 8 + (wv - 8);
        memcpy(&Wp[(size_t)v * K], &W[(size_t)src * K], (size_t)K * 4);
        if (bias) bp[v] = bias[src];
      }
      Wu = Wp.data(); if (bias) bu = bp.data();
    }
    const int Nout = geglu ? N / 2 : N;
    f16* dA = up16(c, A, (long)M * K); f16* dW = up16(c, Wu, (long)N * K);
    f16* db = up16_opt(c, bu, N); f16* dR = up16_opt(c, R1, (long)M * Nout);
    f16* dO = c.ws.get<f16>((long)M * Nout);
    GemmP p; memset(&p, 0, sizeof(p));
    p.A0 = dA; p.C0 = K; p.M = M; p.N = N; p.K = K; p.W = dW; p.ldw = K; p.bias = db; p.R1 = dR; p.ldr1 = Nout;
    p.c0 = c0; p.c1 = c1; p.act = act; p.flags = geglu ? UG_F_GEGLU : 0; p.Out = dO; p.ldo = Nout; p.zero = c.zero; p.nb_inner = 1;
    gemm_apply_tune(p, c.tune);
    { int cf, sp; gemm_plan(p, 1, &cf, &sp); p.cfg_p1 = cf + 1; p.splitk = sp; if (sp > 1) p.partial = c.ws.get<float>((long)sp * M * N); }
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
    std::vector<float> w1((size_t)2 * I * C), bb1((size_t)2 * I);
    for (int v = 0; v < 2 * I; ++v) {
      const int blk = v / 16, wv = v % 16, src = wv < 8 ? blk * 8 + wv : I + blk * 8 + (wv - 8);
      memcpy(&w1[(size_t)v * C], &W1[(size_t)src * C], sizeof(float) * C);
      bb1[v] = b1[src];
    }
    const int nvec = addvec ? (M + rows_per_vec - 1) / rows_per_vec : 0;
    f16* dX = up16(c, X, (long)M * C); f16* dW1 = up16(c, w1.data(), (long)2 * I * C); f16* db1 = up16(c, bb1.data(), 2 * I);
    f16* dW2 = up16(c, W2, (long)C * I); f16* db2 = up16(c, b2, C);
    f16* dg = up16(c, gamma, C); f16* dbt = up16(c, beta, C); f16* dav = addvec ? up16(c, addvec, (long)nvec * C) : nullptr;
    f16* dO = c.ws.get<f16>((long)M * C);
    FFusedP p; memset(&p, 0, sizeof(p));
    p.W1 = dW1; p.b1 = db1; p.W2 = dW2; p.b2 = db2; p.c0 = c0; p.c1 = c1; p.Out = dO; p.M = M; p.C = C; p.zero = c.zero; p.variant = c.ff_variant;
    if (mode == 2) {
      p.X = dX; p.R1 = dX; p.ln_g = dg; p.ln_b = dbt; p.ln_eps = eps; p.addvec = dav; p.rows_per_vec = rows_per_vec;
      launch_ff_fused(p, c.stream);
    } else {
      f16* t1 = c.ws.get<f16>((long)M * C); f16* xo = c.ws.get<f16>((long)M * C);
      LayerNormP l; memset(&l, 0, sizeof(l));
      l.X = dX; l.Y = t1; l.M = M; l.C = C; l.eps = eps; l.gamma = dg; l.beta = dbt; l.addvec = dav; l.rows_per_vec = rows_per_vec; l.Xout = dav ? xo : nullptr;
      launch_layernorm(l, c.stream);
      const f16* res = dav ? xo : dX;
      if (mode == 1) {
        p.X = t1; p.R1 = res;
        launch_ff_fused(p, c.stream);
      } else {
        f16* mid = c.ws.get<f16>((long)M * I);
        GemmP g1; memset(&g1, 0, sizeof(g1));
        g1.A0 = t1; g1.C0 = C; g1.M = M; g1.N = 2 * I; g1.K = C; g1.W = dW1; g1.ldw = C; g1.bias = db1; g1.c0 = 1.f; g1.Out = mid; g1.ldo = I;
        g1.flags = UG_F_GEGLU; g1.zero = c.zero; g1.nb_inner = 1;
        gemm_apply_tune(g1, c.tune); launch_gemm(g1, 1, c.stream);
        GemmP g2; memset(&g2, 0, sizeof(g2));
        g2.A0 = mid; g2.C0 = I; g2.M = M; g2.N = C; g2.K = I; g2.W = dW2; g2.ldw = I; g2.bias = db2; g2.c0 = c0; g2.R1 = res; g2.ldr1 = C; g2.c1 = c1;
        g2.Out = dO; g2.ldo = C; g2.zero = c.zero; g2.nb_inner = 1; g2.splitk = 1;
        gemm_apply_tune(g2, c.tune); launch_gemm(g2, 1, c.stream);
      }
    }
    down16(c, dO, out, (long)M * C);
  });
}

int ug_op_ff(ug_ctx* x, const float* X, int M, int C, const float* W1, const float* b1, const float* W2, const float* b2, const float* R1,
             float c0, float c1, int fused, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int I = 4 * C;
    // W1 / b1 in the engine's GEGLU row order: blocks of 16 rows = [8 value | 8 gate]
    std::vector<float> w1((size_t)2 * I * C), bb1((size_t)2 * I);
    for (int v = 0; v < 2 * I; ++v) {
      const int blk = v / 16, wv = v % 16, src = wv < 8 ? blk * 8 + wv : I + blk * 8 + (wv - 8);
      memcpy(&w1[(size_t)v * C], &W1[(size_t)src * C], sizeof(float) * C);
      bb1[v] = b1[src];
    }
    f16* dX = up16(c, X, (long)M * C); f16* dW1 = up16(c, w1.data(), (long)2 * I * C); f16* db1 = up16(c, bb1.data(), 2 * I);
    f16* dW2 = up16(c, W2, (long)C * I); f16* db2 = up16(c, b2, C); f16* dR = up16_opt(c, R1, (long)M * C);
    f16* dO = c.ws.get<f16>((long)M * C);
    if (fused) {
      FFusedP p; memset(&p, 0, sizeof(p));
      p.X = dX; p.W1 = dW1; p.b1 = db1; p.W2 = dW2; p.b2 = db2; p.R1 = dR; p.c0 = c0; p.c1 = c1; p.Out = dO; p.M = M; p.C = C; p.zero = c.zero; p.variant = c.ff_variant;
      launch_ff_fused(p, c.stream);
    } else {
      f16* mid = c.ws.get<f16>((long)M * I);
      GemmP g1; memset(&g1, 0, sizeof(g1));
      g1.A0 = dX; g1.C0 = C; g1.M = M; g1.N = 2 * I; g1.K = C; g1.W = dW1; g1.ldw = C; g1.bias = db1; g1.c0 = 1.f; g1.Out = mid; g1.ldo = I;
      g1.flags = UG_F_GEGLU; g1.zero = c.zero; g1.nb_inner = 1;
      gemm_apply_tune(g1, c.tune); launch_gemm(g1, 1, c.stream);
      GemmP g2; memset(&g2, 0, sizeof(g2));
      g2.A0 = mid; g2.C0 = I; g2.M = M; g2.N = C; g2.K = I; g2.W = dW2; g2.ldw = I; g2.bias = db2; g2.c0 = c0; g2.R1 = dR; g2.ldr1 = C; g2.c1 = c1;
      g2.Out = dO; g2.ldo = C; g2.zero = c.zero; g2.nb_inner = 1; g2.splitk = 1;
      gemm_apply_tune(g2, c.tune); launch_gemm(g2, 1, c.stream);
    }
    down16(c, dO, out, (long)M * C);
  });
}
int ug_bench_flash(ug_ctx* x, int B, int H, int S, int variant, int iters, float* us_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const long M = (long)B * S; const int C = H * 64;
    f16* qkv = c.ws.get<f16>(M * 3 * C); f16* o = c.ws.get<f16>(M * C);
    launch_fill_random(qkv, M * 3 * C, 7, c.stream);
    FlashP p; p.Q = qkv; p.K = qkv + C; p.V = qkv + 2 * C; p.ldq = p.ldk = p.ldv = 3 * C; p.O = o; p.ldo = C; p.B = B; p.H = H; p.S = S; p.scale = 0.125f;
    p.variant = variant;     // passed with the launch: the process default (and every other launch) is untouched
    launch_flash_attn64(p, c.stream); launch_flash_attn64(p, c.stream);
    hipEvent_t e0, e1; UG_CHECK(hipEventCreate(&e0)); UG_CHECK(hipEventCreate(&e1));
    UG_CHECK(hipEventRecord(e0, c.stream));
    for (int i = 0; i < iters; ++i) launch_flash_attn64(p, c.stream);
    UG_CHECK(hipEventRecord(e1, c.stream));
    UG_CHECK(hipEventSynchronize(e1));
    float ms = 0.f; UG_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *us_out = ms * 1000.f / iters;
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
    auto run = [&]() {
      if (fused) {
        FFusedP p; memset(&p, 0, sizeof(p)); p.variant = c.ff_variant;
        p.X = dX; p.W1 = dW1; p.b1 = db1; p.W2 = dW2; p.b2 = db2; p.R1 = dR; p.c0 = 1.f; p.c1 = 1.f; p.Out = dO; p.M = M; p.C = C; p.zero = c.zero;
        launch_ff_fused(p, c.stream);
      } else {
        GemmP g1; memset(&g1, 0, sizeof(g1));
        g1.A0 = dX; g1.C0 = C; g1.M = M; g1.N = 2 * I; g1.K = C; g1.W = dW1; g1.ldw = C; g1.bias = db1; g1.c0 = 1.f; g1.Out = mid; g1.ldo = I;
        g1.flags = UG_F_GEGLU; g1.zero = c.zero; g1.nb_inner = 1;
        gemm_apply_tune(g1, c.tune); launch_gemm(g1, 1, c.stream);
        GemmP g2; memset(&g2, 0, sizeof(g2));
        g2.A0 = mid; g2.C0 = I; g2.M = M; g2.N = C; g2.K = I; g2.W = dW2; g2.ldw = I; g2.bias = db2; g2.c0 = 1.f; g2.R1 = dR; g2.ldr1 = C; g2.c1 = 1.f;
        g2.Out = dO; g2.ldo = C; g2.zero = c.zero; g2.nb_inner = 1; g2.splitk = 1;
        gemm_apply_tune(g2, c.tune); launch_gemm(g2, 1, c.stream);
      }
    };
    run(); run();
    hipEvent_t e0, e1; UG_CHECK(hipEventCreate(&e0)); UG_CHECK(hipEventCreate(&e1));
    UG_CHECK(hipEventRecord(e0, c.stream));
    for (int i = 0; i < iters; ++i) run();
    UG_CHECK(hipEventRecord(e1, c.stream));
    UG_CHECK(hipEventSynchronize(e1));
    float ms = 0.f; UG_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *us_out = ms * 1000.f / iters;
  });
}
int ug_op_linear_mx8(ug_ctx* x, const float* A, int M, int K, const float* W, int N, const float* bias, int geglu, float* out,
                     unsigned char* a8_out, unsigned* sa_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    UG_REQUIRE(K % 128 == 0 && N % 8 == 0, "op_linear_mx8: K % 128 == 0, N % 8 == 0");
    f16* dA = up16(c, A, (long)M * K); f16* dW = up16(c, W, (long)N * K);
    f16* db = up16_opt(c, bias, N);
    const long ld_sa = (M + 255) / 256 * 256, ld_sw = (N + 255) / 256 * 256;
    unsigned char* a8 = (unsigned char*)c.ws.alloc((size_t)M * K); unsigned char* w8 = (unsigned char*)c.ws.alloc((size_t)N * K);
    unsigned* sa = (unsigned*)c.ws.alloc((size_t)(K / 128) * ld_sa * 4); unsigned* sw = (unsigned*)c.ws.alloc((size_t)(K / 128) * ld_sw * 4);
    UG_CHECK(hipMemsetAsync(sa, 0, (size_t)(K / 128) * ld_sa * 4, c.stream)); UG_CHECK(hipMemsetAsync(sw, 0, (size_t)(K / 128) * ld_sw * 4, c.stream));
    f16* dW2 = dW;
    if (geglu) {   // the engine's GEGLU row order: blocks of 16 rows = [8 value | 8 gate]
      std::vector<f16> hw((size_t)N * K), hb(N);
      const int inner = N / 2;
      for (int v = 0; v < N; ++v) {
        const int blk = v / 16, wv = v % 16, srcr = wv < 8 ? blk * 8 + wv : inner + blk * 8 + (wv - 8);
        for (int k = 0; k < K; ++k) hw[(size_t)v * K + k] = (f16)W[(size_t)srcr * K + k];
        hb[v] = bias ? (f16)bias[srcr] : (f16)0.f;
      }
      dW2 = c.ws.get<f16>((long)N * K);
      UG_CHECK(hipMemcpy(dW2, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
      if (bias) UG_CHECK(hipMemcpy(db, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
    }
    launch_quant_mx8(dA, K, M, K, a8, sa, ld_sa, c.stream);
    launch_quant_mx8(dW2, K, N, K, w8, sw, ld_sw, c.stream);
    const int nout = geglu ? N / 2 : N;
    f16* dO = c.ws.get<f16>((long)M * nout);
    GemmP p; memset(&p, 0, sizeof(p));
    p.A0 = (const f16*)a8; p.C0 = K; p.M = M; p.N = N; p.K = K; p.W = (const f16*)w8; p.ldw = K; p.bias = db; p.c0 = 1.f;
    p.Out = dO; p.ldo = nout; p.flags = geglu ? UG_F_GEGLU : 0; p.zero = c.zero; p.nb_inner = 1;
    p.sa = sa; p.ld_sa = ld_sa; p.sw = sw; p.ld_sw = ld_sw;
    gemm_apply_tune(p, c.tune);
    launch_gemm_mx8(p, c.stream);
    down16(c, dO, out, (long)M * nout);
    if (a8_out) UG_CHECK(hipMemcpy(a8_out, a8, (size_t)M * K, hipMemcpyDeviceToHost));
    if (sa_out) UG_CHECK(hipMemcpy(sa_out, sa, (size_t)(K / 128) * ld_sa * 4, hipMemcpyDeviceToHost));
  });
}

int ug_op_conv(ug_ctx* x, const float* x0, int C0, const float* x1, int C1, int T, int H, int W, const float* weight,
               const float* bias, int O, int kt, int k, int stride, int pad_t, int pad_l, int ups, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int I = C0 + C1, taps = kt * k * k;
    std::vector<float> wp((size_t)O * taps * I);
    const bool kch = (I % 64 == 0) && taps > 1 && !getenv("UG_NO_KCHUNK");     // the engine's chunk-major K order (GemmP::kchunk); UG_NO_KCHUNK: tap-major weights -> general path
    for (int o = 0; o < O; ++o) for (int i = 0; i < I; ++i) for (int tp = 0; tp < taps; ++tp)
      wp[kch ? (((size_t)o * (I / 64) + i / 64) * taps + tp) * 64 + i % 64 : ((size_t)o * taps + tp) * I + i] = weight[((size_t)o * I + i) * taps + tp];
    const long px = (long)T * H * W;
    f16* d0 = up16(c, x0, px * C0); f16* d1 = C1 ? up16(c, x1, px * C1) : nullptr;
    f16* dW = up16(c, wp.data(), (long)wp.size()); f16* db = up16_opt(c, bias, O);
    const int Ho = H * ups / stride, Wo = W * ups / stride;
    f16* dO = c.ws.get<f16>((long)T * Ho * Wo * O);
    GemmP p; memset(&p, 0, sizeof(p));
    p.conv = 1; p.A0 = d0; p.A1 = d1; p.C0 = C0; p.C1 = C1; p.T = T; p.Hi = H; p.Wi = W; p.Ho = Ho; p.Wo = Wo;
    p.ups = ups; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l; p.kt = kt; p.ky = k; p.kx = k;
    p.M = T * Ho * Wo; p.N = O; p.K = I * taps; p.W = dW; p.ldw = p.K; p.bias = db; p.c0 = 1.f;
    p.Out = dO; p.ldo = O; p.zero = c.zero; p.nb_inner = 1; p.kchunk = kch;
    gemm_apply_tune(p, c.tune);
    { int cf, sp; gemm_plan(p, 1, &cf, &sp); p.cfg_p1 = cf + 1; p.splitk = sp; if (sp > 1) p.partial = c.ws.get<float>((long)sp * p.M * p.N); }
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
    std::vector<float> wp((size_t)O * taps * I);
    for (int o = 0; o < O; ++o) for (int i = 0; i < I; ++i) for (int tp = 0; tp < taps; ++tp)
      wp[(((size_t)o * (I / 64) + i / 64) * taps + tp) * 64 + i % 64] = weight[((size_t)o * I + i) * taps + tp];
    const long M = (long)T * H * W;
    f16* d0 = up16(c, x0, M * C0); f16* dW = up16(c, wp.data(), (long)wp.size()); f16* db = up16_opt(c, bias, O);
    f16* dR = up16_opt(c, res, M * O);
    f16* dg = up16(c, gamma, O); f16* dbt = up16(c, beta, O);
    f16* o1 = c.ws.get<f16>(M * O); f16* o2 = c.ws.get<f16>(M * O); f16* y1 = c.ws.get<f16>(M * O); f16* y2 = c.ws.get<f16>(M * O);
    float2* part = (float2*)c.ws.get<float>(((M + 47) / 48) * (long)O * 2);
    int rb = 0;
    for (int pass = 0; pass < 2; ++pass) {
      GemmP p; memset(&p, 0, sizeof(p));
      p.conv = 1; p.A0 = d0; p.C0 = C0; p.T = T; p.Hi = H; p.Wi = W; p.Ho = H; p.Wo = W;
      p.ups = 1; p.stride = 1; p.pad_t = k / 2; p.pad_l = k / 2; p.kt = kt; p.ky = k; p.kx = k;
      p.M = (int)M; p.N = O; p.K = I * taps; p.W = dW; p.ldw = p.K; p.bias = db; p.c0 = 1.f; p.R1 = dR; p.ldr1 = O; p.c1 = 1.f;
      p.Out = pass ? o2 : o1; p.ldo = O; p.zero = c.zero; p.nb_inner = 1; p.kchunk = taps > 1;
      gemm_apply_tune(p, c.tune);
      const size_t mk = c.ws.mark();
      { int cf, sp; gemm_plan(p, 1, &cf, &sp); p.cfg_p1 = cf + 1; p.splitk = sp; if (sp > 1) p.partial = c.ws.get<float>((long)sp * p.M * p.N); }
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

int ug_op_groupnorm(ug_ctx* x, const float* x0, int C0, const float* x1, int C1, int T, int HW, int G, float eps,
                    int temporal, int silu, const float* gamma, const float* beta, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int C = C0 + C1; const long M = (long)T * HW;
    GroupNormP p; memset(&p, 0, sizeof(p));
    p.X0 = up16(c, x0, M * C0); p.X1 = C1 ? up16(c, x1, M * C1) : nullptr; p.C0 = C0; p.C1 = C1;
    p.T = T; p.HW = HW; p.G = G; p.eps = eps; p.temporal = temporal; p.silu = silu;
    p.gamma = up16(c, gamma, C); p.beta = up16(c, beta, C);
    f16* y = c.ws.get<f16>(M * C); p.Y = y;
    p.ws = c.ws.get<float>((long)groupnorm_ws_floats(T, HW, C, G));
    launch_groupnorm(p, c.stream);
    down16(c, y, out, M * C);
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
    for (int i = 0; i < 3; ++i) launch_groupnorm(p, c.stream);
    hipEvent_t e0, e1; UG_CHECK(hipEventCreate(&e0)); UG_CHECK(hipEventCreate(&e1));
    UG_CHECK(hipEventRecord(e0, c.stream));
    for (int i = 0; i < iters; ++i) launch_groupnorm(p, c.stream);
    UG_CHECK(hipEventRecord(e1, c.stream)); UG_CHECK(hipEventSynchronize(e1));
    float ms; UG_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    us_out[0] = ms * 1000.f / iters;
  });
}

int ug_op_layernorm(ug_ctx* x, const float* xin, int M, int C, float eps, const float* gamma, const float* beta,
                    const float* addvec, int rows_per_vec, float* out, float* xout) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    LayerNormP p; memset(&p, 0, sizeof(p));
    p.X = up16(c, xin, (long)M * C); p.M = M; p.C = C; p.eps = eps; p.gamma = up16(c, gamma, C); p.beta = up16(c, beta, C);
    f16* y = c.ws.get<f16>((long)M * C); p.Y = y;
    f16* xo = nullptr;
    if (addvec) {
      const int nv = (M + rows_per_vec - 1) / rows_per_vec;
      p.addvec = up16(c, addvec, (long)nv * C); p.rows_per_vec = rows_per_vec;
      xo = c.ws.get<f16>((long)M * C); p.Xout = xo;
    }
    launch_layernorm(p, c.stream);
    down16(c, y, out, (long)M * C);
    if (xo && xout) down16(c, xo, xout, (long)M * C);
  });
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

int ug_op_attention_generic(ug_ctx* x, const float* qkv, int B, int S, int H, int d, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int C = H * d; const long M = (long)B * S;
    f16* dq = up16(c, qkv, M * 3 * C); f16* o = c.ws.get<f16>(M * C);
    test_unfused_attention(c, dq, 3 * C, B, S, H, d, o, C);
    down16(c, o, out, M * C);
  });
}

int ug_op_flash_attn_dh(ug_ctx* x, const float* qkv, int B, int S, int H, int d, float* out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    const int C = H * d; const long M = (long)B * S;
    f16* dq = up16(c, qkv, M * 3 * C); f16* o = c.ws.get<f16>(M * C);
    FlashP p; p.variant = c.flash_variant; p.Q = dq; p.K = dq + C; p.V = dq + 2 * C; p.ldq = p.ldk = p.ldv = 3 * C; p.O = o; p.ldo = C; p.B = B; p.H = H; p.S = S;
    p.scale = 1.0f / sqrtf((float)d);
    launch_flash_attn_dh(p, d, c.stream);
    down16(c, o, out, M * C);
  });
}

int ug_bench_mfma_peak(ug_ctx* x, int iters, float* tflops_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    float* scratch = c.ws.get<float>(256 * 512);
    *tflops_out = bench_mfma_peak(scratch, iters > 0 ? iters : 20000, c.stream);
  });
}
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

// GEMM / conv microbenchmark on device-resident pseudo-random data: average ms per launch over `iters`.
int ug_bench_gemm(ug_ctx* x, int M, int N, int K, int conv, int T, int Hi, int Wi, int C0, int C1, int kt, int k,
                  int stride, int ups, int cfg, int split, int iters, float* ms_out) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    GemmP p; memset(&p, 0, sizeof(p));
    long asz;
    if (conv) {
      p.conv = 1; p.T = T; p.Hi = Hi; p.Wi = Wi; p.ups = ups; p.stride = stride; p.kt = kt; p.ky = k; p.kx = k;
      p.pad_t = k / 2; p.pad_l = k / 2; p.Ho = Hi * ups / stride; p.Wo = Wi * ups / stride;
      p.C0 = C0; p.C1 = C1; M = T * p.Ho * p.Wo; K = (C0 + C1) * kt * k * k;
      asz = (long)T * Hi * Wi * C0;
    } else { p.C0 = K; asz = (long)M * K; }
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
    p.M = M; p.N = N; p.K = K; p.W = Wt; p.ldw = K; p.bias = b; p.c0 = 1.f; p.ldo = N;
    p.zero = c.zero; p.nb_inner = 1;
    p.kchunk = (conv && kt * k * k > 1 && (C0 + C1) % 64 == 0 && !getenv("UG_NO_KCHUNK")) ? 1 : 0;   // the engine's chunk-major K order (random weights: the layout itself is immaterial)
    p.A0 = As[0]; p.A1 = A1s[0]; p.Out = Os[0];
    if (getenv("UG_BENCH_GEGLU") && !conv && N % 128 == 0) { p.flags |= UG_F_GEGLU; p.ldo = N / 2; }   // A/B aid: GEGLU epilogue
    if (getenv("UG_BENCH_R1")) { p.R1 = Os[nbuf - 1]; p.ldr1 = N; p.c1 = 1.f; }                          // A/B aid: a residual operand in the epilogue
    if (getenv("UG_BENCH_NOBIAS")) p.bias = nullptr;
    gemm_apply_tune(p, c.tune);
    int cf = cfg, sp = split;
    if (cf < 0 || sp < 1) { int c2, s2; gemm_plan(p, 1, &c2, &s2); if (cf < 0) cf = c2; if (sp < 1) sp = s2; }
    p.cfg_p1 = cf + 1; p.splitk = sp;
    if (sp > 1) p.partial = c.ws.get<float>((long)sp * M * N);
    unsigned* trace = nullptr;
    if (getenv("UG_GEMM_TRACE")) { trace = c.ws.get<unsigned>(3 * 24 * 5); UG_CHECK(hipMemsetAsync(trace, 0, 3 * 24 * 5 * 4, c.stream)); p.trace = trace; }
    for (int i = 0; i < 2; ++i) launch_gemm(p, 1, c.stream);
    hipEvent_t e0, e1; UG_CHECK(hipEventCreate(&e0)); UG_CHECK(hipEventCreate(&e1));
    UG_CHECK(hipEventRecord(e0, c.stream));
    for (int i = 0; i < iters; ++i) { p.A0 = As[i % nbuf]; p.A1 = A1s[i % nbuf]; p.Out = Os[i % nbuf]; launch_gemm(p, 1, c.stream); }
    UG_CHECK(hipEventRecord(e1, c.stream)); UG_CHECK(hipEventSynchronize(e1));
    float ms; UG_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
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

int ug_op_euler_step(ug_ctx* x, const float* v, float* lat, long n, float sigma, float sigma_next) {
  UG_TRY(x, {
    Ctx& c = x->c; Scope sc(c);
    f16* dv = up16(c, v, n); f16* dl = up16(c, lat, n);
    launch_euler_step(dv, dl, n, sigma, sigma_next, c.stream);
    down16(c, dl, lat, n);
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

}  // extern "C"
