/* libunigeo_hip.so - C ABI of the MI355X-native (gfx950) DepthCrafter inference path.
 *
 * This is the drop-in boundary behind UniGeo's model/ plugin surface.  Each entry point
 * names the reference interface it replaces (paths relative to the reference checkout).
 * Plain C types only: no torch / numpy types cross this boundary.
 *
 * Conventions
 *   - every function returning int: 0 = OK, non-zero = error; the message is available from
 *     ug_last_error(ctx) (the reference raises Python exceptions instead - the ctypes shim in
 *     unigeo_amd/_lib.py turns a non-zero code back into RuntimeError).
 *   - the caller owns all host buffers; the library owns all device memory.
 *   - one context per GPU; calls on a context must be serialised by the caller; the library
 *     runs on its own HIP stream and synchronises before returning.
 *   - "video" tensors are channels-last: frames [T,H,W,3] float32 in [0,1] exactly as
 *     DepthCrafter.prepare_input produces them (model/depthcrafter.py:39-45).
 *   - noise is an INPUT (the reference draws it from the global CUDA RNG without a generator,
 *     model/depthcrafter.py:80-90): noise_latents [T,4,H/8,W/8], noise_aug [T,3,H,W], float32,
 *     laid out as torch.randn would produce them inside the pipeline (NCHW).  ug_dc_set_inputs_ex can instead generate both on the
 *     device from one 64-bit seed (the reference draws on the GPU too, unseeded).
 */
#ifndef UNIGEO_HIP_H
#define UNIGEO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ug_ctx ug_ctx;

enum { UG_DTYPE_F16 = 0, UG_DTYPE_F32 = 1 };

/* Architecture hyper-parameters.  Defaults (ug_*_config_default) are SVD-XT / DepthCrafter:
 * replaces the config.json files read by from_pretrained (model/depthcrafter.py:18-29). */
typedef struct {
  int in_channels, out_channels, num_levels;
  int block_out_channels[8];
  int num_attention_heads[8];
  int down_has_attn[8];
  int layers_per_block, cross_attention_dim, addition_time_embed_dim, projection_class_embeddings_input_dim;
  int norm_groups;
  float eps_cross_attn_blocks, eps_plain_down_block, eps_mid_block, eps_up_blocks;
} ug_unet_config;

typedef struct {
  int in_channels, out_channels, latent_channels, num_levels;
  int block_out_channels[8];
  int layers_per_block, norm_groups;
  float scaling_factor;
} ug_vae_config;

typedef struct {
  int hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, image_size, patch_size, projection_dim;
  float layer_norm_eps;
} ug_clip_config;

void ug_unet_config_default(ug_unet_config* c);
void ug_vae_config_default(ug_vae_config* c);
void ug_clip_config_default(ug_clip_config* c);

/* Context: replaces `self.device = cuda:0` + pipeline.to(device) (model/depthcrafter.py:11,31).
 * workspace_bytes: transient activation arena; persist_bytes: weights in kernel-ready layout. */
ug_ctx* ug_create(int device_id, size_t workspace_bytes, size_t persist_bytes);
void ug_destroy(ug_ctx* ctx);
const char* ug_last_error(ug_ctx* ctx);   /* ctx may be NULL: returns the creation error */
size_t ug_workspace_peak(ug_ctx* ctx);

/* Weights: replaces DiffusersUNet...from_pretrained / DepthCrafterPipeline.from_pretrained
 * (model/depthcrafter.py:18-29).  Tensors are uploaded under their diffusers / transformers
 * state-dict names with a component prefix ("unet.", "vae.", "clip."), then bound; binding
 * hard-fails on any missing, mis-shaped or unexpected tensor. */
int ug_load_tensor(ug_ctx* ctx, const char* name, int dtype, int ndim, const int64_t* shape, const void* host_data);
int ug_bind_unet(ug_ctx* ctx, const ug_unet_config* cfg);
int ug_bind_vae(ug_ctx* ctx, const ug_vae_config* cfg);
int ug_bind_clip(ug_ctx* ctx, const ug_clip_config* cfg);

/* The pipeline call: replaces `self.pipeline(frames, height, width, output_type="np",
 * guidance_scale=1.0, num_inference_steps, window_size=len(frames), overlap, ...).frames[0]`
 * (model/depthcrafter.py:80-90) plus the wrapper post-processing at :92-97 (depth) and
 * prepare_output at :48-59 (normals, OpenGL frame).
 *   ug_dc_set_inputs : host -> HBM (frames, noise, per-frame 3x3 intrinsics or NULL)
 *   ug_dc_run        : CLIP + VAE-encode + `steps` x (scale, concat, UNet, Euler) + VAE temporal
 *                      decode (chunks of decode_chunk frames) + depth (+ normals); all on device
 *   ug_dc_get_outputs: HBM -> host; any pointer may be NULL
 *                      frames_out [T,H,W,3], depth_out [T,H,W], normals_out [T,H,W,3] float32 */
int ug_dc_set_inputs(ug_ctx* ctx, const float* frames_thwc, int T, int H, int W, const float* noise_latents,
                     const float* noise_aug, const float* intrinsics_t33);
int ug_dc_run(ug_ctx* ctx, int steps, int decode_chunk, int with_normals);
/* Opt-in input modes of the same call (ug_dc_set_inputs is unchanged): replaces DepthCrafter.prepare_input (model/depthcrafter.py:39-45) and the
 * noise the pipeline draws from the global CUDA RNG (model/depthcrafter.py:80-90).
 *   frames_format UG_FRAMES_F32_THWC: frames = float32 [T,H,W,3] in [0,1], as ug_dc_set_inputs.
 *                 UG_FRAMES_U8_TCHW : frames = uint8 planar [T,3,H,W], the dataset's images stacked; converted on the device to x / 255, bit-identical
 *                                     to prepare_input (a quarter of the upload).
 *   noise_latents and noise_aug both given: host noise, as ug_dc_set_inputs.  Both NULL: the two resident noise tensors (same buffers, same layout)
 *   are generated on the context's stream from noise_seed by a counter-based generator (Philox4x32-10 + Box-Muller): element
 *   e of a tensor depends on (noise_seed, tensor, e) only - not on the context, the rank, the launch geometry or what ran before; |z| <= 5.768.
 *   One of the two NULL is an error.  Same checks as ug_dc_set_inputs; ug_dc_run / ug_dc_run_windows / guidance read the same buffers.
 * ug_dc_get_noise: HBM -> host, the resident noise of the current inputs however it got there (noise_latents_out [T,4,H/8,W/8], noise_aug_out
 *   [T,3,H,W], float32; either may be NULL) - what to pass to ug_dc_set_inputs to repeat a seeded clip bit for bit. */
enum { UG_FRAMES_F32_THWC = 0, UG_FRAMES_U8_TCHW = 1 };
int ug_dc_set_inputs_ex(ug_ctx* ctx, const void* frames, int frames_format, int T, int H, int W, const float* noise_latents,
                        const float* noise_aug, uint64_t noise_seed, const float* intrinsics_t33);
int ug_dc_get_noise(ug_ctx* ctx, float* noise_latents_out, float* noise_aug_out);
/* Long-video mode of the pipeline call (`window_size` / `overlap` of model/depthcrafter.py:87-88, which the reference pins to
 * len(frames) / 25, i.e. OFF): latent sliding windows of `window` (<= 128) frames with `overlap` re-noised + cross-faded frames,
 * restated from upstream DepthCrafter's published pipeline (UNPINNED).  window == 0 or >= T is ug_dc_run.  The first `window`
 * frames of the noise passed to ug_dc_set_inputs are the window noise (rotated by `overlap` frames per window, as upstream). */
int ug_dc_run_windows(ug_ctx* ctx, int steps, int decode_chunk, int with_normals, int window, int overlap);
int ug_dc_get_outputs(ug_ctx* ctx, float* frames_out, float* depth_out, float* normals_out);
/* Classifier-free guidance: `guidance_scale` of the pipeline call (model/depthcrafter.py:80-90, where the reference passes 1.0).  Per-context
 * state for ug_dc_run and ug_dc_run_windows, default 1.0.  <= 1: no guidance (the reference path).  > 1: every Euler step evaluates the UNet on
 * the conditional input and on an unconditional one (zero image embeddings, zero conditioning latents) and steps on v_u + g (v_c - v_u),
 * restated from upstream DepthCrafter's published pipeline (UNPINNED); both evaluations run as one UNet pass over the two stacked videos.
 * A value that is not finite is rejected. */
int ug_dc_set_guidance(ug_ctx* ctx, float guidance_scale);
/* Arithmetic of the VAE *encoder*.  The reference pipeline up-casts the VAE to float32 around encode (diffusers force_upcast;
 * pipeline built at model/depthcrafter.py:24-29) and runs everything else in fp16.  on = 1 (default): float32-grade encoder -
 * fp32 residual stream / GroupNorm / softmax, GEMMs on fp16 hi/lo activation pairs against the (fp16-valued) weights, which is
 * exact to fp32 rounding.  on = 0: fp16 storage with fp32 accumulation, like the decoder (faster, ~1e-3 off the fp32 result). */
int ug_set_vae_encode_fp32(ug_ctx* ctx, int on);
/* Independent sub-graphs of one pipeline call in flight at a time (default 1 = strictly one kernel after another; 2 measured -0.6 % on the headline clip).  The reference's
 * pipeline encodes / decodes the clip in chunks of `decode_chunk_size` frames one after the other and computes the CLIP embeddings before
 * them (the calls inside pipeline(...) at model/depthcrafter.py:80-90); those chunks do not depend on each other, so the engine issues them on
 * separate HIP streams - one chunk's HBM-bound passes overlap another's MFMA-bound ones.  Same kernels, same launch parameters:
 * outputs are bit-identical for every setting. */
int ug_set_concurrency(ug_ctx* ctx, int lanes);
/* Two (or more) contexts on ONE GPU, each running its own clip (round 5): the reference's evaluation loop handles one independent clip after the other
 * (eval.py:33-56: `for data_idx ...: output = model.forward(data)`), so a second plugin instance on the same GPU can process the next clip meanwhile - its
 * kernels fill the CUs that one clip's tile tails and under-filled launches leave idle (+10 % aggregate frames/s).  on = 1 tells a context that it shares the
 * GPU: heuristics that pay extra launches / work to fill the last round of ONE kernel are dropped (the fused feed-forward takes all rows, the tile planner
 * ignores the last-round fill).  Same arithmetic per layer up to the tile choice (all tiles are bit-identical, tests/test_ops_gpu.py).  Default 0. */
int ug_set_coscheduled(ug_ctx* ctx, int on);
/* BASELINE configs[4] (north_star: "fp8 MFMA ... (CDNA4 fp8)"): on = 1 runs the UNet transformers' linear layers whose K is a multiple
 * of 128 on MX-fp8 matrix instructions (v_mfma_scale_f32_16x16x128_f8f6f4: OCP e4m3 elements, one e8m0 power-of-two scale per 32
 * K elements; activations are quantised on the fly, weights once at bind time).  Reduced precision - the reference has no fp8 path;
 * the measured error against the fp16 path and the oracle is reported by tests/test_fp8_gpu.py.  Default 0. */
int ug_set_fp8_linears(ug_ctx* ctx, int on);
/* Device addresses of the resident outputs (valid until the next ug_dc_set_inputs): lets the caller hand
 * them to RCCL (torch.distributed) for the cross-GPU gather without a host round trip. */
int ug_dc_device_ptrs(ug_ctx* ctx, void** frames_dev, void** depth_dev, void** normals_dev);

/* StableNormal: replaces `self.predictor = torch.hub.load("Stable-X/StableNormal", "StableNormal")` (model/stablenormal.py:16) and
 * `self.predictor(image)` (:39).  The hub predictor's code is un-vendored; what runs here is the restatement documented in
 * oracle/stablenormal.py / DESIGN.md (UNPINNED): SD AutoencoderKL, two SD-2.1-class UNet2DConditionModels (one-step "YOSO" estimate
 * + DDIM refinement), two ControlNet trunks (image latent; image latent + DINOv2 tokens) and a DINOv2 ViT-L/14 tower.
 *   ug_bind_stablenormal : tensors uploaded with ug_load_tensor under "sn.vae.", "sn.unet_yoso.", "sn.controlnet_yoso.", "sn.unet.",
 *                          "sn.controlnet_dino.", "sn.dino."; sd = UNet2DConditionModel config (ug_unet_config; the SVD-only fields are
 *                          ignored), dino = ViT config (ug_clip_config; projection_dim ignored)
 *   ug_sn_run            : images [B,H,W,3] float32 in [0,1] (H, W multiples of 64; the frames of a clip are a batch - the reference
 *                          loops over them), prompt_embeds [77, cross_attention_dim] float32 (text-encoder output for the fixed
 *                          prompt, computed once by the caller), YOSO timestep, and the refinement schedule as data: nsteps DDIM
 *                          timesteps with the per-step update x <- ca[i]*x + cb[i]*unet(x, t_i)  ->  unit normals [B,H,W,3] in [-1,1] */
int ug_bind_stablenormal(ug_ctx* ctx, const ug_unet_config* sd, const ug_vae_config* vae, const ug_clip_config* dino);
int ug_sn_run(ug_ctx* ctx, const float* images_bhwc, int B, int H, int W, const float* prompt_embeds, float yoso_timestep, int nsteps,
              const float* timesteps, const float* ca, const float* cb, float* normals_out);
/* Antialiased bilinear resize [B,Hi,Wi,C] -> [B,Ho,Wo,C] (float32, C <= 4) on the device = torch F.interpolate(mode="bilinear",
 * align_corners=False, antialias=True); normalise = 1 re-normalises the channel vector of every output pixel (unit normals).  Used by the
 * StableNormal predictor's optional processing resolution (the hub predictor behind model/stablenormal.py:16,39 resizes its input to a fixed
 * processing resolution and the prediction back - DESIGN.md section 9, S1). */
int ug_resize_bilinear(ug_ctx* ctx, const float* in_bhwc, int B, int Hi, int Wi, int C, int Ho, int Wo, int normalise, float* out_bhwc);

int ug_normals_from_depth(ug_ctx* ctx, const float* depth_thw, const float* intrinsics_t33, int T, int H, int W,
                          float* normals_out);

/* Evaluation metrics on device.  pred == NULL uses the resident output of the last ug_dc_run
 * (depth [T,H,W] / normals [T,H,W,3]); gt / mask are host arrays (mask: 1 byte per pixel, may be NULL).
 *   ug_eval_depth  : replaces depth_evaluation(..., custom_mask, align_with_lstsq=True) (metrics/eval_depth.py:6-246,
 *                    metrics/alignment.py:150-167) -> out[11] = AbsRel, SqRel, RMSE, LogRMSE, d<1, d<1.25, d<1.25^2,
 *                    d<1.25^3, valid_pixels, scale, shift.  mask1 = 0 < gt < max_depth (a NaN or non-positive max_depth selects no
 *                    pixel).  In every ug_eval_depth* call the prediction must be free of NaN on mask1: such a pixel is read as -inf
 *                    (s comes out NaN here, UG_ALIGN_L1 rejects it)
 *   ug_eval_normal : replaces normal_evaluation (metrics/eval_normal.py:4-72) -> out[8] = mean, median, rmse,
 *                    %<5, %<7.5, %<11.25, %<22.5, %<30 */
int ug_eval_depth(ug_ctx* ctx, const float* pred_depth, const float* gt_depth, const unsigned char* custom_mask, long n,
                  float max_depth, double* out11);
int ug_eval_normal(ug_ctx* ctx, const float* pred_normals, const float* gt_normals, const unsigned char* mask, long n,
                   double* out8);
/* ug_eval_depth with the other alignment modes of the reference's depth_evaluation (metrics/eval_depth.py:59-204):
 * p = clamp(pred, pre_clip) on mask1 = gt > 0 (and gt < max_depth) -> (s, t) of the mode -> p' = clamp(s p + t, post_clip) -> the same metrics.
 *   UG_ALIGN_LSTSQ  (align_with_lstsq=True)  least-squares scale and shift, as ug_eval_depth, fitted on the pre-clipped p
 *   UG_ALIGN_MEDIAN (the reference's default) s = median(gt) / median(p), float32 division of the exact LOWER medians (torch.median), t = 0
 *   UG_ALIGN_SCALE  (align_with_scale=True)  s0 = mean(gt) / mean(p), ten Weiszfeld steps w = 1 / (|s p - gt| + 1e-8), s = sum(w p gt) / sum(w p p),
 *                   s = max(s, 1e-3), t = 0; sums and s in float64 with a fixed order: the same input gives the same bits.  The 1 / |r| weights make
 *                   this mode ill-conditioned at clip size - s moves by 1e-4 .. 3e-3 with the summation order alone, and the reference's float32
 *                   value is as far from any float64 one - so the value is deterministic, but no more "the" answer than another order's
 *   UG_ALIGN_METRIC (metric_scale=True)      s = 1, t = 0
 *   UG_ALIGN_L1     (no reference flag; takes the place of align_with_lad)  the exact minimiser of sum |s p + t - gt| over mask1 (DESIGN.md
 *                   section 23).  E = the smallest integer with max |p| < 2^E, q_i = rint(p_i * 2^(36 - E)) as a 64-bit integer (exact for every
 *                   p_i within 12 binades of the largest).  A step from pivot j: over the i with q_i != q_j, weights w_i = |q_i - q_j| and slopes
 *                   r_i = (double(g_i) - double(g_j)) / (double(q_i - q_j) * 2^(E - 36)), -0.0 read as 0.0; S = the LOWER WEIGHTED MEDIAN, the
 *                   smallest r whose weight at or below it reaches the weight above it - integer sums, found by a weighted radix select.  The
 *                   descent starts at the lowest index holding the lower median of p and takes one step.  At a vertex (j, S): Z = the points
 *                   whose slope through j equals S, one (lowest index) per distinct q; for each z of Z in index order, with pivot z, B / A = the
 *                   weight of the slopes below / above S and W the total; S is optimal along z's line iff 2B <= W and 2A <= W.  The first z
 *                   that fails becomes the pivot of the next step; when none fails the vertex is the minimiser.  s = S and
 *                   t = double(g_j) - s * (double(q_j) * 2^(E - 36)), each rounded once to float32.  Every q equal: s = 0, t = the lower median of
 *                   gt.  At most 64 steps and 4096 tied points at a vertex; past either cap the current vertex is returned and the call still
 *                   succeeds (ug_eval_depth_l1_info reports certified = 0).  2^26 valid pixels or more, or a non-finite prediction, is an error.
 *                   Scratch comes from the workspace: 12 bytes per valid pixel plus 100 KB; a workspace too small for it is an error
 * out11 as ug_eval_depth.  err_map_out (host, [n], may be NULL) = |s * pred + t - gt| / gt on mask1 and 0 elsewhere, from the ORIGINAL
 * (unclipped) prediction - the reference's second return value.  No valid pixel: zero metrics, (s, t) = (1, 0) for METRIC, (0, 0) otherwise.
 * An unknown alignment is an error (ug_last_error).  With the default options the result equals ug_eval_depth's bit for bit.
 * align_with_lad / align_with_lad2 (BFGS / 1000-step Adam on a non-smooth objective: no reproducible answer) have no counterpart; UG_ALIGN_L1
 * returns the exact minimiser of the objective lad / lad2 approach.  disp_input (alignment in disparity space) is ug_eval_depth_ex2 below, with the
 * function the reference calls and never defines supplied. */
enum { UG_ALIGN_LSTSQ = 0, UG_ALIGN_MEDIAN = 1, UG_ALIGN_SCALE = 2, UG_ALIGN_METRIC = 3, UG_ALIGN_L1 = 4 };
typedef struct { int alignment; float max_depth;            /* <= 0 or NaN: gt > 0 only */
                 float pre_clip_min, pre_clip_max, post_clip_min, post_clip_max; /* NaN: off */ } ug_depth_eval_opts;
void ug_depth_eval_opts_default(ug_depth_eval_opts* o);     /* LSTSQ, 80, all clips off */
int ug_eval_depth_ex(ug_ctx* ctx, const float* pred_depth /* NULL: resident depth */, const float* gt_depth, const unsigned char* custom_mask,
                     long n, const ug_depth_eval_opts* opts, double* out11, float* err_map_out /* [n] or NULL */);
/* How the last UG_ALIGN_L1 evaluation on this context ended: out_info[4] = j, k (the two valid pixels, counted in pixel order, that the fitted
 * line passes through; -1 where there is none), the number of pivot steps, certified (1: the vertex passed every check; 0: a cap was met). */
int ug_eval_depth_l1_info(ug_ctx* ctx, long* out_info /*[4]*/);
/* ug_eval_depth_ex with the alignment in DISPARITY space (the reference's depth_evaluation(..., disp_input=True), metrics/eval_depth.py:75-78,
 * 123-126,169-198, with the depth2disparity it never defines taken as y = 1 / x where x > 0, else 0).  With
 * UG_DEPTH_ALIGN_DISPARITY in flags, pred is a disparity.  Every operation below is one float32 operation rounded on its own, never fused:
 *   p = clamp(pred, pre_clip) and gd = 1 / (gt + 1e-8f) on mask1 = gt > 0 (and gt < max_depth), mask1 from the original gt
 *   (s, t) = the alignment of opts->base of p against gd, each mode exactly as ug_eval_depth_ex defines it with gd in the place of gt
 *   a = s * p + t;  with disp_clip_min = c (NaN: off), a = c where a < c;  d = 1 / a where a > 0, else 0 (a NaN a gives 0), the division
 *   correctly rounded;  d = clamp(d, post_clip);  the metrics of ug_eval_depth on d against the REAL gt over mask1 & custom_mask
 * err_map_out = |d0 - gt| / gt on mask1 and 0 elsewhere, d0 made in the same way from a0 = pred * s + t of the ORIGINAL prediction (no pre- or
 * post-clip; the floor applies).  No valid pixel: zero metrics and a zero map, (s, t) = (1, 0) for METRIC, (0, 0) otherwise.  Without the floor a
 * pixel whose aligned disparity is not positive becomes depth 0 (near); with it, 1 / c (far, then post-clipped) - the floor is not in the
 * reference; the benchmark protocol its file descends from clamps the aligned disparity at 1e-3.
 * pred_disp == NULL with the flag: the resident DISPARITY of the last ug_dc_run / ug_dc_run_windows - x = (m - lo) / (hi - lo), m the channel
 * mean of the resident decoded frames and (lo, hi) its min and max over the clip, the value the resident depth 1 / (x + 0.1f) was made from -
 * produced at evaluation time from the resident frames; ug_dc_get_disparity copies the same array to the host ([T*H*W], min 0, max 1).  Without
 * the flag pred == NULL is the resident depth, and with flags == 0 and the floor off the call is ug_eval_depth_ex: one shared body, its bytes.
 * ug_eval_depth_l1_info reports the last UG_ALIGN_L1 fit of either call.  Errors (ug_last_error; the context stays usable): an unknown flag bit;
 * a disp_clip_min that is not NaN and is <= 0 or infinite; a disp_clip_min without the flag; pred == NULL without a resident output of that
 * size (for the disparity: before any run); everything ug_eval_depth_ex rejects.  Scratch: 4 bytes per pixel more than ug_eval_depth_ex (8 with
 * the resident disparity). */
#define UG_DEPTH_ALIGN_DISPARITY 1
typedef struct { ug_depth_eval_opts base; unsigned flags; float disp_clip_min; /* NaN: off */ } ug_depth_eval_opts2;
void ug_depth_eval_opts2_default(ug_depth_eval_opts2* o);   /* base defaults, flags 0, NaN */
int ug_eval_depth_ex2(ug_ctx* ctx, const float* pred /* NULL: resident */, const float* gt_depth, const unsigned char* custom_mask, long n,
                      const ug_depth_eval_opts2* opts, double* out11, float* err_map_out /* [n] or NULL */);
int ug_dc_get_disparity(ug_ctx* ctx, float* disp_out /* host, [T*H*W] */);
/* Depth evaluation in global coordinates: the reference's depth_evaluation_in_global_coord (metrics/eval_depth.py:250-441,
 * utils/geometry_utils.py:246-253).  mask1 = gt_depth > 0 (and gt_depth < max_depth) - from the ground-truth DEPTH, never
 * from the radius.  Fit 1: least squares (s_d, t_d) of clamp(pred, pre_clip) against gt_depth on mask1.  Every pixel, from the ORIGINAL
 * prediction: d = clamp(s_d * pred + t_d, post_clip) in float32, the product and the sum rounded separately; in float64 from that d,
 * x = (col - cx) * d / fx, y = (row - cy) * d / fy, z = d (integer pixel indices, no half-pixel offset), world = R (x, y, z) + t with the top
 * three rows of the frame's pose, r = |world| rounded once to float32.  Fit 2: least squares (s_r, t_r) of r against gt_radius on mask1.
 * radius_map_out (host, [T*H*W], may be NULL) = s_r * r + t_r for every pixel; the metrics of ug_eval_depth on it against gt_radius over
 * mask1 & custom_mask, no clamp at that stage.  cam2world_t44: [T,4,4] row-major camera-to-world (OpenCV), intrinsics_t33: [T,3,3].
 * out13[0..8] as ug_eval_depth, out13[9..10] = (s_r, t_r), out13[11..12] = (s_d, t_d).  Both fits are float64 normal equations with
 * ug_eval_depth's degenerate cases; no valid pixel: zero metrics, both fits (0, 0), a zero map.  opts: max_depth and the clip bounds as in
 * ug_eval_depth_ex; alignment must be UG_ALIGN_LSTSQ (the reference asserts it).  Errors (ug_last_error; the context stays usable): another
 * alignment; NULL opts / gt_depth / gt_radius / cam2world / intrinsics / out13; T, H or W <= 0; 2^32 pixels or more; pred_depth == NULL
 * without a resident depth of that shape.  A ground-truth radius of 0 on mask1 divides by zero, as in the reference. */
int ug_eval_depth_global(ug_ctx* ctx, const float* pred_depth /* NULL: resident depth */, const float* gt_depth, const float* gt_radius,
                         const float* cam2world_t44, const float* intrinsics_t33, const unsigned char* custom_mask /* or NULL */, int T, int H,
                         int W, const ug_depth_eval_opts* opts, double* out13, float* radius_map_out /* [T*H*W] or NULL */);
/* Temporal alignment error (TAE) of a video depth (kernels/temporal.hip, harness/temporal.py).  UNPINNED: the reference
 * has no such metric; it is restated from the published definition (ChronoDepth, Video Depth Anything), with one deliberate difference below.
 * Aligned depth d of every pixel, float32, each operation rounded on its own, from the ORIGINAL prediction and the (s, t) that the clip's depth
 * evaluation reported: a = fl(fl(s * pred) + t); with UG_DEPTH_ALIGN_DISPARITY, a = disp_clip_min where a is below it, d = 1 / a where a > 0,
 * else 0; then d = post_clip_min where d is below it and post_clip_max where above (a NaN stays NaN).  Pre-clips enter through (s, t) only.
 * Directed pairs P = 2 * (T - stride): pair 2i carries frame a = i into b = i + stride, pair 2i + 1 carries a = i + stride into b = i;
 * rel_p34[p] = (inv(C_b) C_a)[:3] in float64, built on the host (harness/temporal.py relative_poses).
 * Splat: a source pixel (row, col) of frame a with d > 0 and finite; in float64, one IEEE operation per step, never fused:
 *   D = d;  X = ((col - cx_a) * D) / fx_a;  Y = ((row - cy_a) * D) / fy_a   (integer pixel indices, no half-pixel offset)
 *   x3 = ((m0 * X + m1 * Y) + m2 * D) + m3, likewise y3, z3;  u = rint(((x3 / z3) * fx_b) + cx_b), v likewise (ties to even);  z = float32(z3)
 * kept when z3 > 0, z > 0, z finite, u >= 0, v >= 0, v < H and u < W (a NaN anywhere drops the pixel).  The target pixel keeps the smallest z
 * that reaches it (an integer atomicMin on an order-preserving key: the bytes do not depend on the order of arrival).  There is no source mask.
 * Score: a reached target pixel q of pair p with d_b[q] > 0, 0 < gt_b[q] (and gt_b[q] < max_depth) and custom_mask_b[q] gives
 * e = fl(|z - d_b|) / d_b in float32; the pair's value is sum(double(e)) / count, the sum in the fixed order of kernels/eval_reduce.h.  A pair
 * with count == 0 is left out and counted as unscored - the deliberate difference: the published code scores it as 0.
 * out4 = TAE (the mean of the scored pairs' values, a fraction like Abs Rel; NaN when no pair is scored), pairs scored, pairs total, pixels scored.
 * pair_out [P,2] = value (NaN when unscored), count; warp_out [P,H,W] = the warped depth, 0 where unreached; err_out [P,H,W] = e, 0 where
 * unscored (host arrays, each may be NULL).  pred == NULL: the resident depth of the last run, with the flag its resident disparity.
 * T <= stride is no error: NaN, 0, 0, 0.  Errors (ug_last_error; the context stays usable): NULL opts / gt_depth / intrinsics / rel / out4;
 * T, H or W <= 0; stride < 1; an unknown flag bit; a disp_clip_min that is not NaN and is <= 0 or infinite, or that comes without the flag;
 * pred == NULL without a resident output of that shape; 2^31 or more pair-pixels P * H * W; a workspace too small (the message names the bytes
 * needed).  Scratch: 4 bytes per pair-pixel for the z-buffer, 4 more for each requested map, and the uploads. */
typedef struct { float s, t; unsigned flags /* UG_DEPTH_ALIGN_DISPARITY */; float disp_clip_min, post_clip_min, post_clip_max /* NaN: off */;
                 float max_depth /* <= 0 or NaN: gt > 0 only */; int stride; } ug_tae_opts;
void ug_tae_opts_default(ug_tae_opts* o);      /* 1, 0, 0, NaN, NaN, NaN, 80, 1 */
int ug_eval_tae(ug_ctx* ctx, const float* pred /* NULL: resident depth; with the flag, the resident disparity */, const float* gt_depth,
                const unsigned char* custom_mask /* or NULL */, const float* intrinsics_t33, const double* rel_p34 /* [P,3,4] */,
                int T, int H, int W, const ug_tae_opts* opts, double* out4 /* TAE, pairs scored, pairs total, pixels scored */,
                double* pair_out /* [P,2] value,count or NULL */, float* warp_out /* [P,H,W] or NULL */, float* err_out /* [P,H,W] or NULL */);

/* Point-cloud evaluation: the reference's eval_pcd branch (eval.py:66-83, metrics/eval_pcd.py:10-168 with pcd_alignment.py, metrics/utils.py:14-42
 * and the Open3D calls it makes; kernels/pcd.hip).
 * ug_pcd_world_points: the first half of ug_eval_depth_global - fit 1, d = clamp(s_d * pred + t_d, post_clip) in float32, float64 back-projection
 *   and world transform - with every coordinate rounded once to float32.  out_fit2 = (s_d, t_d); out_pts (host, [T*H*W*3], may be NULL).  The points
 *   stay resident on the device until the next ug_pcd_world_points; ug_eval_pcd reads them with pred_pts == NULL.  opts as in ug_eval_depth_global.
 * ug_eval_pcd: pred_pts (NULL: the resident points) / gt_pts float32 [n_pixels,3], mask uint8 [n_pixels] (> 0 keeps the pixel).  Masked
 *   selection in pixel order; the alignment of Regr3D_t_ScaleShiftInv(norm_mode=False, gt_scale=True) on ALL masked points (exact lower medians;
 *   the norms behind the scales in float64, rounded once); then the points at positions sample_idx[0 .. n_sample) of the masked sequence (NULL:
 *   all of them); point-to-point ICP from the identity (nearest neighbour closer than threshold, Umeyama without scaling, stop when fitness and
 *   inlier rmse both move by less than 1e-6 or after max_iteration updates); normals from the float64 covariance of the min(knn, n) nearest
 *   points ((0, 0, 1) below 3 points); accuracy / completion of metrics/utils.py.  All pair arithmetic is unfused float64; the nearest target is
 *   the one with the smallest (dx*dx + dy*dy) + dz*dz, ties to the lowest index.  out32: acc, comp, nc1, nc2, acc_med, comp_med, nc1_med,
 *   nc2_med, n_points, icp_iterations, icp_fitness, icp_rmse, transformation[16] row-major, pred_scale (clipped), gt_scale, pred_shift_z,
 *   gt_shift_z.  pred_cloud_out / gt_cloud_out (host, [n_points*3] float32, may be NULL): the aligned, sampled clouds before ICP.  No masked
 *   pixel: n_points = 0, NaN metrics and scalars, the identity.  Errors (ug_last_error; the context stays usable): NULL opts / gt_pts / mask /
 *   out32; n_pixels <= 0 or >= 2^31; pred_pts == NULL without resident points of that size; a sample index outside the masked points; knn outside
 *   1..UG_PCD_MAX_KNN; threshold <= 0; max_iteration < 0; more than 2^40 point pairs in one pass (lower pcd_downsample_num). */
enum { UG_PCD_MAX_KNN = 32 };
typedef struct { float threshold; int max_iteration; int knn; } ug_pcd_opts;
void ug_pcd_opts_default(ug_pcd_opts* o);     /* 0.1, 30, 30 */
int ug_pcd_world_points(ug_ctx* ctx, const float* pred_depth /* NULL: resident depth */, const float* gt_depth, const float* cam2world_t44,
                        const float* intrinsics_t33, int T, int H, int W, const ug_depth_eval_opts* opts, float* out_fit2,
                        float* out_pts /* [T*H*W*3] or NULL */);
int ug_eval_pcd(ug_ctx* ctx, const float* pred_pts /* NULL: resident points */, const float* gt_pts, const unsigned char* mask, long n_pixels,
                const long* sample_idx /* or NULL */, long n_sample, const ug_pcd_opts* opts, double* out32, float* pred_cloud_out /* or NULL */,
                float* gt_cloud_out /* or NULL */);
/* ug_eval_pcd_fps: ug_eval_pcd with farthest-point sampling in place of the index list (the reference's disabled branch, metrics/eval_pcd.py:84-93,
 *   172-193).  After the alignment of ALL masked points, each aligned float32 cloud is sampled on its own: m[j] = +inf for a
 *   point with three finite coordinates, else -1; step i picks s = argmax m (ties to the lowest index, so step 0 is the first finite point), then
 *   m[j] = d if d < m[j] with d = (dx*dx + dy*dy) + dz*dz in unfused float32.  The n_sample picked points of each cloud, in pick order, go on to
 *   the ICP, the normals and the scores.  n_sample <= 0 or n_sample >= the masked count: every point, no sampling, ug_eval_pcd with no index list.
 *   out32 as ug_eval_pcd (n_points = the sampled count); pred_idx_out / gt_idx_out (host, [n_points], may be NULL): the picked positions in the
 *   masked sequence (0 .. n_points - 1 without sampling).  Errors as ug_eval_pcd; the 2^40 pair cap counts the sampled sizes. */
int ug_eval_pcd_fps(ug_ctx* ctx, const float* pred_pts /* NULL: resident points */, const float* gt_pts, const unsigned char* mask, long n_pixels,
                    long n_sample, const ug_pcd_opts* opts, double* out32, float* pred_cloud_out /* or NULL */, float* gt_cloud_out /* or NULL */,
                    long* pred_idx_out /* or NULL */, long* gt_idx_out /* or NULL */);
/* ug_eval_pcd_ex: both calls above behind one flag word, plus the choice of the search.
 *   UG_PCD_FPS        : farthest-point sampling as ug_eval_pcd_fps (sample_idx must then be NULL); without it sample_idx / n_sample as ug_eval_pcd.
 *   UG_PCD_SEARCH_GRID: every nearest-neighbour pass (ICP, accuracy, completion) and both KNN passes go through a uniform grid over the target
 *                       cloud - one grid over the ground truth and one over the moved prediction, each built once.  The search is exact: a query
 *                       that the grid cannot settle within a few rings of cells is finished by the brute-force kernels, so every output is
 *                       bit-equal to the call without the flag.  The 2^40 pair cap then counts only those leftover queries times the target
 *                       size, which is what lets an unsampled clip (pcd_downsample_num = -1) run.
 *   ug_eval_pcd(...) is ug_eval_pcd_ex(..., 0, ...), ug_eval_pcd_fps(...) is ug_eval_pcd_ex(..., NULL, n_sample, ..., UG_PCD_FPS, ...).
 *   search_stats (host, [8], may be NULL; zeros without the grid flag): queries settled by a grid and leftover queries, both summed over all
 *   passes; cells and fullest cell of the ground-truth grid; cells and fullest cell of the moved-prediction grid; peak workspace bytes; 0.
 *   Errors as above, and a flag bit other than the two named here (the context stays usable). */
#define UG_PCD_FPS         1
#define UG_PCD_SEARCH_GRID 2
int ug_eval_pcd_ex(ug_ctx* ctx, const float* pred_pts /* NULL: resident points */, const float* gt_pts, const unsigned char* mask, long n_pixels,
                   const long* sample_idx /* or NULL */, long n_sample, const ug_pcd_opts* opts, int flags, double* out32,
                   float* pred_cloud_out /* or NULL */, float* gt_cloud_out /* or NULL */, long* pred_idx_out /* or NULL */,
                   long* gt_idx_out /* or NULL */, long* search_stats /* [8] or NULL */);
/* ug_eval_pcd_scores: ug_eval_pcd_ex plus precision / recall counts at distance thresholds and voxel-set counts for an occupancy IoU (DESIGN.md
 * section 32; kernels/pcd.hip k_pcd_count_below, kernels/voxel.hip).  Both go beyond what the reference evaluates: metrics/utils.py carries
 * completion_ratio (:7-11, recall at 0.05) and compute_iou (:45-60) and calls neither.
 *   thresholds[0 .. n_thresholds), n_thresholds 0..8, each positive and finite: score_counts[2 * k] = how many moved predictions lie strictly
 *     closer than thresholds[k] to their nearest ground-truth point, score_counts[2 * k + 1] = how many ground-truth points lie strictly closer
 *     than that to their nearest moved prediction.  The distances are the arrays that acc and comp are the means of; no second search runs.
 *     precision = count / n_points, recall likewise, in float64 on the host.
 *   voxel_sizes[0 .. n_voxel_sizes), n_voxel_sizes 0..4, each positive and finite: a point's cell is floor(x / v) per axis from the world origin;
 *     a point with a non-finite coordinate or a cell index outside (-2^20, 2^20) is skipped.  voxel_counts[6 * k ..] = cells of the moved
 *     prediction, cells of the ground truth, cells of both, cells of either, skipped predictions, skipped ground-truth points.
 *   With both counts 0 (or sopts NULL) the call is ug_eval_pcd_ex: the same launches, the same outputs.  An empty mask gives zero counts.
 *   Errors (the context stays usable): a count outside its range, a threshold or voxel size that is not positive and finite, a NULL output for
 *   a non-zero count, a voxel table that overflowed, and a workspace too small - the message names the bytes the call needs. */
typedef struct { int n_thresholds; double thresholds[8]; int n_voxel_sizes; double voxel_sizes[4]; } ug_pcd_score_opts;
void ug_pcd_score_opts_default(ug_pcd_score_opts* o);     /* both counts 0 */
int ug_eval_pcd_scores(ug_ctx* ctx, const float* pred_pts /* NULL: resident points */, const float* gt_pts, const unsigned char* mask, long n_pixels,
                       const long* sample_idx /* or NULL */, long n_sample, const ug_pcd_opts* opts, int flags, double* out32,
                       float* pred_cloud_out /* or NULL */, float* gt_cloud_out /* or NULL */, long* pred_idx_out /* or NULL */,
                       long* gt_idx_out /* or NULL */, long* search_stats /* [8] or NULL */, const ug_pcd_score_opts* sopts,
                       long* score_counts /* [8 * 2] */, long* voxel_counts /* [4 * 6] */);

/* Focal, camera poses and depth from world point maps: what the reference's point-map plugins take from
 * solve_depth_and_camera_from_3d_points (metrics/utils.py:68-160, called from model/spann3r.py:43; kernels/pointmap.hip).
 * The arithmetic is that of harness/pointmap.py in unfused float64, every sum in a fixed order; two calls return the same bytes.
 * ug_pointmap_focal: estimate_focal_knowing_depth(pts[0:1], pp, 'weiszfeld') (metrics/utils.py:93-115) of pts0 float32 [H,W,3], the point map of
 *   the frame whose camera is the world frame; pp = (cx, cy), the reference passes (W/2, H/2).  xy = (x/z, y/z) with non-finite values set to 0,
 *   pixel grid 0..W-1, 0..H-1 minus pp, f0 = mean(xy.px) / mean(xy.xy), ten steps f = mean(w xy.px) / mean(w xy.xy) with
 *   w = 1 / max(|px - f xy|, 1e-8), means over all pixels, clipped below at 0.  The reference runs this in float32.
 * ug_pointmap_poses: in place of cv2.solvePnPRansac (random samples) a deterministic solver.  pts float32 [T,H,W,3] world points; mask uint8
 *   [T,H,W] (> 0 keeps, may be NULL); a pixel is valid when its three coordinates are finite and the mask keeps it.  Unit rays
 *   b = normalize(K^-1 (col, row, 1)), K from focal and (cx, cy).  Per frame the orthogonal (object-space) iteration of Lu, Hager and Mjolsness
 *   with V = b b^T: t = (1/n) (I - mean V)^-1 sum (V - I) R X, q = V (R X + t), next R = Kabsch of the centred X onto the centred q; frame 0 starts
 *   from the identity, every other frame from the frame before.  A fit ends when E = sum |(I - V)(R X + t)|^2 changes by less than a relative
 *   1e-12, or E or its change is at most 1e-6 sum (2^-24 |X|)^2, or after max_iter iterations.  Then the pixels whose reprojection error exceeds
 *   reproj_px or whose camera z <= 0 are dropped and the fit continues from the current pose, until no membership changes or max_rounds trims
 *   were made (a trim that would leave fewer than 4 pixels is not made).  extrinsics_out [T,16] row-major world to camera (cam2world is its
 *   inverse); depth_out float32 [T,H,W] = z of R X + t rounded once, 0 at invalid pixels; frame_stats_out [T,3] = inlier count, iterations (all
 *   fits of the frame), rms reprojection error of the inliers in pixels; inliers_out uint8 [T,H,W] (may be NULL) the final inlier set.
 * Errors (ug_last_error; the context stays usable): a NULL pts, opts or required output; T, H or W <= 0, or H * W >= 2^31; a focal that is not
 *   positive and finite; reproj_px <= 0, max_iter < 1 or max_rounds < 0; a frame with fewer than 4 valid pixels (the frame is named). */
typedef struct { double reproj_px; int max_iter; int max_rounds; } ug_pointmap_opts;
void ug_pointmap_opts_default(ug_pointmap_opts* o);     /* 8.0 (cv2's default), 300, 5 */
int ug_pointmap_focal(ug_ctx* ctx, const float* pts0, int H, int W, double cx, double cy, double* focal_out);
int ug_pointmap_poses(ug_ctx* ctx, const float* pts, const unsigned char* mask /* or NULL */, int T, int H, int W, double focal, double cx,
                      double cy, const ug_pointmap_opts* opts, double* extrinsics_out, float* depth_out, double* frame_stats_out,
                      unsigned char* inliers_out /* or NULL */);

/* Visualisation panels composed on the device: replaces save_depth_normal_maps / colorize / colorize_np (utils/vis_utils.py:38-84,139-199, as
 * eval.py:58-62 calls them under `vis_depth: True`).  One image per frame, uint8 [T,H,Wp,3] row-major,
 *   Wp = (rgb ? W : 0) + W + W + (cbar ? 5 + Wc : 0):   rgb | normals | coloured depth | 5 black columns | colour bar.
 * Every step is one IEEE float32 operation, rounded on its own (fl32), and u8(v) = trunc(v) saturated to 0..255 with NaN -> 0 (numpy's cast is
 * undefined outside 0..255 - a deliberate difference no reference input reaches):
 *   rgb        u8(fl32(r * 255))                      r: float32 [T,H,W,3] in [0,1]
 *   normals    t = fl32(fl32(n * 0.5) + 0.5); u8(fl32(t * 255))
 *   depth      x = min(max(d, vmin), vmax); u = fl32(fl32(x - vmin) / fl32(vmax - vmin)) (correctly rounded division);
 *              i = min((int)fl32(u * 256), 255); the bytes are row i of the colour table u8(fl32(lut * 255)), lut: float32 [256,3].
 *              NaN depth, or vmax == vmin (0 / 0), gives 0,0,0 - matplotlib's "bad" colour
 *   colour bar u8(fl32(c * 255))                      c: float32 [H,Wc,3], the same strip for every frame
 * ug_vis_depth_range: out2 = (min, max) of float32 [n], NaN ignored; all NaN or n == 0 gives (0, 0) (the reference's depth_maps.min() / .max()
 *   propagate NaN instead).  It is a call of its own because the colour bar's tick labels depend on it: the host renders the strip between the
 *   two calls, and ug_vis_panels takes vmin / vmax as inputs, like colorize(range=...).
 * depth / normals NULL: the resident outputs of the last ug_dc_run on the current inputs.  rgb_mode: UG_VIS_RGB_NONE no rgb section (rgbs
 *   ignored), UG_VIS_RGB_HOST rgbs = host [T,H,W,3], UG_VIS_RGB_RESIDENT the input frames of the last ug_dc_set_inputs* (rgbs ignored).
 *   cbar NULL: no gap and no colour bar, Wc ignored.
 * Errors (ug_last_error; the context stays usable): NULL lut, panels_out or out2; T, H or W <= 0; n < 0; Wc < 0, or cbar given with Wc == 0;
 *   unknown rgb_mode; UG_VIS_RGB_HOST with NULL rgbs; a NULL / resident request without a resident tensor of that shape (for normals also when
 *   the last run had with_normals = 0, or no run followed the last ug_dc_set_inputs*); 2^31 output bytes or more. */
enum { UG_VIS_RGB_NONE = 0, UG_VIS_RGB_HOST = 1, UG_VIS_RGB_RESIDENT = 2 };
int ug_vis_depth_range(ug_ctx* ctx, const float* depth /* NULL: resident depth */, long n, float* out2 /* vmin, vmax */);
int ug_vis_panels(ug_ctx* ctx, const float* depth /* NULL: resident */, const float* normals /* NULL: resident */, const float* rgbs, int rgb_mode,
                  int T, int H, int W, float vmin, float vmax, const float* lut_256x3, const float* cbar_hwc3 /* [H,Wc,3] or NULL */, int Wc,
                  unsigned char* panels_out /* host, [T,H,Wp,3] */);

/* ScanNet++ clip preparation on the device: replaces the pixel arithmetic of the reference's loader (dataset/scannetpp/scannetpp.py:81-187) and
 * of its resize transforms (dataset/dataset_core/transforms.py:38-110).  The host decodes the files and builds the tables.
 * ug_prep_resize_frames: the anti-aliased order-1 input resize (scikit-image's resize recipe: gaussian pre-filter, then grid-mode zoom, both in
 *   'mirror' mode) as a separable linear map.  frames: host uint8 [T,Hi,Wi,3], channels last.  Per axis a tap table of fixed length,
 *   row_idx / row_w [Ho,Kr] and col_idx / col_w [Wo,Kc]: output o = sum_k w[o,k] * source[idx[o,k]] (pad a short row with weight 0).  Two
 *   passes, rows first: mid[t,c,oy,x] = sum_k row_w[oy,k] * frames[t,row_idx[oy,k],x,c] kept in float64, then
 *   out[t,c,oy,ox] = fl32(sum_k col_w[ox,k] * mid[t,c,oy,col_idx[ox,k]]); both sums in float64 in the table's tap order, ONE rounding to
 *   float32 at the end.  out: host float32 [T,3,Ho,Wo], planar, 0..255.  The clip is processed in chunks of frames of bounded device size.
 * ug_prep_gt: the ground truth at the pixels an order-0 target resize keeps.  Output pixel (oy, ox) of frame t is computed from source pixel
 *   (v, u) = (row_idx[oy], col_idx[ox]) - the identity tables without a resize.  Every fl32 below is ONE IEEE float32 operation:
 *   depth  d = fl32(float(depth_u16) / depth_divisor)
 *   camera x = fl32((u - cx) * d / fx), y = fl32((v - cy) * d / fy), each evaluated in float64 from the frame's intrinsics_t33;
 *          cam_coord = (x, -y, -d)  (OpenGL)
 *   normal n_j = fl32(fl32(fl32(byte_j / 255) * 2) - 1), n = 0 where all three bytes are 0; normals_u8 NULL: n = 0, and cam_normal_out /
 *          world_normal_out may then be NULL
 *   world  world_normal = fl32(M33 n), world_coord = fl32(M33 cam_coord + t), the sums in float64 and rounded once, M33 | t the top three rows
 *          of the frame's cam2key_t44 (source camera -> key view, row-major)
 *   bad    = isnan(x) | isnan(y) | isnan(d) | d < 1e-3f | d > max_depth;  all four arrays are 0 on bad, mask = bad ? 0 : 1
 *   zero   where (Ho, Wo) differs from (Hi, Wi) - the host's order-0 zoom ran - a -0 (y = 0 on the principal row) comes out as +0, as the zoom's
 *          sum 0 + 1 * v makes it; at the source size the sign of a zero is kept, as the host keeps it
 *   Outputs are host float32: cam_normal / cam_coord / world_normal / world_coord [T,3,Ho,Wo], mask [T,Ho,Wo].  cam_normal, cam_coord and mask
 *   equal the host loader's bit for bit; the world arrays differ from its float32 matrix product by that product's rounding.
 * Errors (ug_last_error; the context stays usable): a NULL required pointer; T, a size or a tap count <= 0; a tap, row or column index outside
 *   the source (checked on the host before anything is uploaded); 2^31 output elements (T * 3 * Ho * Wo) or more. */
int ug_prep_resize_frames(ug_ctx* ctx, const unsigned char* frames_thwc3, int T, int Hi, int Wi, int Ho, int Wo, const int* row_idx,
                          const double* row_w, int Kr, const int* col_idx, const double* col_w, int Kc, float* out /* host, [T,3,Ho,Wo] */);
int ug_prep_gt(ug_ctx* ctx, const unsigned short* depth_u16 /* [T,Hi,Wi] */, float depth_divisor, const unsigned char* normals_u8 /* [T,Hi,Wi,3] or NULL */,
               const float* intrinsics_t33, const float* cam2key_t44, int T, int Hi, int Wi, const int* row_idx /* [Ho] */, int Ho,
               const int* col_idx /* [Wo] */, int Wo, float max_depth, float* cam_normal_out, float* cam_coord_out, float* world_normal_out,
               float* world_coord_out, float* mask_out);
/* ug_prep_gt with two explicit switches, for loaders whose depth arithmetic or geometry differs from ScanNet++'s (harness/rgbd.py; DESIGN.md
 * section 17).  Everything ug_prep_gt documents holds, except:
 *   UG_PREP_DEPTH_F64  the depth stays float64 from the division to the end of the back-projection (bonn.py:123-134), one rounding per component:
 *                      d64 = double(depth_u16) / double(depth_divisor)
 *                      x = fl32((u - cx) * d64 / fx), y = fl32((v - cy) * d64 / fy), d = fl32(d64);  cam_coord = (x, -y, -d)
 *                      bad tests d, the float32 value, as the host tests -cam_coord[2].  A raw 0 gives d = 0: masked, all outputs +0 - what the
 *                      host's NaN -> masked -> 0 gives.  Without the flag d = fl32(float(depth_u16) / depth_divisor) enters the float64 expressions.
 *   UG_PREP_ZOOMED     the "zero" rule as an argument instead of a size comparison: with the flag a -0 comes out as +0 (the host's order-0 zoom
 *                      ran on the targets), without it the sign of a zero is kept - also where (Ho, Wo) differs from (Hi, Wi) because the tables
 *                      describe a crop, which the host does by slicing.
 * ug_prep_gt(...) is ug_prep_gt_ex(..., (Ho != Hi || Wo != Wi) ? UG_PREP_ZOOMED : 0).
 * Errors, in addition: a flag bit other than the two above (the bits are named in ug_last_error; the context stays usable). */
#define UG_PREP_DEPTH_F64 1   /* depth kept in float64 through the back-projection (Bonn) */
#define UG_PREP_ZOOMED    2   /* the host's order-0 zoom ran on the targets: -0 comes out as +0 */
int ug_prep_gt_ex(ug_ctx* ctx, const unsigned short* depth_u16 /* [T,Hi,Wi] */, float depth_divisor, const unsigned char* normals_u8 /* [T,Hi,Wi,3] or NULL */,
                  const float* intrinsics_t33, const float* cam2key_t44, int T, int Hi, int Wi, const int* row_idx /* [Ho] */, int Ho,
                  const int* col_idx /* [Wo] */, int Wo, float max_depth, float* cam_normal_out, float* cam_coord_out, float* world_normal_out,
                  float* world_coord_out, float* mask_out, unsigned flags);

/* Ground-truth normals for the loaders that have none (7-Scenes, Bonn, NeuralRGBD, Replica, ScanNetv2; harness/rgbd.py `normals="depth"`;
 * DESIGN.md section 30): a plane fit to the back-projected depth, the reference's get_surface_normal_np (utils/geometry_utils.py:73-134, as
 * test_vis_dataset.py uses it on 7-Scenes) with a masked window, an edge test and a validity mask.  The inputs, the tables, the two flags and
 * the back-projection are ug_prep_gt_ex's: p(v, u) = cam_coord and bad(v, u) of NATIVE pixel (v, u) as documented above, computed by the same
 * device function.  The fit runs on the full native frame and is produced only at the picked pixels (v, u) = (row_idx[oy], col_idx[ox]).
 * ONE definition, evaluated identically here and by harness/normals.py's fit_normals.  Below the float32 points are widened to float64, every
 * operation is ONE IEEE float64 operation, never contracted into an FMA, in the order the brackets give, and every sum runs left to right
 * from +0:
 *   centre   pc = p(v, u), dc = -pc.z.  bad(v, u): the pixel is invalid.
 *   window   offsets (dy, dx), dy = -r..r outer, dx = -r..r inner (row-major); q = (v + dy, u + dx) is absent outside 0 <= row < Hi,
 *            0 <= col < Wi; it takes part iff !bad(q) and, with edge >= 0, |(-p(q).z) - dc| <= edge * dc.  The centre always takes part.
 *   sums     cnt = number of participants;  Sxx = sum x*x, Sxy = sum x*y, Sxz = sum x*z, Syy = sum y*y, Syz = sum y*z, Szz = sum z*z;
 *            sx = sum x, sy = sum y, sz = sum z  over the participants' (x, y, z) = p(q).  cnt < min_count: the pixel is invalid.
 *   system   c = double(cnt);  axx = Sxx/c + 1e-6, ayy = Syy/c + 1e-6, azz = Szz/c + 1e-6, axy = Sxy/c, axz = Sxz/c, ayz = Syz/c;
 *            bx = sx/c, by = sy/c, bz = sz/c  (with the full 5 x 5 window the reference's ATA + 1e-6 I and AT1)
 *   adjugate c00 = ayy*azz - ayz*ayz,  c01 = axz*ayz - axy*azz,  c02 = axy*ayz - axz*ayy,
 *            c11 = axx*azz - axz*axz,  c12 = axy*axz - axx*ayz,  c22 = axx*ayy - axy*axy   (each two products and one difference)
 *   solve    det = (axx*c00 + axy*c01) + axz*c02
 *            n0 = ((c00*bx + c01*by) + c02*bz) / det,  n1 = ((c01*bx + c11*by) + c12*bz) / det,  n2 = ((c02*bx + c12*by) + c22*bz) / det
 *   unit     den = sqrt((n0*n0 + n1*n1) + n2*n2) + 1e-6;  n = (n0/den, n1/den, n2/den)   (the reference's n / (|n| + 1e-6))
 *   orient   n = -n where (n0*pc.x + n1*pc.y) + n2*pc.z > 0: the normal faces the camera
 *   valid    iff the centre is valid, cnt >= min_count and n0, n1, n2 are finite
 *   outputs  cam_normal = fl32(n);  world_normal_j = fl32((m_j0*g0 + m_j1*g1) + m_j2*g2) with g = cam_normal widened and m = M33 of the
 *            frame's cam2key_t44, rounded once;  normal_mask = 1.  An invalid pixel gives +0 in all seven values.  UG_PREP_ZOOMED: a -0
 *            comes out as +0, as in ug_prep_gt_ex; without it the sign of a zero is kept.
 * ug_gt_normals_opts: radius r in 1..8 (2 = the reference's patch_size 5); edge < 0 switches the edge test off; min_count 0 = the majority of
 *   the full window, (2r+1)^2 / 2 + 1 (integer division).  ug_gt_normals_opts_default: 2, 0.05, 0.  edge and the majority count are design
 *   choices, not measurements; opts NULL: the defaults.
 * Outputs are host float32: cam_normal / world_normal [T,3,Ho,Wo], normal_mask [T,Ho,Wo].  One thread per picked pixel walks its window; no
 * atomics.  The clip is processed in chunks of frames of bounded device size.
 * Errors (ug_last_error; the context stays usable; all are found on the host before anything is uploaded): a NULL required pointer; T or a
 *   size <= 0; a row or column index outside the source; radius outside 1..8; a NaN edge; a negative min_count; a flag bit other than
 *   UG_PREP_DEPTH_F64 | UG_PREP_ZOOMED (the bits are named); 2^31 output elements (T * 3 * Ho * Wo) or more. */
typedef struct {
  int radius;      /* 2 */
  double edge;     /* 0.05; negative: off */
  int min_count;   /* 0: (2 * radius + 1)^2 / 2 + 1 */
} ug_gt_normals_opts;
void ug_gt_normals_opts_default(ug_gt_normals_opts* o);
int ug_prep_gt_normals(ug_ctx* ctx, const unsigned short* depth_u16 /* [T,Hi,Wi] */, float depth_divisor, const float* intrinsics_t33,
                       const float* cam2key_t44, int T, int Hi, int Wi, const int* row_idx /* [Ho] */, int Ho, const int* col_idx /* [Wo] */,
                       int Wo, float max_depth, const ug_gt_normals_opts* opts /* NULL: defaults */, float* cam_normal_out,
                       float* world_normal_out, float* normal_mask_out, unsigned flags);

/* 7-Scenes depth registration on the device: the raw Kinect depth image warped into the colour camera - what the reference does once, offline,
 * in dataset/sevenScenes/preprocess.py:82-140, to write the *.depth.proj.png files its loader reads.  A forward splat
 * with a z-buffer.  depth_u16 / out: host uint16 [T,H,W]; the output has the input's size and both principal points sit at the image centre.
 * fl32 / fl64 below are ONE IEEE operation in that type, never contracted into an FMA; every sum runs left to right.
 *   depth    d = fl32(float(raw) / divisor).  The pixel takes part iff d > 0 && d < max_valid (and, with UG_REG_DROP_SENTINEL, raw != 65535).
 *            From here on d is widened to float64.
 *   source   X = fl64(fl64(fl64(fl64(0.5 + col) - W/2) / src_focal) * d),  Y likewise with row and H/2,  Z = d
 *   target   x3 = fl64(fl64(fl64(fl64(m00*X) + fl64(m01*Y)) + fl64(m02*Z)) + m03), y3 and z3 likewise from rows 1 and 2 of src2dst
 *   project  u = fl64(fl64(fl64(x3 / z3) * dst_focal) + W/2), v likewise with y3 and H/2;  xi = rint(u), yi = rint(v), ties to even.
 *            The point is kept iff xi >= 0 && yi >= 0 && yi < H && xi < W, compared as float64 before any integer cast (a NaN is dropped).
 *   minimum  zbuf[yi, xi] = min over the points that land there of fl32(z3), and 2000f where none does
 *   output   z = zbuf > 1000f ? 0 : zbuf;  v = fl32(1000f * z);  out = int32(trunc(v)) modulo 65536.  A v outside int32 (it cannot occur with
 *            the defaults) gives 0.
 * The modulo is part of the definition: 7-Scenes marks an invalid raw pixel with 65535, which passes the depth test as 65.535 m; where such a
 * point fills a hole with z3 > 65.535 m its output wraps to a few hundred millimetres, as it does in the reference's files.
 * UG_REG_DROP_SENTINEL leaves those pixels out; after that only a measured depth beyond 65 m could wrap.  The minimum is one integer atomic per source pixel on an
 * order-preserving key of fl32(z3): the output does not depend on scheduling, equals harness/rgbd.py's register_depth bit for bit and, with
 * the defaults, the reference's files.  The clip is processed in chunks of frames of bounded device size.
 * ug_register_opts_default: the 7-Scenes calibration (depth focal 585, colour focal 525, the depth-to-colour transform of the Kinect calibration
 *   the reference cites, divisor 1000, max_valid 100), flags 0.
 * Errors (ug_last_error; the context stays usable; all are found on the host before anything is uploaded): NULL depth_u16 or out; T, H or
 *   W <= 0; T * H * W >= 2^31; a flag bit other than UG_REG_DROP_SENTINEL; a src_focal, dst_focal, divisor or max_valid that is not finite
 *   and positive; a non-finite entry of src2dst. */
typedef struct {
  double src_focal, dst_focal;   /* 585, 525 */
  double src2dst[12];            /* row-major 3x4 */
  float divisor, max_valid;      /* 1000, 100 */
  unsigned flags;
} ug_register_opts;
#define UG_REG_DROP_SENTINEL 1   /* raw == 65535 takes no part */
void ug_register_opts_default(ug_register_opts* o);
int ug_prep_register_depth(ug_ctx* ctx, const unsigned short* depth_u16 /* host [T,H,W] */, int T, int H, int W,
                           const ug_register_opts* opts /* NULL: defaults */, unsigned short* out /* host [T,H,W] */);

/* ScanNet++ mesh renderer on the device: depth, normals and the triangle index of a triangle mesh seen from T pinhole cameras - what the
 * reference makes offline, through pyrender, OpenGL and two GLSL shaders, in dataset/scannetpp/preprocess_scannetpp_imu.py:470-497 to write
 * the depth PNG and normal WebP files its loader reads.  ONE definition, evaluated identically here and by
 * harness/render.py's render_mesh.  fl32 / fl64 are ONE IEEE operation in that type, never contracted into an FMA; a*b - c*d is two products
 * and one difference; sums run in the order the brackets give.
 *   inputs   verts float32 [NV,3], widened to float64; faces int32 [NF,3]; per frame world2cam = (R | T), row-major 3x4 float64, OpenCV axes
 *            (x right, y down, z forward) and K = fx, fy, cx, cy in the convention in which pixel (col, row) looks along u = col + 0.5,
 *            v = row + 0.5 (what the script hands to pyrender's IntrinsicsCamera); H, W; znear, zfar.
 *   corners  p_i = R v_i + T per component as ((R_j0*x + R_j1*y) + R_j2*z) + T_j,  i = 0, 1, 2
 *   cross    c0 = p1 x p2, c1 = p2 x p0, c2 = p0 x p1, with (a x b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x): swapping the
 *            operands negates every component exactly, so the two triangles of a shared edge see edge values of exactly opposite sign
 *   det      D = (p0.x*c0.x + p0.y*c0.y) + p0.z*c0.z
 *   ray      r = (((col + 0.5) - cx) / fx, ((row + 0.5) - cy) / fy, 1)
 *   edges    e_k = (r.x*c_k.x + r.y*c_k.y) + c_k.z,  den = (e0 + e1) + e2
 *   covered  iff den != 0 and (e0 >= 0 and e1 >= 0 and e2 >= 0, or e0 <= 0 and e1 <= 0 and e2 <= 0) and, with z = D / den,
 *            z >= znear and z <= zfar - double-sided, as the script's MetallicRoughnessMaterial(doubleSided=True).  All comparisons in this
 *            positive form: a NaN drops out.  2-D homogeneous rasterisation: a triangle that crosses the camera plane needs no clipping, its
 *            mirror image behind the camera has z < 0.
 *   winner   per pixel the covered triangle of smallest fl32(z); equal fl32(z): the smaller triangle index (GL_LESS in draw order)
 *   skipped  a triangle whose world normal n = (v1 - v0) x (v2 - v0) has a squared length (n.x*n.x + n.y*n.y) + n.z*n.z that is not > 0 and finite
 *   depth    depth_mm = trunc(fl32(fl32(z) * 1000f)), 0 where no triangle covers the pixel; then 0 where mask < 255 (mask may be NULL)
 *   normal   n / sqrt((n.x*n.x + n.y*n.y) + n.z*n.z) of the winner, negated when D > 0 (it then faces the camera);
 *            q = floor(255 * (0.5 * n + 0.5) + 0.5);  m = (q / 255) * 2 - 1;  w_j = (R_j0*m.x + R_j1*m.y) + R_j2*m.z;  g = (w_0, -w_1, -w_2);
 *            normal = trunc(((g + 1) / 2) * 255) clamped to 0..255; (0, 0, 0) where no triangle covers the pixel.  The mask leaves it alone.
 *   index    tri_index = the winner, -1 where no triangle covers the pixel (optional)
 * Which pixels a triangle is tested at is an implementation matter (a conservative screen box when all three corners lie in front of the
 * camera, the whole frame otherwise); it never changes a result.  The minimum is ONE 64-bit integer atomicMin per covered pixel on
 * (order-preserving key of fl32(z) << 32) | triangle index: no floating-point atomic, equal bytes from run to run.  The mesh is uploaded once
 * per call, the frames are processed in chunks of bounded device size.
 * ug_render_opts_default: znear 0.05, zfar 20 (the script's), flags 0.
 * Errors (ug_last_error; the context stays usable; all are found on the host before anything is uploaded): NULL verts, faces, world2cam, K,
 *   depth_mm or normal; NV, NF, T, H or W <= 0; NF >= 2^31; T * H * W >= 2^31; a face index outside 0..NV-1; a non-finite vertex, pose or
 *   intrinsic; fx or fy <= 0; znear <= 0 or not finite; zfar <= znear; zfar > 65.535 (depth_mm is 16 bits of millimetres); any flag bit (none
 *   is defined yet). */
typedef struct {
  double znear, zfar;   /* 0.05, 20 */
  unsigned flags;       /* 0 */
} ug_render_opts;
void ug_render_opts_default(ug_render_opts* o);
int ug_prep_render_mesh(ug_ctx* ctx, const float* verts /* host [NV,3] */, long NV, const int* faces /* host [NF,3] */, long NF,
                        const double* world2cam /* host [T,12] */, const double* K /* host [T,4]: fx fy cx cy */, int T, int H, int W,
                        const unsigned char* mask /* NULL or host [T,H,W] */, const ug_render_opts* opts /* NULL: defaults */,
                        unsigned short* depth_mm /* host [T,H,W] */, unsigned char* normal /* host [T,H,W,3] */, int* tri_index /* NULL or host [T,H,W] */);

/* HIP-event profiling of everything launched between begin and end; end returns a JSON
 * object {kernel_family: {ms, calls, flops, bytes}} valid until the next call on ctx. */
int ug_profile_begin(ug_ctx* ctx);
const char* ug_profile_end(ug_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif

