/* libunigeo_hip.so - TEST / TUNING entry points (not part of the drop-in boundary).
 *
 * include/unigeo_hip.h is the product header: what INTEGRATION.md section 2 maps to the reference's model/ plugin surface.  The entry points
 * here exist for the parity tests (stage- and op-level calls, host in / host out), the A/B tools under tools/ and the profiling scripts;
 * a maintainer integrating the library does not need them.  Same conventions as unigeo_hip.h (int return, ug_last_error).
 */
#ifndef UNIGEO_HIP_TEST_H
#define UNIGEO_HIP_TEST_H
#include "unigeo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning / parity aids for the fused GEGLU feed-forward kernel of the narrow transformer blocks (kernels/ff_fused.hip; the reference's
 * FeedForward module inside the un-vendored UNet): ug_set_ff_fused(0) falls back to two GEMM launches; ug_op_ff evaluates
 * c0 * (GEGLU(X W1^T + b1) W2^T + b2) + c1 * R1 on [M, C] with either implementation (W1 [8C][C], b1 [8C], W2 [C][4C] in diffusers order). */
int ug_set_ff_fused(ug_ctx* ctx, int on);   /* bit 0: fused feed-forward kernel, bit 1: the block's LayerNorm inside it; default 3 */
/* The same block with its pre-norm (reference: BasicTransformerBlock.norm3 -> ff, TemporalBasicTransformerBlock.norm_in -> ff_in, inside
 * the un-vendored UNet): out = c0 * FF(LayerNorm(x') * gamma + beta) + c1 * x', x' = fp16(X + addvec[row / rows_per_vec]) (addvec NULL: x' = X).
 * mode 0: LayerNorm launch + two GEMMs, 1: LayerNorm launch + fused feed-forward, 2: all inside the fused kernel (product path at C <= 320). */
int ug_op_ln_ff(ug_ctx* ctx, const float* X, int M, int C, const float* gamma, const float* beta, float eps, const float* addvec, int rows_per_vec,
                const float* W1, const float* b1, const float* W2, const float* b2, float c0, float c1, int mode, float* out);
int ug_bench_flash(ug_ctx* ctx, int B, int H, int S, int variant, int iters, float* us_out);   /* flash-attention A/B on device-resident random data */
int ug_bench_ff(ug_ctx* ctx, int M, int C, int fused, int iters, float* us_out);
int ug_op_ff(ug_ctx* ctx, const float* X, int M, int C, const float* W1, const float* b1, const float* W2, const float* b2, const float* R1,
             float c0, float c1, int fused, float* out);
/* Every launch form of that feed-forward (tests/test_ff_forms_gpu.py): out = c0 * FF(xn) + c1 * r1 + c2 * R2, FF(xn) = GEGLU(xn W1^T + b1) W2^T + b2.
 *   operands : b2 may be NULL.  The residual r1: none (R1 NULL, r1_is_x 0), the stream itself (r1_is_x != 0, R1 NULL: the device pointer of X) or a
 *              separate tensor R1 [M,C]; R2 [M,C] may be NULL.  gamma NULL: no pre-norm, xn = X.  Else xn = fp16(LayerNorm(x') * gamma + beta) with
 *              x' = fp16(X + addvec[row / rows_per_vec]) (addvec NULL: x' = X), and with addvec the stream residual is x' as well; a separate R1 next
 *              to addvec is the launcher's refusal (an error).
 *   mode     : 0 / 1 / 2 as ug_op_ln_ff (LayerNorm launch + two GEMMs / LayerNorm launch + fused kernel / all in the fused kernel; without pre-norm 1
 *              and 2 are the same launch; mode 0 takes no R2).  3: the engine's own ln_ff, called as transformer_forward calls it on a Lin pair and a
 *              Norm built from these tensors (pre-norm and r1_is_x required): ug_set_ff_fused and M decide between the fused kernel, its in-kernel
 *              LayerNorm and the whole-rounds row split with its LayerNorm + two-GEMM tail.  The kernel variant is the context's (ug_tune_ff).
 *   max_wg   : FFusedP::max_wg, a cap on the fused kernel's grid (0 = the launcher's choice, the only value the product uses; modes 1 and 2 only): at
 *              small M one workgroup then walks several 128-row tiles, as every workgroup of the product's launches does.
 *   guards   : X, R1 and R2 hold M + in_guard rows and, with in_guard > 0, addvec one vector more than ceil(M / rows_per_vec); all of it goes to the
 *              device as given while the kernels are told M.  out_inout [M + out_guard, C] is uploaded as given and all of it comes back.
 *   info_out : [3] (may be NULL) = the grid of the fused launch, the largest number of tiles one of its workgroups walked, the rows it took (M in
 *              modes 1 and 2, the whole rounds M1 in mode 3); all 0 when no fused kernel ran. */
int ug_op_ff_ex(ug_ctx* ctx, const float* X, int M, int C, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* R1, int r1_is_x, const float* R2, float c0, float c1, float c2,
                const float* gamma, const float* beta, float eps, const float* addvec, int rows_per_vec,
                int mode, int max_wg, long in_guard, long out_guard, float* out_inout, int* info_out /*[3]*/);
/* Parity instrumentation (no reference counterpart; the reference would use the pipeline's callback_on_step_end): while
 * host_latents != NULL, ug_dc_run copies the latents after each of the first `steps` Euler steps to
 * host_latents[step][T][h][w][4] (float32, channels-last).  NULL switches it off.  Costs one host sync per step. */
int ug_dc_set_trace(ug_ctx* ctx, float* host_latents, int steps);
/* stage-level (parity tests): which = 0 YOSO pair / 1 refinement pair; use_ctrl: run the matching ControlNet on zimg (and DINO tokens) first */
int ug_sn_unet_forward(ug_ctx* ctx, int which, const float* sample_bchw, const float* zimg_bchw, int B, int h, int w, float t_unet,
                       float t_ctrl, const float* prompt_embeds, const float* dino_tokens, int use_ctrl, float* out_bchw);
int ug_sn_dino(ug_ctx* ctx, const float* images_bhwc, int B, int H, int W, float* tokens_out /*[B, g*g, D]*/);
int ug_sn_vae_decode(ug_ctx* ctx, const float* z_bchw, int B, int h, int w, float* out_bhwc /*[B,8h,8w,3] raw decoder output*/);
int ug_sn_vae_encode(ug_ctx* ctx, const float* img_m11_bhwc, int B, int H, int W, float* lat_out /*[B,4,H/8,W/8] posterior mode, unscaled*/);
/* Stage-level entry points (host in / host out) - what the parity tests drive.  Each replaces
 * the corresponding diffusers module call inside the pipeline (un-vendored). */
int ug_clip_embed(ug_ctx* ctx, const float* frames_thwc, int T, int H, int W, float* emb_out /*[T,proj]*/);
int ug_vae_encode(ug_ctx* ctx, const float* video_m11_thwc, int T, int H, int W, float* lat_out /*[T,4,H/8,W/8]*/);
int ug_vae_decode(ug_ctx* ctx, const float* z_tchw, int T, int h, int w, float* frames_out /*[T,8h,8w,3] in [0,1]*/);
int ug_unet_forward(ug_ctx* ctx, const float* sample_tchw /*[T,Cin,h,w]*/, int T, int h, int w, float timestep,
                    const float* clip_emb /*[T,cross]*/, float* out_tchw /*[T,Cout,h,w]*/);
/* ONE batched UNet pass over two arbitrary videos stacked [2][T] (what ug_dc_run runs per step under classifier-free guidance, without the
 * combine): samples [T,Cin,h,w], embeddings [T,cross], outputs [T,Cout,h,w].  The guided pass is b = the same latents with zero conditioning
 * channels and emb_b = 0.  Frame-mixing operators stay inside each video (tests/test_cfg_gpu.py). */
int ug_unet_forward_pair(ug_ctx* ctx, const float* sample_a, const float* emb_a, const float* sample_b, const float* emb_b, int T, int h, int w,
                         float timestep, float* out_a, float* out_b);
/* Op-level entry points for kernel parity tests (row-major host matrices, fp32 in/out, computed in fp16). */
int ug_op_linear(ug_ctx* ctx, const float* A, int M, int K, const float* W, int N, const float* bias,
                 const float* R1, float c0, float c1, int act, int geglu, float* out);
/* MX-fp8 linear: A [M,K], W [N,K] are quantised on device (kernels/mx8.hip) and multiplied on the fp8 matrix cores; optional outputs:
 * the quantised A bytes [M,K] and its scale dwords [K/128][round_up(M,256)] (4 e8m0 per dword) for bit-level checks. */
int ug_op_linear_mx8(ug_ctx* ctx, const float* A, int M, int K, const float* W, int N, const float* bias, int geglu, float* out,
                     unsigned char* a8_out, unsigned* scales_out);
/* The MX-fp8 path launch by launch (tests/test_mx8_forms_gpu.py), with the conventions of the other _ex entries: every *_inout
 * buffer goes to the device as the caller gives it and comes back whole.  A bad call returns an error and leaves the context usable.
 *   ug_op_quant_mx8_ex : launch_quant_mx8 alone.  x [M + guard, ldx] (fp16-representable), q_inout [M + guard, K] bytes, s_inout [K/128][ld_s] dwords with
 *                        the caller's ld_s >= M; the bytes of the guard rows and the dwords of rows >= M return unchanged.  K % 128 == 0, ldx % 8 == 0.
 *   ug_op_linear_mx8_ex: both quantiser launches, then launch_gemm_mx8 with the whole epilogue: out = act(c0 * f(A W^T + bias) + c1 * R1 + c2 * R2), f = GEGLU
 *                        with geglu != 0 (N % 128 == 0; W / bias in checkpoint order, packed to the bound row order here).  R1 [M, ldr1], R2 [M, ldr2] (may be
 *                        NULL), out_inout [M + guard, ldo]; scale areas of round_up(M,256) / round_up(N,256) rows as the engine sizes them.  poison != 0:
 *                        the quantised bytes, both scale areas and the rest of the workspace are filled with 0xFF (e8m0 NaN) before the quantiser launches
 *                        and nothing is zeroed, so the scale rows >= M / >= N hold what a product launch may find there.  Honours ug_tune_force(100 + pick);
 *                        plan_out [2] (may be NULL) = (tile pick, group_m) as launched.  a8_out / sa_out as ug_op_linear_mx8, which is this entry with
 *                        tight rows and no residual (the dwords of rows >= M are then unspecified).
 *   ug_op_linear_engine: a Lin of W [N,K] and bias goes through the engine's quant_lin() and linear() with lda (>= K), ldo and an Epi of R1, c1, R2, c2, c0,
 *                        act and the GEGLU flag, over a 0xFF-filled workspace; the caller sets the context's fp8_linears (ug_set_fp8_linears).  gamma / beta
 *                        [K] given (lda == K): ln_linear() of LayerNorm(A) with a QAct from qact_alloc() - the pre-quantised hand-off; with epilogue operands
 *                        the LayerNorm launch and linear() on that QAct, as the engine's feed-forward sends its GEGLU projection.
 *                        info_out [3] (may be NULL): the Lin got an MX-fp8 weight, the MX GEMM ran (else the fp16 one), the LayerNorm wrote the QAct.
 *                        What quant_lin() took from the persistent arena is released before the entry returns. */
int ug_op_quant_mx8_ex(ug_ctx* ctx, const float* x, int M, int K, long ldx, long guard, long ld_s, unsigned char* q_inout, unsigned* s_inout);
int ug_op_linear_mx8_ex(ug_ctx* ctx, const float* A, int M, int K, const float* W, int N, const float* bias, const float* R1, long ldr1, const float* R2, long ldr2,
                        float c0, float c1, float c2, int act, int geglu, long ldo, long guard, int poison, float* out_inout,
                        unsigned char* a8_out, unsigned* sa_out, int* plan_out /*[2]*/);
int ug_op_linear_engine(ug_ctx* ctx, const float* A, int M, long lda, const float* W, int N, int K, const float* bias, const float* gamma, const float* beta, float eps,
                        const float* R1, long ldr1, const float* R2, long ldr2, float c0, float c1, float c2, int act, int geglu, long ldo, long guard,
                        float* out_inout, int* info_out /*[3]*/);
int ug_op_conv(ug_ctx* ctx, const float* x0_thwc, int C0, const float* x1_thwc, int C1, int T, int H, int W,
               const float* weight /*[O][I][kt][ky][kx]*/, const float* bias, int O, int kt, int k, int stride,
               int pad_t, int pad_l, int ups, float* out_thwc);
/* convolution (k x k pad k/2, or (kt,1,1)) + residual, then GroupNorm + SiLU of its output with the statistics (a) from a pass over the stored tensor,
 * (b) from the convolution's epilogue (GemmP::stat_part); *rb_out = rows per statistics block (0: the planner's kernel has no statistics epilogue) */
int ug_op_conv_gn(ug_ctx* ctx, const float* x_thwc, int C0, int T, int H, int W, const float* weight, const float* bias, const float* res, int O, int kt, int k,
                  int G, float eps, int temporal, const float* gamma, const float* beta, float* conv_out, float* y_pass, float* y_epi, int* rb_out);
int ug_op_groupnorm(ug_ctx* ctx, const float* x0, int C0, const float* x1, int C1, int T, int HW, int G, float eps,
                    int temporal, int silu, const float* gamma, const float* beta, float* out);
int ug_op_layernorm(ug_ctx* ctx, const float* x, int M, int C, float eps, const float* gamma, const float* beta,
                    const float* addvec, int rows_per_vec, float* out, float* xout);
/* The launch forms of kernels/norm.hip that the two entries above leave to the launcher's heuristics (tests/test_norm_forms_gpu.py).
 *   ug_op_groupnorm_ex: mode -> GroupNormP::mode (0 = the launcher picks; 1 / 2 / 4 / 6 force a scheme, which the launcher may still replace when the
 *     tensor cannot take it).  out_inout [T*HW + guard, C0+C1]: with guard > 0 all of it is uploaded as the caller gives it, and all of it comes back -
 *     the guard rows must return unchanged.  plan_out [4] (may be NULL): the scheme launched, the slab kernel's threads and register vectors VMAX
 *     (0, 0 unless scheme 4 / 6), chunks per frame (0 unless scheme 1).
 *   ug_op_layernorm_ex: row0 -> LayerNormP::row0 (addvec then holds ceil((M + row0) / rows_per_vec) vectors); form 0 = the launcher picks, 1 = the
 *     one-wave-per-row kernel also at C = 320 / 640 / 1280; out_inout [M + guard, C] as above; *form_out (may be NULL) = L (8 / 16 / 32) when
 *     ln40_kernel<L> ran, -VPL (-1 .. -4) when ln_kernel<VPL> ran.  y8_out [M][C] with s8_out [C/128][round_up(M,256)] (both or neither; C % 128 == 0):
 *     the same launch once more with the MX-fp8 output pair - e4m3 bytes and scale dwords in ug_op_linear_mx8's layout, zeroed before the launch. */
int ug_op_groupnorm_ex(ug_ctx* ctx, const float* x0, int C0, const float* x1, int C1, int T, int HW, int G, float eps,
                       int temporal, int silu, const float* gamma, const float* beta, int mode, long guard, float* out_inout, int* plan_out /*[4]*/);
int ug_op_layernorm_ex(ug_ctx* ctx, const float* x, int M, int C, float eps, const float* gamma, const float* beta,
                       const float* addvec, int rows_per_vec, long row0, int form, long guard, float* out_inout, float* xout,
                       unsigned char* y8_out, unsigned* s8_out, int* form_out);
int ug_op_flash_attn(ug_ctx* ctx, const float* qkv /*[B*S,3*H*64]*/, int B, int H, int S, float* out /*[B*S,H*64]*/);
int ug_op_temporal_attn(ug_ctx* ctx, const float* qkv /*[T*HW,3*H*64]*/, int T, int HW, int H, float* out);
/* The other launch forms of the d = 64 flash attention (the cross-attention of the StableNormal transformer blocks): Sk keys per batch (0: self-attention,
 * kv holds B*S rows), kv_shared = 1: one context of Sk rows read by every batch.  q [B*S, ldq]; kv [(kv_shared ? 1 : B)*Sk + guard, ldkv] with K in
 * columns [0, H*64) and V in [H*64, 2*H*64); out_inout [B*S + guard, ldo].  All three go to the device as given - guard rows, surplus columns and the
 * caller's contents of out_inout included - and all of out_inout comes back.  ldq, ldkv % 8 == 0, ldo % 4 == 0 (the launcher's rules), else an error. */
int ug_op_flash_cross_attn(ug_ctx* ctx, const float* q, const float* kv, int B, int H, int S, int Sk, int kv_shared, long ldq, long ldkv, long ldo,
                           long guard, float* out_inout);
/* ug_op_temporal_attn over nv videos stacked [nv][T][HW] in one launch (the guided UNet pass): qkv [nv*T*HW,3*H*64], out [nv*T*HW,H*64] */
int ug_op_temporal_attn_nv(ug_ctx* ctx, const float* qkv, int nv, int T, int HW, int H, float* out);
int ug_op_attention_generic(ug_ctx* ctx, const float* qkv /*[B*S,3*H*d]*/, int B, int S, int H, int d, float* out);
int ug_op_flash_attn_dh(ug_ctx* ctx, const float* qkv /*[B*S,3*H*d]*/, int B, int S, int H, int d, float* out);   /* fused self-attention, head dim d in {32,48,80,96,112,128}: the CLIP tower's 16 x 80 heads */
/* The same two paths with the conventions of ug_op_flash_cross_attn (tests/test_attn_general_gpu.py): qkv [B*S + guard, ld] with
 * Q | K | V in columns [0, 3*H*d), out_inout [B*S + guard, ldo]; both go to the device as given - guard rows, surplus columns and the caller's contents of
 * out_inout included - and all of out_inout comes back.  ld >= 3*H*d, ldo >= H*d, ld % 8 == 0, ldo % 4 == 0, a supported d, else an error that leaves
 * the context usable.  ug_op_flash_attn_dh_ex calls launch_flash_attn_dh; ug_op_attention_generic_ex the four launches of the engine's
 * unfused_attention (d % 8 == 0), plan_out [4] (may be NULL) = the planner's (tile config, split factor) of the Q K^T and of the P V batched GEMM.
 * The two entries above are these with tight buffers (ld = 3*H*d, ldo = H*d, no guard). */
int ug_op_flash_attn_dh_ex(ug_ctx* ctx, const float* qkv, int B, int S, int H, int d, long ld, long ldo, long guard, float* out_inout);
int ug_op_attention_generic_ex(ug_ctx* ctx, const float* qkv, int B, int S, int H, int d, long ld, long ldo, long guard, float* out_inout, int* plan_out /*[4]*/);
/* One batched GEMM through the engine's run_gemm with exactly the fields unfused_attention fills: Out[b] = c0 * A[b] W[b]^T for b < batch, no bias;
 * batch b = (bo, bi) = (b / nb_inner, b % nb_inner) sits at element offset bo * s?_o + bi * s?_i of its buffer.  A [M,K] rows of lda and W [N,K] rows
 * of ldw are fp16 on the device (a_elems / w_elems floats on the host); the output [M,N] rows of ldo is float32 (out_f32 != 0: UG_F_OUT_F32) or fp16.
 * out_inout holds o_elems floats, goes to the device as given and comes back whole.  The entry checks on the host that the last element every batch
 * addresses lies inside the three buffers (else an error) and honours ug_tune_force as run_gemm does; plan_out [2] (may be NULL) = the (tile config,
 * split factor) launched. */
int ug_op_gemm_batched(ug_ctx* ctx, const float* A, long lda, long sA_o, long sA_i, const float* W, long ldw, long sW_o, long sW_i, int M, int N, int K,
                       int batch, int nb_inner, float c0, int out_f32, long ldo, long sO_o, long sO_i, long a_elems, long w_elems, long o_elems,
                       float* out_inout, int* plan_out /*[2]*/);
int ug_op_euler_step(ug_ctx* ctx, const float* v, float* latents_inout, long n, float sigma, float sigma_next);
/* The pipeline glue of kernels/misc.hip one launch at a time (tests/test_glue_gpu.py).  Each entry calls the product's own
 * launcher on the context's stream and nothing else.  Host in / host out in float32; what the device holds as fp16 is rounded on the way in (the tests
 * pass fp16-representable values) and widened on the way out.  Every *_inout buffer has `guard` extra rows (or elements), goes to the device as the
 * caller gives it and comes back whole: the guard, and whatever else the kernel must not write, returns unchanged.
 *   ug_op_clip_patchify   : video_m11 [T,H,W,3] -> out_inout [T*(S/P)^2 + guard, Kpad]: pre-blur, bicubic resample to S x S, CLIP (imagenet_norm = 0) or
 *                           ImageNet mean / std, patch column c*P*P + py*P + px; columns [3*P*P, Kpad) are not written
 *   ug_op_prep_video      : frames [T,H,W,3] and noise [T,3,H,W], both float32 on the device -> clip_src_inout [T*H*W + guard, 3], vae_in_inout [.. , 8]
 *   ug_op_init_latents    : noise [T,4,hw] float32 on the device -> lat_inout [T*hw + guard, 4] = fp16(fp16(noise) * sigma0)
 *   ug_op_unet_input      : lat, cond [pixels,4] -> x_inout [pixels + guard, 8] = (lat / den | cond); guided != 0: [2*pixels + guard, 8], the second
 *                           video (lat / den | 0) stacked under the first (launch_make_unet_input_cfg)
 *   ug_op_euler_step_cfg  : the guided step on v_u + g (v_c - v_u); lat_inout [n + guard]
 *   ug_op_window_blend    : the two overlap launches of the latent sliding windows over n = overlap * frame_elems elements.  renoised_inout [n + guard]
 *                           holds the window's noise on entry and returns prev + coef * noise (launch_axpby_f16, in place as the engine calls it);
 *                           faded_inout [n + guard] holds the running result on entry and returns the cross-fade with cur (launch_crossfade_f16)
 *   ug_op_time_conv_out   : x [T,HW,Cs] (Cs >= 3, channels 3.. ignored), w [3 out][3 in][3 taps], b [3] -> out_inout [T*HW + guard, 3] float32
 *   ug_op_depth_post      : frames [n,3] float32 -> depth_inout [n + guard] (launch_depth_post), disp_inout [n + guard] (launch_disparity_from_frames on
 *                           the min-max words that launch left), minmax_out [2] = those words decoded to float (min, max)
 *   ug_op_add_grid_nearest: x_inout [B*h*w + guard, C] += grid [B,g,g,C] at (y*g/h, x*g/w); C % 8 == 0
 *   ug_op_sn_normals_out  : dec [pixels, ldd] (columns 3.. ignored) -> out_inout [pixels + guard, 3] float32, clipped to [-1,1] and normalised
 *   ug_op_clip_assemble   : patches [T*np, d], cls [d], pos [np+1, d] -> tok_inout [T*(np+1) + guard, d] */
int ug_op_clip_patchify(ug_ctx* ctx, const float* video_m11, int T, int H, int W, int S, int P, int Kpad, int imagenet_norm, long guard, float* out_inout);
int ug_op_prep_video(ug_ctx* ctx, const float* frames, const float* noise, int T, int H, int W, float aug, long guard, float* clip_src_inout, float* vae_in_inout);
int ug_op_init_latents(ug_ctx* ctx, const float* noise_tchw, int T, long hw, float sigma0, long guard, float* lat_inout);
int ug_op_unet_input(ug_ctx* ctx, const float* lat, const float* cond, long pixels, float den, int guided, long guard, float* x_inout);
int ug_op_euler_step_cfg(ug_ctx* ctx, const float* vc, const float* vu, float g, long n, float sigma, float sigma_next, long guard, float* lat_inout);
int ug_op_window_blend(ug_ctx* ctx, const float* prev, const float* cur, long frame_elems, int overlap, float coef, long guard,
                       float* renoised_inout, float* faded_inout);
int ug_op_time_conv_out(ug_ctx* ctx, const float* x, const float* w, const float* b, int T, long HW, int Cs, long guard, float* out_inout);
int ug_op_depth_post(ug_ctx* ctx, const float* frames, long n, long guard, float* depth_inout, float* disp_inout, float* minmax_out /*[2]*/);
int ug_op_add_grid_nearest(ug_ctx* ctx, const float* grid, int B, int h, int w, int g, int C, long guard, float* x_inout);
int ug_op_sn_normals_out(ug_ctx* ctx, const float* dec, int ldd, long pixels, long guard, float* out_inout);
int ug_op_clip_assemble(ug_ctx* ctx, const float* patches, const float* cls, const float* pos, int T, int np, int d, long guard, float* tok_inout);
/* The float32-grade VAE encoder's kernels op by op (kernels/wide.hip and the engine's pair convolution / attention; the reference runs the encoder in
 * float32 under force_upcast, inside the un-vendored AutoencoderKL).  float32 in and out, no rounding of the inputs to fp16 (weights, bias, gamma and
 * beta are bound as fp16, as the checkpoint stores them).
 *   ug_op_split_pair: x [M,C] -> hi = fp16(x), lo = fp16(x - hi), both widened to float32 [M,C]
 *   ug_op_gn32_pair : GroupNorm (+ SiLU) of x [T,HW,C] in float32, split into its pair
 *   ug_op_conv_wide : the weight [O][C][k][k] bound and K-doubled exactly as the encoder's convolutions are, x [T,H,W,C] split and convolved with float32
 *                     output [T,H/stride,W/stride,O]; res (may be NULL): float32 residual added in the epilogue - res_in_place: it is first copied
 *                     into the output buffer and read from there (the aliasing of a residual block with a shortcut convolution)
 *   ug_op_attn_wide : qkv [T*S,3C] -> softmax(q k^T / sqrt(C)) v per frame [T*S,C], the three-term products of the mid-block attention */
int ug_op_split_pair(ug_ctx* ctx, const float* x, long M, int C, float* hi, float* lo);
int ug_op_gn32_pair(ug_ctx* ctx, const float* x, int T, int HW, int C, int G, float eps, int silu, const float* gamma, const float* beta, float* hi, float* lo);
int ug_op_conv_wide(ug_ctx* ctx, const float* x_thwc, int T, int H, int W, int C, const float* weight, const float* bias, int O, const float* res, int res_in_place,
                    int k, int stride, int pad_t, int pad_l, float* out_thwc);
int ug_op_attn_wide(ug_ctx* ctx, const float* qkv, int T, int S, int C, float* out);
/* One convolution through the product's own path (tests/test_conv_bound_gpu.py): the checkpoint-layout weight [O][cin][k][k] (kt == 1) or [O][cin][3][1][1]
 * (kt == 3, k == 1) and the optional bias are bound on the device by the engine's bind_conv - upsampler != 0 as the models' upsamplers are bound, with the
 * sub-pixel phase weights - and launched by the engine's conv().  ug_op_conv packs its weights on the host instead.
 *   ug_op_bind_conv : the bound tensors, fp16 widened to float: w_out [O * kt*k*k * cinp]; wphase_out [4 * O * 4 * cinp] (may be NULL; written only if phase
 *                     weights were bound); info_out [3] = cinp (cin rounded up to 8), the chunk-major flag (Conv::kchunk), 1 if phase weights were bound.
 *   ug_op_conv_bound: x0 [T,H,W,C0] and x1 [T,H,W,C1] (may be NULL, C1 = 0) with C0 + C1 == cin; with cin % 8 != 0 one source of cin channels, which is
 *                     padded with zero channels on the device.  ups == 2 with upsampler != 0, stride 1 and pads (1, 1): four 2x2 phase launches that scatter
 *                     to the output parities; every other form: one launch, with the optional residual R1 [rows, O]: out = act(c0 * (conv + bias) + c1 * R1).
 *                     out_inout [rows + guard, ldo], rows = T * (H*ups/stride) * (W*ups/stride), ldo >= O: uploaded as the caller gives it and all of it
 *                     comes back - guard rows, surplus columns and pixels no launch wrote return unchanged.  plan_out [9] (may be NULL): the number of GEMM
 *                     launches (1 or 4), then the planner's (tile config, split factor) of each in launch order, -1 where there was none. */
int ug_op_bind_conv(ug_ctx* ctx, const float* weight, const float* bias, int cin, int O, int kt, int k, int upsampler,
                    float* w_out, float* wphase_out, int* info_out /*[3]*/);
int ug_op_conv_bound(ug_ctx* ctx, const float* weight, const float* bias, int cin, int O, int kt, int k, int upsampler,
                     const float* x0_thwc, int C0, const float* x1_thwc, int C1, int T, int H, int W, int stride, int pad_t, int pad_l, int ups,
                     const float* R1, float c0, float c1, int act, long ldo, long guard, float* out_inout, int* plan_out /*[9]*/);
/* The epilogue operands of the graphs on every GEMM kernel family (tests/test_epilogue_forms_gpu.py):
 *     out = act(c0 * f(acc + bias + bias2) + c1 * R1 + c2 * R2),  f = GEGLU or the identity
 * through the engine's linear() / conv(), honouring ug_tune_force.  bias, bias2, R1, R2 may be NULL.  out_inout [rows + guard, ldo] goes to the device as
 * given and comes back whole.  plan_out [2] (may be NULL) = the tile config launch_gemm launched (the planner's or the forced one; 70 - 73 / 80 where the
 * halo-staged / streaming kernel took the launch, 60 for the row-split pair) and the split factor.  A bad call returns an error and leaves the context usable.
 *   ug_op_linear_ex: the fp16 path of linear(); refuses a context with fp8_linears set.  A [M, lda] (lda >= K, lda % 8 == 0), W [N, K], bias / bias2 [N],
 *                    R1 [M, ldr1], R2 [M, ldr2], out_inout [M + guard, ldo]; the output width is N, with geglu != 0 N / 2 (N % 128 == 0; W, bias and bias2
 *                    in checkpoint order [values | gates], packed into the bound row order here).
 *   ug_op_conv_epi : the checkpoint-layout weight bound by bind_conv and launched by conv(), as ug_op_conv_bound (no upsampling forms): one or two sources,
 *                    kt in {1, 3}, stride 1 / 2; bias2 [O], R1 [rows, ldr1], R2 [rows, ldr2], rows = T * (H / stride) * (W / stride).  want_stats != 0: the
 *                    launch is handed a StatPart of ceil(rows / 48) * O float2 (the size stat_alloc gives it): stat_inout (2 floats per float2) is uploaded
 *                    bit for bit, downloaded whole, and *rb_out = rows per statistics block, 0 when the launch declined (it then wrote nothing there). */
int ug_op_linear_ex(ug_ctx* ctx, const float* A, int M, long lda, const float* W, int N, int K, const float* bias, const float* bias2,
                    const float* R1, long ldr1, const float* R2, long ldr2, float c0, float c1, float c2, int act, int geglu,
                    long ldo, long guard, float* out_inout, int* plan_out /*[2]*/);
int ug_op_conv_epi(ug_ctx* ctx, const float* weight, const float* bias, int cin, int O, int kt, int k,
                   const float* x0_thwc, int C0, const float* x1_thwc, int C1, int T, int H, int W, int stride, int pad_t, int pad_l,
                   const float* bias2, const float* R1, long ldr1, const float* R2, long ldr2, float c0, float c1, float c2, int act,
                   long ldo, long guard, float* out_inout, int want_stats, float* stat_inout, int* rb_out, int* plan_out /*[2]*/);
/* Clip inputs made on the device (kernels/noise.hip; behind ug_dc_set_inputs_ex of the product header).
 *   ug_op_philox_u32  : Philox4x32-10 words of blocks block_offset .. block_offset + nblocks - 1 for key = seed (lo, hi) and counter
 *                       (q lo, q hi, stream, 0) -> out [nblocks][4] uint32 (the generator against the published known-answer vectors)
 *   ug_op_randn       : standard normal numbers element_offset .. element_offset + n - 1 of (seed, stream).  inout holds n + guard floats: all of
 *                       it is uploaded, the kernel writes the first n, all of it is downloaded - the guard words come back as they went in
 *   ug_op_u8_to_frames: uint8 planar [T,3,H,W] -> float32 [T,H,W,3] = x / 255, bit-identical to DepthCrafter.prepare_input (H * W % 4 == 0) */
int ug_op_philox_u32(ug_ctx* ctx, uint64_t seed, uint32_t stream, uint64_t block_offset, long nblocks, uint32_t* out);
int ug_op_randn(ug_ctx* ctx, uint64_t seed, uint32_t stream, uint64_t element_offset, long n, long guard, float* inout);
int ug_op_u8_to_frames(ug_ctx* ctx, const unsigned char* frames_tchw, int T, int H, int W, float* out_thwc);
/* The exact masked selection behind UG_ALIGN_MEDIAN alone (kernels/metrics.hip): out_medians = the lower medians (element (count - 1) / 2 of the
 * sorted values) of clamp(pred, pre_clip_min, pre_clip_max) and of gt over gt > 0 (and gt < max_depth; <= 0 or NaN: off), *out_count = how many
 * pixels that is.  NaN clip bounds are off.  count = 0 leaves the medians 0. */
int ug_op_masked_median(ug_ctx* ctx, const float* pred, const float* gt, long n, float max_depth, float pre_clip_min, float pre_clip_max,
                        float* out_medians /*[2]*/, long* out_count);
/* The exact L1 scale-and-shift fit behind UG_ALIGN_L1 alone (kernels/metrics.hip; the definition stands with UG_ALIGN_L1 in
 * unigeo_hip.h): opts gives max_depth and the pre-clip bounds, the other fields are not read.  out_st = (s, t) in double, before the rounding to
 * float32; out_info = j, k, steps, certified as ug_eval_depth_l1_info.  No valid pixel: (0, 0) and j = k = -1; every q equal: k = -1, steps = 0. */
int ug_op_l1_fit(ug_ctx* ctx, const float* pred /* NULL: resident depth */, const float* gt, long n, const ug_depth_eval_opts* opts,
                 double* out_st /*[2]*/, long* out_info /*[4]*/);
/* The kernels behind ug_eval_pcd one by one (kernels/pcd.hip).
 *   ug_op_pcd_nn         : nearest target of every query, float64 [n,3] each, the query first moved by T44 (row-major 4x4, may be NULL) as
 *                          ((r0 x + r1 y) + r2 z) + t -> idx_out [nq], dist_out [nq] = sqrt of the smallest (dx*dx + dy*dy) + dz*dz, ties to the
 *                          lowest index; unfused float64
 *   ug_op_pcd_select     : the exact k-th smallest (k from 0) of n float32 (is_f64 = 0) or float64 (is_f64 = 1) values -> *out of that type;
 *                          -0.0 sorts below +0.0; no NaN
 *   ug_op_pcd_knn_normals: per point of a float64 cloud [n,3] the min(knn, n) nearest points, itself included, ordered by (squared distance,
 *                          index) -> nbr_out [n, min(knn, n)] (may be NULL), and the unit eigenvector of the smallest eigenvalue of their float64
 *                          covariance -> normals_out [n,3]; (0, 0, 1) for n < 3
 *   ug_op_pcd_fps        : farthest-point sampling of a float32 cloud [n,3] alone -> idx_out [k] in pick order and
 *                          sel_dist_out [k] = the squared distance to the points picked before (+inf for the first; -1 for a non-finite point, picked
 *                          only when no finite one exists); 1 <= k <= n < 2^31, else an error that leaves the context usable */
int ug_op_pcd_nn(ug_ctx* ctx, const double* query, long nq, const double* target, long nt, const double* T44, int* idx_out, double* dist_out);
int ug_op_pcd_select(ug_ctx* ctx, const void* values, int is_f64, long n, long k, void* out);
int ug_op_pcd_knn_normals(ug_ctx* ctx, const double* pts, long n, int knn, int* nbr_out, double* normals_out);
int ug_op_pcd_fps(ug_ctx* ctx, const float* pts, long n, long k, long* idx_out, float* sel_dist_out);
/* The same two searches through a uniform grid over the target cloud: arguments and outputs as ug_op_pcd_nn /
 * ug_op_pcd_knn_normals, and the same bytes.  Queries the grid cannot settle within PCD_GRID_RINGS rings of cells (far from every target, a
 * non-finite query, an empty grid) are finished by the brute-force kernels; the 2^40 pair cap counts those leftovers times the target size.
 * stats (host, [4], may be NULL): queries settled by the grid, leftover queries, cells of the grid, points in its fullest cell. */
int ug_op_pcd_nn_grid(ug_ctx* ctx, const double* query, long nq, const double* target, long nt, const double* T44, int* idx_out, double* dist_out,
                      long* stats /* [4] or NULL */);
int ug_op_pcd_knn_normals_grid(ug_ctx* ctx, const double* pts, long n, int knn, int* nbr_out, double* normals_out, long* stats /* [4] or NULL */);
/* The voxel set of ug_eval_pcd_scores alone (kernels/voxel.hip) on two host float64 clouds [na,3] / [nb,3] (either may be
 * empty) -> out6: cells of a, cells of b, cells of both, cells of either, skipped points of a, skipped points of b.  capacity_log2 forces the
 * table to 2^capacity_log2 slots (1..30) so that probing, wrap-around and a full table can be reached with a few thousand points; 0 takes the
 * production rule (the smallest power of two >= 2 * (na + nb), at least 1024).  A table too small for the cells is an error return ("overflow"),
 * never a wait, and the context stays usable. */
int ug_op_voxel_set(ug_ctx* ctx, const double* a, long na, const double* b, long nb, double voxel_size, int capacity_log2, long* out6);
/* Tuning aids (not on the product path): GEMM / implicit-conv microbenchmark on device-resident random data,
 * and an override of the tile/split-K heuristic (-1 = heuristic). ms_out: [ms per launch, cfg, split, M, K]. */
/* GroupNorm launch-scheme A/B (mode: launch_groupnorm in kernels/norm.hip); tuning aid, no reference counterpart. */
int ug_bench_groupnorm(ug_ctx* ctx, int C0, int C1, int T, int HW, int temporal, int mode, int iters, float* us_out);
int ug_bench_gemm(ug_ctx* ctx, int M, int N, int K, int conv, int T, int Hi, int Wi, int C0, int C1, int kt, int k,
                  int stride, int ups, int cfg, int split, int iters, float* ms_out);
/* calibration: chip-wide fp16 MFMA rate with operands in registers (16x16x32 f16, 256 workgroups x 8 waves), TFLOP/s - the matrix-pipe
 * ceiling at the clock the power management allows under a pure matrix load (bench.py reports it next to the 2.5 PFLOP/s spec peak) */
int ug_bench_mfma_peak(ug_ctx* ctx, int iters, float* tflops_out);
int ug_tune_force(ug_ctx* ctx, int cfg, int split);   /* test / A-B aid, per context: force a GEMM tile config (cfg >= 0) and split-K factor for this context's launches, (-1, -1) = planner; cfg = -100 - mask sets the knob mask (kernels/gemm.hip) */
int ug_tune_ff(ug_ctx* ctx, int variant);      /* A/B aid, per context: fused feed-forward kernel variant, 0 = cross-tile prefetch (default), 1 = without it; bit-identical outputs */
int ug_tune_flash(ug_ctx* ctx, int variant);   /* test aid, per context: flash-attention variant mask of this context's launches (bit 0: one softmax step per 64 keys, bit 1: XCD-grouped workgroup order, bit 2: 2-slot ring + 4 workgroups per CU, bit 4: lazy rescale + dot2 row sums, bit 6: 8-wave ping-pong kernel; -1 = default 23) */
int ug_profile_begin_shapes(ug_ctx* ctx);   /* same, keyed by kernel family AND problem shape */

#ifdef __cplusplus
}
#endif
#endif
