// Shared declarations for the gfx950 (MI355X / CDNA4) DepthCrafter engine.
// Layout convention everywhere: activations are channels-last fp16, i.e. a [T,H,W,C] video
// tensor is the row-major matrix [M = T*H*W, C]; weights are [N][K] row-major ("B^T").
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdexcept>
#include <string>

typedef _Float16 f16;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define UG_CHECK(expr)                                                                        \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      throw std::runtime_error(std::string(#expr) + " failed: " + hipGetErrorString(_e) +    \
                               " at " + __FILE__ + ":" + std::to_string(__LINE__));           \
  } while (0)

#define UG_REQUIRE(cond, msg)                                                                 \
  do {                                                                                        \
    if (!(cond))                                                                              \
      throw std::runtime_error(std::string("requirement failed: ") + #cond + " : " + (msg) + \
                               " at " + __FILE__ + ":" + std::to_string(__LINE__));           \
  } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
// hipFuncSetAttribute is per device: the "already raised the dynamic-LDS limit" caches are indexed by the current device
static inline int ug_dev_slot() { int d = 0; (void)hipGetDevice(&d); return d & 31; }

// ---------------------------------------------------------------------------------------
// GEMM / implicit-GEMM convolution  (kernels/gemm.hip)
//   Out[m,n] = act( c0 * f(acc[m,n] + bias[n] + bias2[n]) + c1*R1[m,n] + c2*R2[m,n] )
//   acc = sum_k A(m,k) * W[n,k];  A is either a dense row-major matrix or the implicit
//   im2col view of one/two channels-last tensors (3x3 / 1x1 / (3,1,1) taps, stride 1|2,
//   optional nearest-2x upsample of the source, optional channel concat of two sources).
// ---------------------------------------------------------------------------------------
enum { UG_ACT_NONE = 0, UG_ACT_SILU = 1, UG_ACT_GELU = 2 };
enum { UG_F_GEGLU = 1, UG_F_OUT_F32 = 2, UG_F_NOXCD = 4, UG_F_PRIO = 8 /* tuning knob: static priority for the younger half of an 8-wave workgroup */,
       UG_F_XCDROUND = 32 /* tuning knob 128: the round-strided XCD tile walk of rounds 1 - 4 (kernels/gemm_common.h: tile_walk) */,
       UG_F_R1_F32 = 16 /* R1 points at float32 (ldr1 in floats): the residual stream of the float32-grade VAE encoder, added in the epilogue instead of by a separate pass */ };

struct GemmP {
  const f16* A0; const f16* A1;
  int C0, C1;            // conv: channels of the two sources; dense: C0 = row stride (lda), C1 = 0
  int M, N, K;
  int conv;              // 0 dense, 1 implicit conv
  int T, Hi, Wi, Ho, Wo; // conv: frames, source dims (pre-upsample), output dims
  int ups, stride, pad_t, pad_l;
  int kt, ky, kx;        // taps along time / y / x
  const f16* W; long ldw;
  const f16* bias; const f16* bias2;
  const f16* R1; long ldr1; float c1;
  const f16* R2; long ldr2; float c2;
  float c0;
  void* Out; long ldo;
  int act, flags;
  const f16* zero;       // >=16 B of zeros in global memory (source for padded / OOB loads)
  int nb_inner;          // batch = gridDim.z = nb_outer * nb_inner
  long sA_o, sA_i, sW_o, sW_i, sO_o, sO_i;
  int cfg_p1;            // 0 = pick the tile config automatically, else tile config id + 1
  int splitk;            // 0 = automatic, 1 = off, >1 = K slices (needs `partial`)
  float* partial;        // split-K scratch: splitk * M * N floats
  void* trace;           // UG_GEMM_TRACE builds only: cycle-stamp dump (tools/gemm_trace.py)
  int up_phase;          // 0 = off; 1 + (a*2+b): conv output row (t,y,x) is stored at row (t, 2y+a, 2x+b) of a 2Ho x 2Wo grid
  // MX-fp8 dense path (launch_gemm_mx8): A0 / W point at OCP e4m3 bytes ([M][K] / [N][K], K % 128 == 0); sa / sw hold the e8m0 block
  // scales, four per dword (K blocks of 32 inside one 128-wide K step), K-step-major: sa[kstep * ld_sa + m], sw[kstep * ld_sw + n]
  const unsigned* sa; const unsigned* sw; long ld_sa, ld_sw;
  int kchunk;            // im2col K order: 0 = [tap][channel] (weights [N][taps][C]); 1 = [64-channel chunk][tap][64] - all taps of a chunk are
                         // consecutive K steps, so the activation rows a tile re-reads per tap are still in the XCD's L2 (needs (C0+C1) % 64 == 0)
  int tm_T, tm_nb;       // temporal conv (kt > 1): walk the M tiles frame-fastest - walk index i -> tile (i % tm_T) * tm_nb + i / tm_T, so the tiles of one
                         // pixel block in neighbouring frames (which read each other's rows as taps) run together; 0 = off (needs Ho*Wo % BM == 0)
  int m_off;             // im2col only, producer / consumer kernel only: this launch covers output rows [m_off, m_off + M) of the convolution
                         // (Out / R1 / R2 already point at row m_off) - row-split launches, see launch_gemm
  int group_m;           // tile walk: 0 / 1 = row-major, g > 1 = g M-tiles x all N tiles column by column (set by launch_gemm; see tile_coord)
  int halo_tw, halo_lg;  // set by launch_conv_halo only (kernels/conv_halo.hip): the tile is (256 / halo_tw) x halo_tw output pixels of one frame, halo_tw = 1 << halo_lg;
                         // the epilogue maps tile row r to launch row m0 + (r >> halo_lg) * Wo + (r & (halo_tw - 1))
  int tune_cfg_p1, tune_split_p1, tune_knobs;   // GemmTune of the launching context, + 1 so that a zeroed GemmP means "no override"
  // GroupNorm statistics of the OUTPUT from the epilogue (round 4): per block of `rb` output rows of ONE frame (rb = the wave tile's rows, reported by
  // launch_gemm) and per column the sum / sum of squares of the fp16 values stored, stat_part[blk * N + n]; stat_hw = output rows per frame (blocks
  // must not straddle frames).  The tile_epilogue family's blocks are rb CONSECUTIVE output rows [blk * rb, (blk + 1) * rb); a halo tile's (configs 71 / 72)
  // are the rb / TW image rows x TW pixels of one wave inside its TH x TW pixel tile - not consecutive rows.  What holds for every kernel, and what
  // gn_finalize_cols consumes: frame t owns the blocks [t * stat_hw / rb, (t + 1) * stat_hw / rb) and they cover exactly its rows (section 28 of DESIGN.md).
  // launch_gemm declines (reports rb = 0, writes nothing) when the chosen kernel cannot: split-K, ragged tiles, ...
  float2* stat_part; int stat_hw;
};
// tuning overrides (A/B tools and the tile-config tests; ug_tune_force sets them on ONE context, the engine copies them into every GemmP):
// cfg / split -1 = planner's choice; knobs = bit mask documented in kernels/gemm.hip
struct GemmTune { int cfg = -1, split = -1, knobs = 0; };
static inline void gemm_apply_tune(GemmP& p, const GemmTune& t) { p.tune_cfg_p1 = t.cfg + 1; p.tune_split_p1 = t.split + 1; p.tune_knobs = t.knobs; }
void launch_gemm_mx8(const GemmP& p, hipStream_t s, int* plan_out = nullptr);   // dense only; C0 = lda and ldw in BYTES (= elements); plan_out [2] = (tile pick, group_m) as launched
// fp16 [M, K] (row stride ldx) -> e4m3 bytes [M, K] + e8m0 scales (layout above, ld_s >= M; launch_gemm_mx8 takes ld_s % 4 == 0 and masks its fetch at ld_s); K % 128 == 0
void launch_quant_mx8(const f16* x, long ldx, long M, int K, unsigned char* q, unsigned* scales, long ld_s, hipStream_t s);
void launch_gemm(const GemmP& p, int batch, hipStream_t s, int* stat_rb = nullptr, int* cfg_out = nullptr);   // stat_rb: rows per statistics block written (0 = none), see GemmP::stat_part; cfg_out: the tile config launched (70 - 73 / 80 where the halo-staged / streaming kernel took the planner's launch, 60 for the row-split pair)
// weight-stationary streaming GEMM for K = 320, N in {320, 640, 960} (kernels/gemm_stream.hip; tile config 80): dense, fp16 out, bias + one residual
bool gemm_stream_supported(const GemmP& p, int batch);
void launch_gemm_stream(const GemmP& p, hipStream_t s);
// halo-staged 3x3 convolution (kernels/conv_halo.hip; tile configs 70 / 71 = 256 x 160 / 256 x 128, 72 / 73 = 192 x 128 / 192 x 160 output pixels x columns): stride 1, pad 1, chunk-major weights, whole 256-pixel tiles
bool conv_halo_supported(const GemmP& p, int batch, int bm, int bn);
void launch_conv_halo(const GemmP& p, int bm, int bn, hipStream_t s);
void gemm_plan(const GemmP& p, int batch, int* cfg_out, int* split_out);   // heuristic used when cfg/splitk are 0

// Fused GEGLU feed-forward (kernels/ff_fused.hip): Out = c0 * (GEGLU(X W1^T + b1) W2^T + b2) + c1 R1 + c2 R2, all [M, C] row-major (ld = C);
// W1 [8C][C] / b1 [8C] in the bound GEGLU row order (blocks of 16 rows = [8 value | 8 gate]), W2 [C][4C], C in {64,...,320}
struct FFusedP {
  const f16* X; const f16* W1; const f16* b1; const f16* W2; const f16* b2;
  const f16* R1; const f16* R2; float c0, c1, c2;
  int max_wg;             // cap on the launch grid, 0 = the launcher's choice (the product; ug_op_ff_ex makes a workgroup walk several tiles at small M).
                          // It sits in the padding behind c2 and adds nothing to the kernels' argument block
  f16* Out; int M, C; const f16* zero;
  // optional pre-norm, done on the X tile in LDS (what launch_layernorm would have written, same roundings):
  //   x' = fp16(X + addvec[row / rows_per_vec]) (addvec optional), X_used = fp16(LayerNorm(x') * ln_g + ln_b);
  // with addvec the R1 residual is taken as fp16(R1 + addvec[...]) as well (R1 == X: the block's residual stream)
  const f16* ln_g; const f16* ln_b; float ln_eps; const f16* addvec; int rows_per_vec;
  int variant;            // 0 = default (cross-tile prefetch), 1 = without it (A/B; Ctx::ff_variant, ug_tune_ff)
};
static_assert(sizeof(FFusedP) == 136, "FFusedP: max_wg must stay in the padding behind c2");
bool ff_fused_supported(int C);
int ff_fused_grid(const FFusedP& p);   // workgroups launch_ff_fused launches for p (each walks tiles blockIdx, + grid, ...)
void launch_ff_fused(const FFusedP& p, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Normalisation (kernels/norm.hip)
// ---------------------------------------------------------------------------------------
// GroupNorm over a (virtual concat of two) channels-last tensor(s); statistics per frame
// (temporal == 0) or pooled over all T frames (temporal == 1); optional fused SiLU.
struct GroupNormP {
  const f16* X0; const f16* X1; int C0, C1;
  int T, HW, G; float eps; int temporal; int silu;
  const f16* gamma; const f16* beta;
  f16* Y;                 // [T*HW, C0+C1]
  float* ws;              // >= T * G * 2 * nchunk floats (+ T*G*2 for mean/rstd)
  int mode;               // 0 = automatic; 1 / 2 / 4 / 6 force a launch scheme (launch_groupnorm)
  // statistics already reduced per block of part_rb rows and per channel by the producing GEMM's epilogue (GemmP::stat_part; single source, HW % part_rb == 0):
  // gn_finalize_cols + gn_apply, no pass over X for the statistics
  const float2* part; int part_rb;
};
bool launch_groupnorm(const GroupNormP& p, hipStream_t s);                 // true = the statistics came from p.part (no pass over X for them)
bool groupnorm_uses_part(const GroupNormP& p, int part_rb);                // the launcher's rule for that, for the callers that decide whether a producer writes partial sums
// the launcher's decision for p: the scheme (1 / 2 / 4 / 6), the slab's threads and register vectors (0, 0 unless 4 / 6), chunks per frame and rows per chunk (0 unless 1)
struct GnPlan { int mode, nt, vmax, nchunk, rpc; };
GnPlan groupnorm_plan(const GroupNormP& p);
size_t groupnorm_ws_floats(int T, int HW, int C, int G);

// LayerNorm over rows of [M, C]; optional pre-add of a per-frame broadcast vector
// (x += vec[(m / rows_per_vec) * C + c]) whose sum is also written back to Xout.
struct LayerNormP {
  const f16* X; f16* Y; int M, C; float eps;
  const f16* gamma; const f16* beta;
  const f16* addvec; int rows_per_vec; f16* Xout;   // optional
  long row0;                                        // index of row 0 in the addvec numbering (a row sub-range of a larger tensor)
  // optional MX-fp8 output INSTEAD of Y (fp8 linear path): e4m3 bytes [M][C] + e8m0 block scales, layout of launch_quant_mx8 (C % 128 == 0)
  unsigned char* Y8; unsigned* S8; long ld_s8;
  int form;                                         // 0 = the launcher picks; 1 = the one-wave-per-row ln_kernel also at C = 320 / 640 / 1280 (op tests; 0 on the product path)
};
void launch_layernorm(const LayerNormP& p, hipStream_t s);
int layernorm_form(const LayerNormP& p);            // the kernel the launcher runs for p: L for ln40_kernel<L>, -VPL for ln_kernel<VPL>

// ---------------------------------------------------------------------------------------
// Attention (kernels/attn.hip)
// ---------------------------------------------------------------------------------------
// Flash-style self-attention, head_dim 64.  Q/K/V are column slices of row-major matrices
// (row stride ld*), batch b = frame, rows [b*S, (b+1)*S), head h at columns [h*64, h*64+64).
// Cross-attention: Sk != 0 gives the key/value sequence length (queries keep S); kv_shared = 1 makes every batch read the
// same Sk key/value rows (a text context computed once), otherwise batch b's keys are rows [b*Sk, (b+1)*Sk).
struct FlashP {
  const f16* Q; const f16* K; const f16* V; long ldq, ldk, ldv;
  f16* O; long ldo;
  int B, H, S; float scale;
  int Sk = 0; int kv_shared = 0;
  int variant = -1;   // A/B aid (tools/bench_flash.py; Ctx::flash_variant, ug_tune_flash): -1 = the default form (23), else a bit mask - 1 = one softmax step per 64 keys, 2 = XCD-grouped
                      // workgroup order, 4 = 2-slot K/V ring + 4 workgroups per CU
};
void launch_flash_attn64(const FlashP& p, hipStream_t s);
bool flash_attn_dh_supported(int d);
void launch_flash_attn_dh(const FlashP& p, int d, hipStream_t s);   // self-attention with head dim d in {32, 48, 80, 96, 112, 128} (CLIP ViT-H/14: 80)

// Temporal self-attention: for every pixel p and head h, sequence over the T frames
// (row of frame t = t*HW + p), head_dim 64, T <= 128 (BASELINE config 5 uses 50-frame clips; upstream DepthCrafter's default window is 110 frames).
struct TemporalAttnP {
  const f16* Q; const f16* K; const f16* V; long ld;
  f16* O; long ldo;
  int T, HW, H; float scale;
  int nv = 1;         // videos stacked [nv][T][HW] (the batched guided UNet pass): grid dimension z, the sequence never crosses a video
};
void launch_temporal_attn64(const TemporalAttnP& p, hipStream_t s);

// Row softmax fp32 [rows, ld_in] (first S cols valid) -> fp16 [rows, ld_out], zero tail.
void launch_softmax_rows(const float* in, long ld_in, f16* out, long ld_out, long rows, int S,
                         hipStream_t s);
// Batched transpose: in [B][R][C] (row stride ldi, batch stride sbi) -> out [B][C][Rpad]
// (row stride ldo >= R, zero tail, batch stride sbo).
void launch_transpose(const f16* in, long ldi, long sbi, f16* out, long ldo, long sbo, int B, int R,
                      int C, int nb_inner, long sbi_inner, long sbo_inner, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Small / memory-bound kernels (kernels/misc.hip)
// ---------------------------------------------------------------------------------------
void launch_cast_f32_f16(const float* in, f16* out, long n, hipStream_t s);
void launch_cast_f16_f32(const f16* in, float* out, long n, hipStream_t s);
// weight re-layouts (one-off at bind time)
void launch_permute_conv_w(const f16* in, f16* out, int O, int I, int taps, int Ipad, int Opad,
                           hipStream_t s);   // [O][I][taps] -> [Opad][taps][Ipad] (zero padded)
void launch_upsample_phase_w(const f16* w9, f16* w4, int O, int I, int Ipad, hipStream_t s);   // [O][I][3][3] -> 4 x [O][2*2][Ipad]
void launch_rechunk_conv_w(const f16* in, f16* out, long O, int taps, int Ipad, hipStream_t s);   // [O][taps][Ipad] -> [O][Ipad/64][taps][64]
void launch_gather_rows(const f16* in, f16* out, const int* rowmap, int rows, int cols, hipStream_t s);
void launch_copy2d(const f16* in, long ldi, f16* out, long ldo, long rows, int cols, hipStream_t s);
void launch_fill_f16(f16* p, float v, long n, hipStream_t s);
void launch_fill_random(f16* p, long n, unsigned seed, hipStream_t s);   // uniform [-1,1) hash noise
void launch_add_rowvec(const f16* x, const f16* vec, f16* y, long M, int C, int rows_per_vec,
                       hipStream_t s);      // y[m,c] = x[m,c] + vec[(m/rows_per_vec)*C + c]
void launch_axpby(const f16* a, const f16* b, f16* y, float ca, float cb, long n, hipStream_t s);

// DepthCrafter pipeline glue
void launch_prep_video(const float* frames, const float* noise, f16* clip_src, f16* vae_in,
                       int T, int H, int W, float noise_aug, hipStream_t s);
void launch_clip_patchify(const f16* video_m11, f16* patches, int T, int H, int W, int S224,
                          int P, int Kpad, hipStream_t s, int imagenet_norm = 0);   // 0: CLIP mean/std, 1: ImageNet mean/std (DINOv2)
void launch_scale_rows(f16* w, const f16* gamma, int N, int K, hipStream_t s);     // w[n][:] *= gamma[n] (LayerScale folded into a projection)
void launch_add_grid_nearest(f16* x, const f16* grid, int B, int h, int w, int g, int C, hipStream_t s);   // x[b,y,x,:] += grid[b, y*g/h, x*g/w, :]
void launch_sn_normals_out(const f16* dec, int ldd, float* out, long pixels, hipStream_t s);   // clip to [-1,1], L2-normalise -> f32 [pixels,3]
void launch_resize_bilinear_aa(const float* in, float* out, int B, int Hi, int Wi, int Ho, int Wo, int C, int normalise, hipStream_t s);   // torch antialias bilinear; normalise: re-normalise the channel vector
void launch_init_latents2(const float* noise, f16* lat, float sigma0, int T, long hw, hipStream_t s);
void launch_silu_f16(const f16* in, f16* out, long n, hipStream_t s);
void launch_clip_assemble(const f16* patches, const f16* cls, const f16* pos, f16* tok, int T, int np, int d,
                          hipStream_t s);   // tok[t][0]=cls+pos[0]; tok[t][1+i]=patches[t*np+i]+pos[1+i]
void launch_make_unet_input(const f16* lat, const f16* cond, f16* x, long pixels, float inv_scale,
                            hipStream_t s);   // x[p, 0:4] = lat/sqrt(s^2+1), x[p,4:8] = cond
void launch_euler_step(const f16* v, f16* lat, long n, float sigma, float sigma_next, hipStream_t s);
// classifier-free guidance: the stacked [2][pixels][8] UNet input of the batched pass (video 0 = lat/den | cond, video 1 = lat/den | 0), and the
// guided Euler step v = v_u + g (v_c - v_u) (fp32, rounded to fp16 like the reference's fp16 noise_pred) followed by k_euler_step's arithmetic
void launch_make_unet_input_cfg(const f16* lat, const f16* cond, f16* x, long pixels, float inv_scale, hipStream_t s);
void launch_euler_step_cfg(const f16* vc, const f16* vu, float g, f16* lat, long n, float sigma, float sigma_next, hipStream_t s);
void launch_scale_f16(const f16* in, f16* out, float sc, long n, hipStream_t s);
void launch_axpby_f16(const f16* x, float a, const f16* y, float b, f16* out, long n, hipStream_t s);
void launch_crossfade_f16(const f16* cur, f16* all, long frame_elems, int overlap, hipStream_t s);
void launch_pad_channels(const f16* in, int Cin, f16* out, int Cout, long pixels, hipStream_t s);
void launch_time_conv_out(const f16* x, const f16* w, const f16* b, float* frames_out, int T,
                          long HW, int Cs, hipStream_t s);  // + (x/2+0.5).clamp(0,1) -> f32 [T,HW,3]
void launch_depth_post(const float* frames, float* depth, float* minmax_ws, long pixels,
                       hipStream_t s);        // channel mean, clip-global min-max, 1/(x+0.1)
void launch_disparity_from_frames(const float* frames, const float* minmax_ws, float* disp, long pixels,
                                  hipStream_t s);   // the x of launch_depth_post, from its frames and the min-max it left
void launch_normals(const float* depth, const float* K33, float* normals, int T, int H, int W,
                    hipStream_t s);

// ---------------------------------------------------------------------------------------
// Clip inputs made on the device (kernels/noise.hip)
// ---------------------------------------------------------------------------------------
// Philox4x32-10, key = seed (lo, hi), counter = (q lo, q hi, stream, 0): the four words of blocks q0 .. q0 + nblocks - 1
void launch_philox_u32(uint32_t* out, long nblocks, uint64_t seed, uint32_t stream, uint64_t q0, hipStream_t s);
// out[i] = standard normal number e0 + i of (seed, stream), i in [0, n): Box-Muller on the words of block (e0 + i) >> 2; writes exactly n floats
void launch_randn(float* out, long n, uint64_t seed, uint32_t stream, uint64_t e0, hipStream_t s);
void launch_u8_to_frames(const unsigned char* in_tchw, float* out_thwc, int T, long HW, hipStream_t s);   // planar uint8 -> channels-last f32 x / 255 (HW % 4 == 0)

// ---------------------------------------------------------------------------------------
// fp32-grade path over fp16 hi/lo pairs (kernels/wide.hip): the VAE encoder, which the reference runs in float32
// ---------------------------------------------------------------------------------------
void launch_split_pair(const float* x, f16* y, long M, int C, hipStream_t s);          // [M,C] f32 -> [M,2C] = [hi | lo]
void launch_add_f32(const float* a, const float* b, float* y, long n, hipStream_t s);
void launch_take_cols_f16(const float* x, long ldx, f16* y, long M, int C, hipStream_t s);
size_t gn32_ws_bytes(int T, int HW, int C, int G);
void launch_gn32_pair(const float* X, f16* Y, int T, int HW, int C, int G, float eps, int silu, const f16* gamma, const f16* beta,
                      void* ws, hipStream_t s);                                          // GroupNorm(+SiLU) f32 -> pair
void launch_qk_terms(const float* qkv, f16* Aq, f16* Bk, long M, int C, hipStream_t s);
void launch_vt_terms(const float* qkv, f16* Vt, int B, int S, int Spad, int C, hipStream_t s);
void launch_softmax_pair(const float* in, long ld_in, f16* out, int Spad, long rows, int S, float pscale, hipStream_t s);   // P = [pl | ph | ph] of pscale * softmax

// calibration probe (kernels/probe.hip): chip-wide fp16 MFMA rate, operands in registers; scratch >= 256 * 512 floats
float bench_mfma_peak(float* scratch, int iters, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Evaluation metrics on device (kernels/metrics.hip).  Every `part` array below holds EVAL_MAXB rows of block partials (kernels/eval_reduce.h,
// which the host units include for the constant); *nb returns how many rows the launch filled.
// ---------------------------------------------------------------------------------------
// Depth: one fit and one metric launch for every entry point.  mask1 = gt > 0 && !(gt >= max_depth) (NaN: no upper bound); lo / hi clamp the
// prediction before the alignment, plo / phi after it, -inf / +inf where a mode has none.  A NaN prediction on mask1 is outside the contract:
// the clamp turns it into -inf.
void launch_depth_fit(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, double* part /*[EVAL_MAXB * 5]*/, int* nb,
                      hipStream_t s);
// unfused: s * p + t in two roundings (the L1 alignment).  disparity: the aligned value is a disparity, inverted before the metrics (floor_ = NaN: no
// floor; always unfused).  emap: optional per-pixel relative error of the ORIGINAL prediction.
void launch_depth_metrics(const float* pred, const float* gt, const unsigned char* cmask, long n, float max_depth, float lo, float hi, float plo,
                          float phi, float floor_, float sc, float sh, double* part /*[EVAL_MAXB * 9]*/, float* emap, int* nb, hipStream_t s,
                          bool unfused, bool disparity);
void launch_normal_err(const float* pn, const float* gn, const unsigned char* mask, long n, float* err, double* part,
                       unsigned* hist, int* nb, hipStream_t s);
void launch_collect_bin(const float* err, long n, int bin, float* out, unsigned* count, unsigned cap, hipStream_t s);
// depth alignment modes beyond least squares (kernels/metrics.hip)
#define SEL_PREFIX 2048       // select state (unsigned words): 4 x 2 x 256 histogram words, then prefix[2], rank[2], count, median[2]
#define SEL_RANK 2050
#define SEL_COUNT 2052
#define SEL_MED 2053
#define SEL_WORDS 2056
void launch_masked_median(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, unsigned* sel, hipStream_t s);
void launch_weiszfeld_scale(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, int iters, double* wz,
                            double* part, hipStream_t s);
// alignment in disparity space (kernels/metrics.hip): gfit = mask1 ? 1 / (gt + 1e-8f) : 0, the target the fit kernels above take
// with the depth bound off; launch_depth_metrics then inverts the aligned disparity against the real gt
void launch_disp_target(const float* gt, long n, float max_depth, float* gfit, hipStream_t s);
// exact L1 scale-and-shift alignment (kernels/metrics.hip): state words (unsigned 64-bit) and caps
#define L1_BITS 36            // q = rint(p * 2^(L1_BITS - E))
#define L1_MAX_STEPS 64
#define L1_MAX_TIES 4096
#define L1_CHK_SLOTS 8        // vertex checks launched per readback
#define L1_HIST 0             // 8 passes x 256 bins
#define L1_PREFIX 2048
#define L1_TARGET 2049
#define L1_W 2050
#define L1_TIE_MIN 2051
#define L1_TIE_CNT 2052
#define L1_CHK 2053           // L1_CHK_SLOTS x (below, above, total)
#define L1_WORDS 2080
#define L1_AUX_WORDS (EVAL_MAXB + 2)   // unsigned words: the bits of max |p|, j0, one count per block
void launch_l1_maxabs(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, unsigned* aux, hipStream_t s);
void launch_l1_compact(const float* pred, const float* gt, long n, float max_depth, float lo, float hi, unsigned* aux, double up, float med,
                       unsigned cap, long long* qc, float* gc, hipStream_t s);
void launch_l1_step(const long long* qc, const float* gc, long nv, long j, double down, unsigned long long* st, unsigned* tie_idx,
                    long long* tie_q, hipStream_t s);
void launch_l1_check(const long long* qc, const float* gc, long nv, long z, double S, double down, unsigned long long* out3, hipStream_t s);
// depth evaluation in global coordinates (kernels/metrics.hip); cam: 16 doubles per frame = fx, fy, cx, cy, R row-major, t
void launch_world_radius(const float* pred, const float* gt, const float* gt_radius, const double* cam, long n, int H, int W, float max_depth,
                         float plo, float phi, float sc, float sh, float* radius, double* part, int* nb, hipStream_t s);
void launch_world_points(const float* pred, const double* cam, long n, int H, int W, float plo, float phi, float sc, float sh, float* pts,
                         hipStream_t s);
void launch_radius_metrics(const float* radius, const float* gt, const float* gt_radius, const unsigned char* cmask, long n, float max_depth,
                           float sc, float sh, double* part, float* rmap, int* nb, hipStream_t s);
// point-cloud evaluation (kernels/pcd.hip).  Clouds are [n,3]; idx / dist are per query.  All launches are stream-ordered and
// deterministic: fixed-order fp64 reductions, integer atomics only in the selection histograms.
#define PCD_MAXB EVAL_MAXB    // most blocks of a compaction / reduction launch: `counts` / `part` arrays are sized by it
#define PCD_SEL_WORDS 264     // select state (unsigned words): 256 histogram words, then prefix (2 words), rank (2 words), padding
// order-preserving 64-bit key of a float32 (in the upper word) / float64: negative values have all bits flipped, the others only the sign bit
__host__ __device__ inline unsigned long long pcd_key(double f) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, f);
  return u ^ ((u >> 63) ? ~0ull : (1ull << 63));
}
__host__ __device__ inline unsigned long long pcd_key(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (unsigned long long)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u)) << 32;
}
__host__ __device__ inline double pcd_unkey_f64(unsigned long long k) {
  return __builtin_bit_cast(double, k ^ ((k >> 63) ? (1ull << 63) : ~0ull));
}
__host__ __device__ inline float pcd_unkey_f32(unsigned long long k) {
  const unsigned w = (unsigned)(k >> 32);
  return __builtin_bit_cast(float, w ^ ((w >> 31) ? 0x80000000u : 0xffffffffu));
}
void launch_pcd_compact(const float* pred, const float* gt, const unsigned char* mask, long n, unsigned* counts /*[PCD_MAXB + 1]*/, float* p_out,
                        float* g_out, hipStream_t s);                 // counts[PCD_MAXB] = how many pixels were kept
// the k-th smallest (rank words of `res` slot: the caller passes k) of v[i * stride + offset], float32 or float64 -> res[slot] as the order-preserving 64-bit key
void launch_pcd_select(const void* v, int is_f64, long n, int stride, int offset, unsigned long long k, unsigned* sel, unsigned long long* res,
                       int slot, hipStream_t s);
void launch_pcd_shift_z(float* p, float* g, long n, const unsigned long long* res, int slot_p, int slot_g, hipStream_t s);
void launch_pcd_center_norm(const float* p, long n, const unsigned long long* res, int slot_c, float* norm, hipStream_t s);
void launch_pcd_align(const float* p, const float* g, const long* idx, long ns, float ratio, float gz, float* p32, float* g32, double* p64, double* g64,
                      hipStream_t s);
int pcd_nn_slices(long nq, long nt);
void launch_pcd_nn(const double* q, long nq, const double* t, long nt, const double* T44 /* device, or NULL */, int* idx, double* dist,
                   int* pidx, double* pdist /* [slices][nq] scratch */, hipStream_t s);
void launch_pcd_kabsch(const double* q, const double* t, long nq, const double* T44, const int* idx, const double* dist, double threshold,
                       double* part /*[PCD_MAXB * 17]*/, int* nb, hipStream_t s);
void launch_pcd_move(const double* q, long n, const double* T44, double* out, hipStream_t s);
void launch_pcd_knn_normals(const double* pts, long n, int knn, int* nbr /* [n][min(knn, n)] or NULL */, double* normals, hipStream_t s);
void launch_pcd_normal_dot(const double* nq, const double* nt, const int* idx, long n, double* dot, hipStream_t s);
void launch_pcd_sum(const double* v, long n, double* part /*[PCD_MAXB]*/, int* nb, hipStream_t s);
// threshold scores and the voxel set (kernels/pcd.hip, kernels/voxel.hip): integer counts only
#define PCD_MAX_THRESHOLDS 8             // = the thresholds array of ug_pcd_score_opts
#define PCD_MAX_VOXEL_SIZES 4            // = its voxel_sizes array
struct PcdThresholds { int n; double tau[PCD_MAX_THRESHOLDS]; };
// how many of v[0 .. n) lie strictly below each threshold -> part [PCD_MAXB * PCD_MAX_THRESHOLDS] per-workgroup counts, *nb rows written
void launch_pcd_count_below(const double* v, long n, const PcdThresholds& t, unsigned* part, int* nb, hipStream_t s);
#define VOX_STAT_WORDS 4                 // stat[0]: a probe ran through the whole table; stat[1] / stat[2]: skipped points of cloud 1 / 2
#define VOX_OVERFLOW 0
// keys [capacity] 64-bit words and flags [capacity] 32-bit words, capacity a power of two; fill empties both and zeroes stat
void launch_vox_fill(unsigned long long* keys, unsigned* flags, long capacity, unsigned* stat, hipStream_t s);
// the cells of pts [n,3] for edge v go into the table with flag `bit` (1: prediction, 2: ground truth)
void launch_vox_insert(const double* pts, long n, double v, unsigned bit, unsigned long long* keys, unsigned* flags, long capacity, unsigned* stat,
                       hipStream_t s);
// slots with flags 1, 2 and 3 -> part [PCD_MAXB * 3] per-workgroup counts, *nb rows written
void launch_vox_count(const unsigned* flags, long capacity, unsigned* part, int* nb, hipStream_t s);
// farthest-point sampling: k picks of a float32 cloud [n,3], 1 <= k <= n < 2^31, in k + 1 stream-ordered launches.
// Scratch: m [n] the running smallest squared distance, pm / pi [2 * PCD_MAXB] the per-workgroup (best m, lowest index) of the even and odd launches.
void launch_pcd_fps(const float* p, long n, long k, float* m, float* pm, int* pi, long* idx /*[k]*/, float* sel_dist /*[k]*/, hipStream_t s);
// out32[j] = src[idx[j]] and its float64 copy (either output may be NULL)
void launch_pcd_gather(const float* src, const long* idx, long ns, float* out32, double* out64, hipStream_t s);
// exact search through a uniform grid (kernels/pcd.hip): the same results as launch_pcd_nn / launch_pcd_knn_normals.
#define PCD_GRID_RINGS 3                 // rings of cells a query walks before it is left to the brute-force kernels
#define PCD_GRID_MAX_CELLS (1L << 24)    // cap on Gx * Gy * Gz
#define PCD_GRID_OCC 4.0                 // points per cell that the rule for h aims at
#define PCD_GRID_EPS 9.5367431640625e-07 // 2^-20: slack of the ring bound, far above the rounding of the cell arithmetic (2^24 cells * 2^-51)
struct PcdGrid {                         // shape from the host (pcd_grid_shape), arrays on the device
  double mn[3], h, inv_h;
  int G[3];
  long cells, n, n_in;                   // n points went in, n_in of them finite and in a cell
  const double* pts;                     // the cloud as given [n,3]
  const double* sorted;                  // [n_in,3] cell by cell
  const int* orig;                       // [n_in] the index in pts
  const unsigned* start;                 // [cells + 1] first sorted position of every cell
};
// box (device, 8 doubles): min xyz, max xyz of the finite points, then their count; part [PCD_MAXB * 7] scratch
void launch_pcd_grid_bbox(const double* t, long n, double* part, double* box, hipStream_t s);
// host: cell edge and cells per axis from the box (the rule of DESIGN.md section 20); fills mn, h, inv_h, G, cells, n, n_in
void pcd_grid_shape(const double* box, long n, PcdGrid* g);
// counting sort into the cells: counts [cells] (zeroed here), start [cells + 1], bsum [PCD_MAXB + 2] (bsum[PCD_MAXB + 1] = the fullest cell),
// cell [n] scratch, sorted [n,3] / orig [n] outputs
void launch_pcd_grid_build(const double* t, long n, const PcdGrid& g, unsigned* counts, unsigned* start, unsigned* bsum, int* cell, double* sorted,
                           int* orig, hipStream_t s);
// settled queries get idx / dist; the others are appended to left [nq] and counted in *n_left (device, zeroed here)
void launch_pcd_nn_grid(const double* q, long nq, const double* T44, const PcdGrid& g, int* idx, double* dist, int* left, unsigned* n_left,
                        hipStream_t s);
void launch_pcd_knn_grid(const PcdGrid& g, int knn, int* nbr /* or NULL */, double* normals, int* left, unsigned* n_left, hipStream_t s);
// launch_pcd_knn_normals for the nl queries list[0 .. nl) only; rows of the other points are not written
void launch_pcd_knn_normals_list(const double* pts, long n, int knn, const int* list, long nl, int* nbr, double* normals, hipStream_t s);
void launch_pcd_gather64(const double* src, const int* list, long nl, double* out, hipStream_t s);                          // out[i] = src[list[i]]
void launch_pcd_nn_scatter(const int* list, long nl, const int* idx_l, const double* dist_l, int* idx, double* dist, hipStream_t s);
// focal, poses and depth from world point maps (kernels/pointmap.hip): the arithmetic of harness/pointmap.py.  A frame is
// n = H * W pixels of pts [n,3]; every sum is per-block fp64 partials (part: PM_MAXB rows) that the caller adds in block order.
#define PM_MAXB EVAL_MAXB
struct PmCam { double f, cx, cy; int W; };           // K = [[f, 0, cx], [0, f, cy], [0, 0, 1]], pixel i = (row i / W, column i % W)
struct PmPose { double R[9], t[3]; };                // world to camera, R row-major
// the Weiszfeld chain on the device: fz[0] = the focal after the closed-form start and `steps` reweighting steps; part [PM_MAXB * 2]
void launch_pm_focal(const float* pts, long n, PmCam cam, int steps, double* part, double* fz, hipStream_t s);
// valid[i] = all three coordinates finite and (mask NULL or mask[i] > 0)
void launch_pm_valid(const float* pts, const unsigned char* mask, long n, unsigned char* valid, hipStream_t s);
// per inlier set: n, the six entries of sum b b^T (xx xy xz yy yz zz), sum |X|^2 -> part [nb * 8]
void launch_pm_pass0(const float* pts, const unsigned char* keep, long n, PmCam cam, double* part, int* nb, hipStream_t s);
// sum (b b^T - I) R X -> part [nb * 3]
void launch_pm_pass1(const float* pts, const unsigned char* keep, long n, PmCam cam, PmPose pose, double* part, int* nb, hipStream_t s);
// q = b b^T (R X + t): n, sum X (3), sum q (3), sum q X^T (9, row = q), the object-space error sum |R X + t - q|^2 -> part [nb * 17]
void launch_pm_pass2(const float* pts, const unsigned char* keep, long n, PmCam cam, PmPose pose, double* part, int* nb, hipStream_t s);
// keep_new[i] = valid, z > 0 and squared reprojection error <= thr2; the count, how many differ from keep, the sum of the kept errors -> part [nb * 3]
void launch_pm_inliers(const float* pts, const unsigned char* valid, const unsigned char* keep, long n, PmCam cam, PmPose pose, double thr2,
                       unsigned char* keep_new, double* part, int* nb, hipStream_t s);
// depth[i] = (float) z of R X + t, 0 where not valid
void launch_pm_depth(const float* pts, const unsigned char* valid, long n, PmPose pose, float* depth, hipStream_t s);
// depth / normal visualisation panels (kernels/vis.hip); part: 2 * 1024 floats of scratch, out2 (device) = (vmin, vmax)
void launch_vis_range(const float* x, long n, float* part, float* out2, hipStream_t s);
void launch_vis_panel(const float* rgb, const float* normals, const float* depth, const float* lut, const float* cbar, unsigned char* out, int T,
                      int H, int W, int Wc, float vmin, float vmax, hipStream_t s);
// ScanNet++ clip preparation (kernels/prep.hip); tap tables tap-major ([K][n_out]), mid: T*3*Ho*Wi doubles of scratch,
// cam: 20 doubles per frame = fx, fy, cx, cy, M33 row-major, t3; the index tables must have been validated by the caller
void launch_prep_resize(const unsigned char* frames, const int* ridx, const double* rw, int Kr, const int* cidx, const double* cw, int Kc,
                        int T, int Hi, int Wi, int Ho, int Wo, double* mid, float* out, hipStream_t s);
void launch_prep_gt(const unsigned short* depth, const unsigned char* normals, const double* cam, const int* row_idx, const int* col_idx, int T,
                    int Hi, int Wi, int Ho, int Wo, float divisor, float max_depth, int depth_f64, int zoomed, float* cam_normal, float* world_normal,
                    float* cam_coord, float* world_coord, float* mask, hipStream_t s);
// Ground-truth normals fitted from the depth at the picked pixels (kernels/gt_normals.hip).  depth [T,Hi,Wi] uint16, cam
// and the tables as launch_prep_gt takes them, the outputs [T,3,Ho,Wo] x 2 and [T,Ho,Wo]; all on the device, n = T * Ho * Wo.  The caller
// has validated the tables, 1 <= radius <= 8 and min_count >= 1; edge is read only when edge_on.
struct GtNormalsArgs {
  const unsigned short* depth; const double* cam; const int* row_idx; const int* col_idx;
  float* cam_normal; float* world_normal; float* normal_mask;
  long n; int Hi, Wi, Ho, Wo; int zoomed, depth_f64; float divisor, max_depth;
  int radius, min_count, edge_on; double edge;
};
void launch_prep_gt_normals(const GtNormalsArgs& a, hipStream_t s);
// 7-Scenes depth registration (kernels/register.hip): depth / out uint16 [T,H,W], zbuf T*H*W words of scratch, all on the
// device; m: the source-to-target transform, row-major 3x4
struct RegArgs { double src_focal, dst_focal; double m[12]; float divisor, max_valid; int drop_sentinel; };
void launch_register_depth(const unsigned short* depth, int T, int H, int W, const RegArgs& a, unsigned* zbuf, unsigned short* out, hipStream_t s);
// Temporal alignment error (kernels/temporal.hip).  s, t: the clip's fit; floor_: NaN when off; plo / phi: the post-clip
// bounds (-inf / +inf when off); md: the depth bound of the score (NaN: gt > 0 only).  pred / gt [T,H,W], cmask NULL or [T,H,W], K [T,9] float32,
// rel [P,12] doubles, zbuf / warp_out / err_out (either may be NULL) P*H*W words, part P * eval_nblocks(H*W) * 2 doubles (the block count comes
// back in *nb_out).  All on the device; P = 2 * (T - stride) >= 1, P * H * W < 2^31.
struct TaeArgs { float s, t, floor_, plo, phi, md; int disparity, stride; };
void launch_tae(const float* pred, const float* gt, const unsigned char* cmask, const float* K, const double* rel, int P, int H, int W,
                const TaeArgs& a, unsigned* zbuf, double* part, float* warp_out, float* err_out, int* nb_out, hipStream_t s);
// ScanNet++ mesh renderer (kernels/render.hip).  verts [NV,3] float32, faces [NF,3] int32 (every index validated by the
// caller), cams 16 doubles per frame = world-to-camera row-major 3x4, fx, fy, cx, cy; mask NULL or [T,H,W]; zbuf: T*H*W 64-bit words of
// scratch; big_id / big_tile: big_cap entries of scratch for the boxes a whole workgroup walks, big_count one word; depth [T,H,W],
// normal [T,H,W,3], tri NULL or [T,H,W].  All on the device; T * H * W < 2^31, NF < 2^31.
struct RenderBufs {
  unsigned long long* zbuf; long long* big_id; int* big_tile; unsigned long long* big_count; unsigned big_cap;
  unsigned short* depth; unsigned char* normal; int* tri;
};
void launch_render_mesh(const float* verts, const int* faces, long NF, const double* cams, int T, int H, int W, double znear, double zfar,
                        const unsigned char* mask, const RenderBufs& b, hipStream_t s);
