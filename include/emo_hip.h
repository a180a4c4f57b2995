/* emo_hip.h - C ABI of the MI355X (gfx950) kernels behind the Emote-hack diffusion hot path.
 *
 * The reference is Python calling Python: it has NO FFI for this path.
 * The drop-in boundary is therefore the Python surface (UNet3DConditionModel /
 * ReferenceAttentionControl / EMOAnimationPipeline, mirrored in emote_hack_amd/), and this
 * header is the C ABI underneath it.  Each entry point names the reference ATen/xformers op
 * (file:line under /root/reference) it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain pointers + sizes; no C++/torch types; every pointer is a DEVICE pointer unless
 *     the name ends in _host.  Buffers are caller-owned and must stay alive until `stream`
 *     has passed the call.
 *   - activations are "rows x channels" row-major (NHWC: row = ((b*F+f)*H + y)*W + x); `ld*`
 *     are leading dimensions in ELEMENTS.  Weights are [N][K] row-major (torch Linear layout;
 *     conv weights re-laid once at load to [Cout][ky][kx][Cin]).
 *   - dtype: EMO_F32 (validation mode: f32 MFMA, exact-f32 accumulate), EMO_BF16 or EMO_F16 (IEEE half: the reference's
 *     `weight_dtype=torch.float16` configurations; same kernels, v_mfma_f32_32x32x16_f16)
 *     (production: bf16 MFMA, f32 accumulate).  Statistics / softmax / latents are always f32.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never allocates,
 *     never synchronises, keeps no global mutable state (re-entrant per stream).
 *   - returns EMO_OK (0) or a negative emo_status; emo_last_error_string() describes the last
 *     failure on the calling thread.
 */
#ifndef EMO_HIP_H
#define EMO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { EMO_F32 = 0, EMO_BF16 = 1, EMO_F16 = 2 } emo_dtype;

typedef enum {
  EMO_OK = 0,
  EMO_ERR_BAD_SHAPE = -1,
  EMO_ERR_BAD_DTYPE = -2,
  EMO_ERR_UNSUPPORTED = -3,
  EMO_ERR_HIP = -4,
  EMO_ERR_NULL = -5
} emo_status;

int emo_version(void);
const char* emo_last_error_string(void);

/* ---- layout / elementwise ------------------------------------------------------------------ */

/* (B,C,F,H,W) f32 -> rows ((b f) h w, ldo>=C) in `dtype`; channels [C, Cpad) are written as 0.
 * Replaces einops "b c f h w -> (b f) c h w" + channels-last (resnet.py:33, attention.py:115). */
int emo_ncfhw_to_rows(const float* x, void* y, int B, int C, int F, int H, int W, int Cpad, int ldo,
                      int dtype, void* stream);
/* rows -> (B,C,F,H,W) f32 (the UNet output boundary, unet_controlnet.py:478-483). */
int emo_rows_to_ncfhw(const void* x, float* y, int B, int C, int F, int H, int W, int ldi, int dtype,
                      void* stream);
/* y[m, coff:coff+C] = x[m, 0:C]   (torch.cat along channels, unet_3d_blocks.py:629,731). */
int emo_copy_cols(const void* x, int ldx, void* y, int ldy, int coff, int64_t M, int C, int dtype, void* stream);
/* y = a + alpha*b elementwise over M x C (ControlNet residual adds, unet_controlnet.py:430-447). */
int emo_add(const void* a, int lda, const void* b, int ldb, float alpha, void* y, int ldy, int64_t M, int C,
            int dtype, void* stream);
/* y[m, :] = x[m, :] + f[m % P, :] over M x C rows, f a (P, C) map: the face-region features added to the output of conv_in for
 * every frame of every batch row (Net.py:509-516 `face_features = self.face_locator(face_mask)`; train_stage_3_speedlayers.py:242-271
 * adds them in front of the UNet), P = H * W.  y may be x (in place: the zero-copy skip slot keeps its address).  f32 sum, rounded once.
 * C, ldx, ldf, ldy multiples of the 16-byte vector, operands 16-byte aligned; M % P != 0 is refused. */
int emo_add_periodic(const void* x, int64_t ldx, const void* f, int64_t ldf, void* y, int64_t ldy, int64_t M, int C, int64_t P,
                     int dtype, void* stream);
/* A face-region mask at pixel size -> the latent-size input rows of FaceRegionController (train_stage_3_speedlayers.py:57-76: the mask
 * is fed at the latents' size): x f32 (Hp, Wp), y (Hp / 8 * Wp / 8, 8) rows of `dtype`; channel 0 = the mean over the cell's 8 x 8
 * pixels, channels 1..7 = 0 (the conv loader's channel pad).  use_thr != 0 pools (x > thr ? 1 : 0) instead - FaceLocator logits
 * (Net.py:819-855) with thr = 0, i.e. sigmoid > 0.5.  Hp, Wp multiples of 8, x 16-byte aligned. */
int emo_mask_pool(const float* x, void* y, int Hp, int Wp, int use_thr, float thr, int dtype, void* stream);
/* dtype conversion of a contiguous buffer (src f32 <-> dst dtype); fp16_round!=0 rounds through IEEE
 * half first (bank hand-off, mutual_self_attention.py:588 `.to(float16)`). */
int emo_convert(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, int fp16_round, void* stream);
/* y = silu(x) over n contiguous elements (F.silu(temb), resnet.py:186). */
int emo_silu(const void* x, void* y, int64_t n, int dtype, void* stream);

/* sinusoidal timestep embedding (embeddings.py:28-68 get_timestep_embedding): out[b] =
 * [sin | cos](t_b * freqs) (flipped to [cos | sin] if flip_sin_to_cos).  `freqs` f32 [dim/2] is the
 * constant table exp(-ln(1e4)*arange(half)/(half - freq_shift)) built once by the host; the integer
 * timestep is consumed bit-exactly. */
int emo_timestep_embedding(const int64_t* timesteps, const float* freqs, void* out, int B, int dim,
                           int flip_sin_to_cos, int dtype, void* stream);

/* emo_timestep_embedding over f32 timesteps (the fractional tables of Euler / Euler-ancestral / LMS); an integral value gives
 * the bits of the int64 entry. */
int emo_timestep_embedding_f32(const float* timesteps, const float* freqs, void* out, int B, int dim,
                               int flip_sin_to_cos, int dtype, void* stream);

/* ---- normalisation ---------------------------------------------------------------------------
 * GroupNorm over NHWC rows.  An "instance" is a contiguous run of S rows normalised together:
 *   5-D joint statistics (resnet.py:180,191; unet_controlnet.py:476): N=B,   S=F*H*W
 *   per-frame            (attention.py:124; motion_module.py:147)   : N=B*F, S=H*W
 * Two launches: emo_groupnorm_stats writes row-chunk partial (sum, sumsq) per group into `partials` (caller
 * workspace of emo_groupnorm_workspace_bytes(N, S, C, G) bytes); emo_groupnorm_apply combines them in f64 in a
 * fixed order (deterministic; every block recomputes the same (mean, rstd)) and normalises (+SiLU).
 * gamma / beta are f32, 16-byte aligned. */
size_t emo_groupnorm_workspace_bytes(int N, int64_t S, int C, int G);
int emo_groupnorm_stats(const void* x, int ldx, void* partials, int N, int64_t S, int C, int G, int dtype,
                        void* stream);
int emo_groupnorm_apply(const void* x, int ldx, const void* partials, const float* gamma, const float* beta,
                        void* y, int ldy, int N, int64_t S, int C, int G, float eps, int silu, int dtype,
                        void* stream);

/* The coefficient half of emo_groupnorm_apply for consumers that normalise on the fly (emo_gemm_params.gn_coef):
 * scale_c = rstd_{n,g(c)} * gamma_c, shift_c = beta_c - mean_{n,g(c)} * scale_c from the `partials` of emo_groupnorm_stats with the
 * same fixed-order f64 combine - bit-identical to the factors emo_groupnorm_apply uses.  coef is f32 [N][2 * C], channel PAIRS
 * interleaved: coef[n][4 * j ..] = (scale_2j, scale_2j+1, shift_2j, shift_2j+1) - one 16-byte read per packed pair.  C even. */
int emo_groupnorm_coeffs(const void* partials, const float* gamma, const float* beta, float* coef, int N, int64_t S,
                         int C, int G, float eps, int dtype, void* stream);

/* Scale-shift GroupNorm (resnet.py:149-156,191-197: ResnetBlock3D(time_embedding_norm="scale_shift")): behind norm2 the time
 * embedding modulates instead of being added in front of it,  y = act(GN(x) * (1 + s) + t),  (s, t) = chunk(time_emb_proj(silu(temb)), 2)
 * per (batch row, channel).  `mod` is f32 [N][(scale | shift)]: mod[n * ldmod + c] = s, mod[n * ldmod + C + c] = t (ldmod >= 2 * C, a
 * multiple of 4; mod 16-byte aligned; C a multiple of 4) - a column view of the batched time-embedding GEMM's output.  A per-(instance,
 * channel) affine of x like the plain norm: the modulation is folded into the thread's copy of the affine, gamma' = gamma (1 + s),
 * beta' = beta (1 + s) + t, and the plain arithmetic runs on it - factors a' = rstd gamma (1 + s), b' = (beta - mean rstd gamma)(1 + s) + t
 * - so the pass stays ONE read and ONE write of the activation (+ N * 2C floats).  Same partials, same fixed-order f64 combine, same limits:
 *   emo_groupnorm_apply_mod   the second of the two launches (after emo_groupnorm_stats)       (resnet.py:191-197)
 *   emo_groupnorm_mod         the one-launch kernel, where emo_groupnorm_one_launch_ok says 1  (resnet.py:191-197)
 *   emo_groupnorm_coeffs_mod  the (a', b') table for emo_gemm_params.gn_coef, bit-identical to the factors the two above use
 *                             (resnet.py:191-200: norm2 -> modulate -> SiLU inside conv2) */
int emo_groupnorm_apply_mod(const void* x, int ldx, const void* partials, const float* gamma, const float* beta,
                            const float* mod, int ldmod, void* y, int ldy, int N, int64_t S, int C, int G, float eps,
                            int silu, int dtype, void* stream);
int emo_groupnorm_mod(const void* x, int ldx, const float* gamma, const float* beta, const float* mod, int ldmod, void* y,
                      int ldy, int N, int64_t S, int C, int G, float eps, int silu, int dtype, void* stream);
int emo_groupnorm_coeffs_mod(const void* partials, const float* gamma, const float* beta, const float* mod, int ldmod,
                             float* coef, int N, int64_t S, int C, int G, float eps, int dtype, void* stream);

/* The PER-FRAME form of the scale-shift modulation: with one speed embedding per frame in the time embedding (EMO's head-rotation
 * speed, train_stage_3_speedlayers.py:57-76,242-271, through time_emb_proj, resnet.py:188-195) the statistics of a resnet's GroupNorm
 * stay joint over the F frames of a batch row, but (scale | shift) differs per frame.  `mod_rows` is the number of consecutive rows of x
 * that share one mod row: row m of x (m = n * S + s) takes mod[(m / mod_rows) * ldmod + c] and mod[(m / mod_rows) * ldmod + C + c];
 * mod has N * S / mod_rows rows and mod_rows divides S (an instance holds whole frames; mod_rows = H * W in the UNet).  Same
 * partials, same combine, same three roundings of the modulation as the instance form: with every frame of an instance sharing one
 * mod row the output is bit-identical to emo_groupnorm_apply_mod / emo_groupnorm_mod / emo_groupnorm_coeffs_mod.
 *   emo_groupnorm_apply_mod_rows   after emo_groupnorm_stats
 *   emo_groupnorm_mod_rows         the one-launch kernel, where emo_groupnorm_one_launch_ok says 1
 *   emo_groupnorm_coeffs_mod_rows  the (a', b') table with ONE ROW PER FRAME, coef [N * S / mod_rows][2 * C]: the consumer sets
 *                                  emo_gemm_params.gn_imgs_per_inst = 1 */
int emo_groupnorm_apply_mod_rows(const void* x, int ldx, const void* partials, const float* gamma, const float* beta,
                                 const float* mod, int ldmod, int64_t mod_rows, void* y, int ldy, int N, int64_t S, int C, int G,
                                 float eps, int silu, int dtype, void* stream);
int emo_groupnorm_mod_rows(const void* x, int ldx, const float* gamma, const float* beta, const float* mod, int ldmod,
                           int64_t mod_rows, void* y, int ldy, int N, int64_t S, int C, int G, float eps, int silu, int dtype,
                           void* stream);
int emo_groupnorm_coeffs_mod_rows(const void* partials, const float* gamma, const float* beta, const float* mod, int ldmod,
                                  int64_t mod_rows, float* coef, int N, int64_t S, int C, int G, float eps, int dtype, void* stream);

/* The same GroupNorm in ONE launch, for instances small enough that one workgroup holds (instance, slab of whole groups)
 * in registers (<= 32 K elements per workgroup: the 8x8 level and the per-frame 16x16 norms at the bench size): one read of x, statistics in the same fixed
 * order (f32 partials, f64 mean / variance), one write.  emo_groupnorm_one_launch_ok returns 1 when the geometry fits;
 * emo_groupnorm returns EMO_ERR_UNSUPPORTED otherwise (the caller then uses the two launches above). */
int emo_groupnorm_one_launch_ok(int N, int64_t S, int C, int G, int dtype);
int emo_groupnorm(const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, int N, int64_t S,
                  int C, int G, float eps, int silu, int dtype, void* stream);

/* What the GroupNorm entries would launch for (N, S, C, G, dtype), asked without a launch (host only; the geometry functions the
 * launches call):
 *   plan[0..5]   the two launches: NC (column parts of whole groups, blockIdx.y), channels per part, row slots per block,
 *                nsplit_stats (row chunks = partials per instance, <= 256), nsplit_apply (row chunks of the apply pass),
 *                wide (1: a part holds more than 256 column vectors, up to 3 per thread)
 *   plan[6..11]  the one-launch kernel: ok (= emo_groupnorm_one_launch_ok), groups per slab, channels per slab, threads per block,
 *                rows per thread the kernel is instantiated for (2 / 4 / 8 / 16), row slots per block (zeros where ok is 0)
 * Returns what the entries' shape checks return for contiguous rows, and writes nothing on a refusal. */
int emo_groupnorm_plan(int N, int64_t S, int C, int G, int dtype, int plan[12]);

/* GroupNorm folded into the Linear / 1x1 conv that consumes it (attention.py:124,135-146 `norm` -> `proj_in`;
 * motion_module.py:147-151): GN(x) W^T + b over an instance n = x W'_n^T + b'_n with
 *   W'_n[o, c] = W[o, c] * gamma_c * rstd_{n, g(c)}      (rounded to the compute dtype, [N][Cout][C] -> `w_out`)
 *   b'_n[o]    = b[o] + sum_c W[o, c] * beta_c - sum_c mean_{n, g(c)} * W'_n[o, c]   (f32, [N][Cout] -> `rowbias_out`)
 * from the `partials` of emo_groupnorm_stats (same fixed-order f64 combine as emo_groupnorm_apply): the normalised tensor is
 * never written or re-read; emo_gemm then runs with W = w_out, bias = rowbias_out, w_slab_rows = S, w_slab_stride = Cout * C.
 * W is [Cout][C] in `dtype`, bias f32 [Cout] or NULL. */
int emo_groupnorm_fold_linear(const void* partials, const float* gamma, const float* beta, const void* W, const float* bias,
                              void* w_out, float* rowbias_out, int N, int64_t S, int C, int G, int Cout, float eps, int dtype,
                              void* stream);

/* LayerNorm over the last dim (attention.py:279-316, motion_module.py:216-224), eps 1e-5 default.
 * Optional fused temporal positional-encoding add (motion_module.py:246-248,282-283):
 * y[row] += pe[frame(row)] with frame(row) = (row / rows_per_frame) % frames, pe f32 [max_len][C]. */
int emo_layernorm(const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, int64_t M,
                  int C, float eps, const float* pe, int rows_per_frame, int frames, int dtype, void* stream);
/* the statistics half of it: stats[m] = (mean, 1 / sqrt(var + eps)) of row m (two-pass, f32) for the LayerNorm fold of
 * emo_gemm (emo_gemm_params.ln_stats) - a read-only pass over x. */
int emo_layernorm_stats(const void* x, int ldx, float* stats, int64_t M, int C, float eps, int dtype, void* stream);
/* y = act(LayerNorm(x)) over the last dim in one read and one write, act 0 none | 1 erf-GELU (emo_channelnorm's convention): the
 * LayerNorm + GELU behind every feature-encoder conv of the layer-norm wav2vec2 family (Net.py:607-648 -> transformers
 * Wav2Vec2LayerNormConvLayer: conv -> LayerNorm over channels -> GELU).  emo_layernorm's row geometry, checks and limits; two-pass
 * f32 statistics, the activation on the f32 normalised value, one rounding to `dtype`.  No pe operand; act = 0 gives what
 * emo_layernorm(pe = NULL) gives, bit for bit. */
int emo_layernorm_act(const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, int64_t M, int C, float eps,
                      int act, int dtype, void* stream);
/* What the three would launch for (M, C, dtype), asked without a launch (host only): plan = lanes per row (1 .. 64), rows per
 * wavefront, grid (blocks of 4 wavefronts, <= 4096), 1 if the rows need a second trip of the grid.  Returns what their shape
 * checks return for contiguous rows, and writes nothing on a refusal. */
int emo_layernorm_plan(int64_t M, int C, int dtype, int plan[4]);

/* ---- GEMM / convolution (MFMA) ----------------------------------------------------------------
 * C[M,N] = epilogue( A[M,K] . W[N,K]^T ).  Replaces F.linear / 1x1 conv (orig_attention.py:566-575,
 * 776,817; attention.py:82,110; resnet.py:175) and, with conv geometry, the per-frame 3x3 conv
 * (resnet.py:30-38 InflatedConv3d).  Epilogue, in order:
 *   + bias[N]  (f32, may be NULL)
 *   + rowbias[(m / rows_per_batch)][N] (f32; the `+ temb[:, :, None, None, None]` of resnet.py:188)
 *   GEGLU: W rows are interleaved (32 value rows, 32 gate rows) per 32 outputs -> out[m,j] = v*gelu_erf(g),
 *          N_out = N/2 (orig_attention.py:825-827)
 *   + residual[M, N_out] (resnet.py:205, attention.py:292-317)        * out_scale
 *   store: row-major (ldc) or TRANSPOSED per batch: Ct[(m / t_rows)][n][m % t_rows] with ld t_ld
 *          (the V^T layout the attention kernels consume). */
typedef struct {
  const void* A; int64_t lda;
  const void* W;              /* [N][K] (K = taps*Cin for conv) */
  const float* bias;
  const float* rowbias; int rows_per_batch; int ld_rowbias;
  const void* residual; int64_t ldr;
  void* C; int64_t ldc;
  int64_t M; int N; int K;
  int geglu;
  float out_scale;
  int transpose_out; int t_rows; int64_t t_ld; int64_t t_batch_stride;
  /* conv geometry (conv_taps==9 -> implicit 3x3 GEMM over NHWC A; 0 -> dense) */
  int conv_taps; int H; int W_; int Cin; int stride; int upsample2x; int Ho; int Wo;
  int dtype;
  /* split-K for problems with too few output tiles to fill 256 CUs (small M at the 8x8 / 16x16 levels):
   * split_k > 1 slices K over grid.y, f32 partial tiles go to `workspace` ([split_k][M][N] floats, at least
   * emo_gemm_workspace_bytes(p) bytes) and a second kernel reduces them in a fixed order (deterministic)
   * and applies the epilogue.  split_k <= 1: single pass, workspace unused. */
  int split_k; void* workspace;
  /* LayerNorm folded into the GEMM (attention.py:279-316, motion_module.py:216-224: every LayerNorm of the transformer
   * blocks feeds a Linear).  With ln_colsum / ln_stats != NULL the kernel computes
   *     C = epilogue( ((A - mean_m) * rstd_m) . W^T + bias ),   ln_stats[m] = (mean_m, rstd_m) from emo_layernorm_stats
   * as rstd_m * (bias[n] / rstd_m - mean_m * ln_colsum[n] + A.W^T) with ln_colsum[n] = sum_k W[n][k]: the correction enters
   * through the accumulator init, the epilogue pays one multiply, and no normalised copy of A ever exists in HBM.  The caller
   * folds the LayerNorm affine into the operands once at load: W <- W * gamma[k], bias <- bias + W . beta.  Dense, split_k <= 1. */
  const float* ln_colsum; const float* ln_stats;
  int tile;   /* 0 = planned from the shape; 1..6 pin a tile (64x64, 128x128, 128x160, 256x256, 256x160, 256x320) - tuning hook
                 in the spirit of a BLAS algorithm id; combinations a tile cannot serve fall back to the nearest one that can.
                 Stride-1 3x3 convs the halo-reuse kernel serves read it as hint bits instead: (tile & 3) 1 / 2 pins 8 / 16-row
                 patches, 4 keeps one launch at N % 128 == 64, 8 keeps the 64-column remainder launch, 16 forces 192-column blocks,
                 32 keeps the rolled main loop where the one with its nine taps unrolled is the default (same bits).
                 A conv the halo kernel does not serve drops bits 8 / 16 / 32 and reads the rest as the tile pin. */
  int conv_asym;   /* conv only: 1 = padding (0, 1, 0, 1) instead of 1 all round - the `F.pad(x, (0,1,0,1))` + stride-2
                      conv of the VAE encoder's Downsample2D (diffusers AutoencoderKL; Ho = (H + 1 - 3) / stride + 1) */
  int up_h; int up_w;  /* conv only: nearest upsampling to an EXPLICIT size folded into the loader (F.interpolate(size=...),
                      resnet.py:74-82 with `output_size`: inputs that are not a multiple of 2^num_upsamplers,
                      unet_controlnet.py:357-365,456-459); source pixel = min((int)floorf(dst * ((float)H / up_h)), H - 1), torch's
                      nearest index with its f32 scale (not the integer dst * H / up_h, which differs from it e.g. at H = 14,
                      up_h = 46, dst = 23: 6 against 7).  0 = off (upsample2x covers x2) */
  int w_slab_rows; int64_t w_slab_stride;  /* dense only: per-instance weights - rows [i * w_slab_rows, (i+1) * w_slab_rows) of A
                      multiply the weight slab W + i * w_slab_stride (elements); w_slab_rows must be a multiple of 256 (a tile never
                      straddles two slabs).  `bias` is then per instance as well: f32 [M / w_slab_rows][N].  0 = one W (and one bias)
                      for every row.  Made by emo_groupnorm_fold_linear (GroupNorm folded into proj_in); row-major output with
                      N % 4 == 0 only, not with the LayerNorm fold, split-K or the conv loader. */
  /* 3x3 conv only: GroupNorm (+ SiLU) of the conv's INPUT applied inside the conv (resnet.py:180-183,191-196: norm -> nonlinearity ->
   * conv).  A holds the RAW producer output; gn_coef is the f32 [instances][2 * Cin] table of emo_groupnorm_coeffs
   * (per channel pair: scale, scale, shift, shift with scale = rstd * gamma, shift = beta - mean * scale), image i of A belongs to
   * instance i / gn_imgs_per_inst (F for the joint 5-D statistics of the resnets, 1 per frame).  The kernel normalises, activates and rounds each halo chunk in LDS right
   * after its direct-to-LDS load lands - the same arithmetic, in the same order, as emo_groupnorm_apply followed by the plain conv
   * (the padding stays zero) - so the normalised tensor is never written to or re-read from HBM.  Served by the halo-reuse kernel
   * only: emo_conv3x3_gn_fusable(p) says whether a given conv qualifies; emo_gemm returns EMO_ERR_UNSUPPORTED otherwise. */
  const float* gn_coef; int gn_imgs_per_inst; int gn_silu;
  /* dense, single pass, row-major: the columns [vt_col0, N) are stored TRANSPOSED into `vt` instead - V^T [(m / t_rows)][n - vt_col0][m % t_rows]
   * with t_ld / t_batch_stride as for transpose_out - while the columns [0, vt_col0) go to C as usual (ldc >= vt_col0): ONE launch for the
   * q | k | v projection of a self-attention whose V the attention kernel wants key-contiguous (orig_attention.py:598-600 to_q / to_k / to_v on
   * the same rows; attention.py:279-293) - the rows are read once.  The accumulator layout of the row-major kernels already has consecutive rows m in
   * consecutive lanes: a register is 32 contiguous elements of a V^T row.  vt_col0 must be a multiple of the planned tile's wave width
   * (emo_gemm_vt_ok), N - vt_col0 a multiple of 8, M a multiple of 32; with the LayerNorm fold (ln_colsum / ln_stats) only; no GEGLU / residual / row bias /
   * out_scale.  NULL = off. */
  void* vt; int vt_col0;
} emo_gemm_params;
int emo_gemm(const emo_gemm_params* p, void* stream);
/* 1 when the conv described by p (gn_* fields ignored) runs on the halo-reuse kernel, i.e. may carry gn_coef */
int emo_conv3x3_gn_fusable(const emo_gemm_params* p);
/* 1 when p (with vt / vt_col0 set) is a GEMM the split row-major | transposed store serves on the tile the planner picks for it */
int emo_gemm_vt_ok(const emo_gemm_params* p);
/* Host-only: what emo_gemm would launch for p.  Runs emo_gemm's argument checks and planning and returns their status; writes nothing
 * on a refusal, launches nothing and touches no device memory (the pointers of p are only compared with NULL and checked for alignment).
 *   plan[0] family      0 = the tile kernel, 1 = the halo-reuse 3x3 conv (the other fields are then 0)
 *   plan[1] tile        the tile instantiated, after every fallback: 1 64x64, 2 128x128, 3 128x160, 4 256x256, 5 256x160, 6 256x320,
 *                       7 256x256 with the phase main loop
 *   plan[2] main loop   0 = lockstep, 1 = phase
 *   plan[3] flags       bit 0 conv loader, bit 1 transposed (V^T) kernel, bit 2 LayerNorm fold, bit 3 split row-major | V^T store (vt)
 *   plan[4] split_k     as launched (1 = single pass)
 *   plan[5] store path  0 LDS-staged full lines, 1 vector row (8 / 16 bytes per quad), 2 scalar row, 3 V^T quad, 4 V^T scalar,
 *                       5 split-K workspace (f32 partials; the reduce kernel stores the output)
 *   plan[6], plan[7]    1 when the bias / the per-batch row bias starts the accumulators instead of being added in the epilogue */
int emo_gemm_plan(const emo_gemm_params* p, int plan[8]);
/* Host-only: the launch decisions of the halo-reuse 3x3 conv for p - the ones emo_gemm launches by (one function makes both).  Runs
 * emo_gemm's argument checks and returns their status; writes nothing on a refusal, launches nothing, touches no operand (C and
 * residual are compared as address ranges: a residual that overlaps the output is an in-place epilogue).
 *   plan[0] served      1 = the halo-reuse kernel runs this conv; 0 = the tile kernel does (the other fields are then 0)
 *   plan[1] patch height 8 or 16 rows
 *   plan[2..4] the main launch: output channels per block (128; 64 at N = 64; 192 at N = 192 under emo_gemm_params.tile bit 2), tiles, grid - 0s when
 *              there is none (N = 192 on 192-column blocks: the tail launch is the only one)
 *   plan[5..7] the tail launch over the last 64 or 192 columns of a width that is an odd multiple of 64: block width, tiles, grid - 0s
 *              when there is none */
int emo_conv3x3_halo_plan(const emo_gemm_params* p, int plan[8]);
/* heuristic split factor for (M, N, K) and the workspace it needs */
int emo_gemm_suggest_split_k(int64_t M, int N, int K, int dtype, int geglu, int transpose_out);
size_t emo_gemm_workspace_bytes(int64_t M, int N, int split_k);

/* ---- attention -------------------------------------------------------------------------------
 * Flash-style softmax(q k^T * scale) v, scores never leave the chip.  Replaces
 * CrossAttention._attention (orig_attention.py:655-684) and xformers.memory_efficient_attention
 * (models/motionmodule.py:300, models/videonet.py:62,117).
 *   q  : [B*Lq][ldq] rows, head h at columns h*d
 *   k0 : [B*Lk0][ldk0] rows (self / context keys of batch b)
 *   v0t: V^T [B][heads*d][ldv0t] (keys contiguous, ldv0t >= Lk0, multiple of 8)
 *   k1/v1t: optional second KV segment shared by `seg1_div` consecutive batches (the ReferenceNet
 *           bank repeated over frames, mutual_self_attention.py:238-241): batch b reads bank row
 *           b / seg1_div - seg1_skip; batches b < seg1_first_batch skip it (uc rows, :243-256).
 *           seg1_skip = leading bank rows that were never materialised: under classifier-free guidance the
 *           bank row of the uncond batch is overwritten by the uc path (:243-256) and need not exist. */
typedef struct {
  const void* q; int64_t ldq;
  const void* k0; int64_t ldk0; const void* v0t; int64_t ldv0t; int Lk0;
  const void* k1; int64_t ldk1; const void* v1t; int64_t ldv1t; int Lk1;
  int seg0_div;   /* batch b reads k0/v0t row-block b / seg0_div (1 = per-batch keys; F = a text context
                     shared by the F frames of a clip, attention.py:118-119 without the repeat) */
  int seg1_div; int seg1_first_batch; int seg1_skip;
  void* out; int64_t ldo;
  int B; int Lq; int heads; int d;
  float scale;
  int dtype;
  const int32_t* seg1_row;   /* optional DEVICE int32: when non-NULL every batch b >= seg1_first_batch reads bank row
                                seg1_row[0] (seg1_div / seg1_skip unused).  A sampling loop keeps the projected banks of a
                                whole group of timesteps resident and selects the current one by writing this word - the
                                launch parameters (hence a captured hipGraph) stay the same from step to step. */
  int causal;   /* 1: causal self-attention - query row i of each batch row attends to keys j <= i of segment 0 only (the
                   CLIP text encoder's causal mask, transformers CLIPAttention behind CLIPTextTransformer._build_causal_attention_mask;
                   the CLIPTextModel that magicanimate/pipelines/animation.py:75-76 loads).  Needs Lq == Lk0 and no segment 1
                   (k1 and seg1_row NULL), else EMO_ERR_UNSUPPORTED.  0 (a zeroed struct): no mask, as before. */
} emo_attention_params;
int emo_attention(const emo_attention_params* p, void* stream);
/* Host-only: what emo_attention would launch for p - plan = (head-dim class in 16-byte chunks, loader rounds per tile, KV ring depth,
 * q tiles walked per block (> 1 = the resident-context variant), causal).  Runs emo_attention's argument checks and returns their
 * status; launches nothing and touches no device memory (the pointers of p only need to be non-NULL where emo_attention wants them). */
int emo_attention_plan(const emo_attention_params* p, int plan[5]);

/* Temporal self-attention of the AnimateDiff motion module (motion_module.py:275-334): tokens
 * "(b f) d c -> (b d) f c"; qkv rows are [(b*F+f)*HW + pix][3*C] (q|k|v), output [(b*F+f)*HW+pix][C].
 * F <= 32.  The transposes are folded into the indexing.
 * Also the `attn_temp` branch of BasicTransformerBlock(unet_use_temporal_attention=True) (attention.py:235-246,309-318;
 * mutual_self_attention.py:274-282): the same regrouping with the block's own heads / head dim and no positional encoding.  The scores
 * accumulate and the softmax runs in f32 for every dtype (only the probabilities are rounded to the value dtype, orig_attention.py:677),
 * so upcast_attention=True (orig_attention.py:656-658) asks nothing more of the kernel. */
int emo_temporal_attention(const void* qkv, int64_t ldqkv, void* out, int64_t ldo, int B, int F, int HW,
                           int heads, int d, float scale, int dtype, void* stream);

/* ---- sampler -------------------------------------------------------------------------------
 * Fused window-average + classifier-free guidance + one scheduler step (EMOAnimationPipeline.py:812-817) - DDIM, DDPM,
 * DPM-Solver++ 2M, Euler, Euler-ancestral, LMS - as a linear form with up to three earlier model outputs, all f32 over
 * n = C*F*HW elements.  Element (c, f, p) has index (c*F + f)*HW + p; counter holds one f32 per frame [F], broadcast over
 * (C, H*W):
 *   eps   = uc + guidance_scale*(c - uc) on noise_pred / counter   (noise_pred f32 [2][n] = (uc, c))
 *   d     = a*x + b*eps                              (the solver's model output: eps, or x0)
 *   x'    = c_x*x + c[0]*d + sum_{k=1..3, slot[k] >= 0} c[k]*history[slot[k]] + c_noise*z
 *   history[slot[0]] = d  (slot[0] >= 0);  latents = x';  lat_in = s_next*x' (lat_in non-null);  eps_out = eps (non-null)
 * guidance_scale <= 1 is the reference's "no classifier-free guidance" (:622 `do_classifier_free_guidance =
 * guidance_scale > 1.0`): noise_pred is then [1][n] and eps = noise_pred / counter.
 * history: ring of EMO_SCHED_RING planes of n floats; slot[0] must differ from every slot read.  z = counter-based N(0,1)
 * keyed by (seed, step, element): every rank draws the same bits.  scale_only != 0: lat_in = s_next*latents, nothing else
 * is read or written (the model input of the first step that runs). */
#define EMO_SCHED_RING 4
typedef struct {
  float guidance_scale;
  float a, b;
  float c_x;
  float c[4];
  int slot[4];
  float c_noise;
  float s_next;
  uint32_t seed, step;
  int scale_only;
} emo_sched_step_params;
int emo_sched_step(const float* noise_pred, const float* counter, float* latents, float* history, float* lat_in, float* eps_out,
                   int C, int F, int HW, const emo_sched_step_params* p, void* stream);
/* noise_pred[branch, :, frames[j]] += pred rows; counter[frames[j]] += 1 (EMOAnimationPipeline.py:790-794).
 * pred: rows ((j) h w, ld) in dtype for ONE branch of ONE window; frames: device int32 [nf].  The frames of a
 * window must be distinct; a position with frames[j] < 0 is skipped (a wrapped window of the uniform scheduler with
 * context_stride > 1 can list a frame twice: `noise_pred[:, :, c] = noise_pred[:, :, c] + pred` then keeps ONE
 * occurrence - the host marks the others negative). */
int emo_accumulate_window(const void* pred, int ld, float* noise_pred_branch, float* counter, const int32_t* frames,
                          int nf, int C, int F, int HW, int add_counter, int dtype, void* stream);

/* ---- EMO conditioning ----------------------------------------------
 * emo_act: y = act(x), kind 0 SiLU | 1 ReLU | 2 tanh | 3 erf-GELU | 4 quick_gelu x * sigmoid(1.702 x) over n contiguous elements
 *   (the ReLU / tanh of Net.py:214-218,246 and train_stage_3_speedlayers.py:36-40,66-73; GELU: the activation of the wav2vec2 encoder
 *   Net.py:611-612 loads - transformers Wav2Vec2FeedForward / conv layers; quick_gelu: transformers QuickGELUActivation, the MLP
 *   activation of the SD-1.x CLIP text encoder, CLIPMLP behind EMOAnimationPipeline.py:226-229).  f32 math, rounded once.
 * emo_speed_encode: SpeedEncoder.encode_speed (Net.py:231-247): out[b,i] = tanh((v[b]-centers[i])/radii[i]*3).
 * emo_speed_bucket: SpeedController.map_speed_to_bucket (train_stage_3_speedlayers.py:42-47), INT bit-exact:
 *   idx[b] = argmin_i |v[b] - centers[i]| (first minimum on ties).
 * emo_gather_rows: nn.Embedding lookup out[b,:] = table[idx[b],:].
 * emo_add_rowbias: y[m,:] = x[m,:] + rb[m / rows_per_batch,:] (EMOStage3.forward combine, :268-269). */
int emo_act(const void* x, void* y, int64_t n, int kind, int dtype, void* stream);
int emo_speed_encode(const float* v, const float* centers, const float* radii, void* out, int B, int nb, int dtype, void* stream);
int emo_speed_bucket(const float* v, const float* centers, int32_t* idx, int B, int nb, void* stream);
int emo_gather_rows(const void* table, const int32_t* idx, void* out, int B, int D, int rows, int dtype, void* stream);
int emo_add_rowbias(const void* x, int ldx, const void* rb, int ldr, void* y, int ldy, int64_t M, int C, int rows_per_batch,
                    int dtype, void* stream);
/* emo_text_embed: CLIPTextEmbeddings.forward (transformers; the text encoder of EMOAnimationPipeline.py:226-229) in one launch:
 *   out[b*L + l, :] = tok_table[ids[b*L + l], :] + pos_table[l, :]   (inputs_embeds + position_embedding(arange(L))).
 *   ids: device int32 [B*L], each in [0, V) - checked by the caller before upload (an out-of-range id is clamped here, never read
 *   out of bounds); tok_table [V][D], pos_table [P][D] with L <= P, out [B*L][D], all in dtype; the sum in f32, rounded once. */
int emo_text_embed(const int32_t* ids, const void* tok_table, const void* pos_table, void* out, int B, int L, int D, int V, int P,
                   int dtype, void* stream);

/* ---- either side of the loop ----------------------------------------------------
 * emo_softmax_rows: y[m, :] = softmax(scale * x[m, :]) over N columns - the VAE mid-block attention (one head of 512
 *   channels; diffusers AutoencoderKL behind EMOAnimationPipeline.py:291-307,402-414) as Q.K^T GEMM -> this -> P.V GEMM.
 * emo_audio_windows: Wav2VecFeatureExtractor.extract_features_from_wav (Net.py:649-667): out[t][j][:] = feats[t-m+j][:],
 *   zero where t-m+j falls outside [0, T); out is [T][m+n+1][D].  Bit-exact (a copy).
 * emo_rows_to_video: rows ((b f) h w, ld) -> (B, C, F, H, W) f32 with y = clamp(x*mul + add, lo, hi): the
 *   `(video / 2 + 0.5).clamp(0, 1)` of decode_latents (EMOAnimationPipeline.py:303-306). */
int emo_softmax_rows(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t M, int N, float scale, int dtype, void* stream);
int emo_audio_windows(const void* feats, void* out, int T, int D, int m, int n, int dtype, void* stream);
int emo_rows_to_video(const void* x, int64_t ld, float* y, int B, int C, int F, int HW, float mul, float add, float lo, float hi,
                      int dtype, void* stream);
/* emo_channelnorm: per-channel normalisation over the S rows of a sequence, y = act((x - mean_c) * rstd_c * gamma_c + beta_c), act 0 none |
 * 1 erf-GELU: nn.GroupNorm(C, C) on (1, C, T) - the first conv layer of the wav2vec2 feature extractor behind
 * Wav2VecFeatureExtractor (Net.py:607-648; transformers Wav2Vec2GroupNormConvLayer).  workspace: emo_channelnorm_workspace_bytes(S, C). */
size_t emo_channelnorm_workspace_bytes(int64_t S, int C);
int emo_channelnorm(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy, int64_t S, int C, float eps,
                    int act, void* workspace, int dtype, void* stream);
/* emo_wav_conv0_ln_act: the whole first feature-encoder layer of the layer-norm wav2vec2 family behind Wav2VecFeatureExtractor
 *   (Net.py:607-648 -> transformers Wav2Vec2LayerNormConvLayer with one input channel: Conv1d(1, C, k, stride, bias) -> LayerNorm(C)
 *   -> GELU) straight from the waveform, with no window matrix and no pre-norm tensor in memory:
 *       y[t][c] = act(LN_c(bias[c] + sum_{j<k} w[c][j] * wave[t * stride + j])),   t in [0, (n - k) / stride + 1)
 *   wave f32 [n]; w f32 [C][k] and bias / gamma / beta f32 [C] (the f32 masters, never rounded to `dtype`); y rows [T0][ldy] in
 *   `dtype`; act 0 none | 1 erf-GELU.  Taps accumulate in ascending j with fmaf from the bias, statistics are two-pass f32, the result
 *   is rounded once.  Served: C % 8 == 0, C <= 1024, 1 <= k <= 16, stride >= 1, n >= k; anything else is EMO_ERR_UNSUPPORTED before
 *   any launch.
 * emo_wav_conv0_ln_act_plan (host only): that shape check without a launch, and on EMO_OK plan = rows T0, lanes per row, 8-channel
 *   vectors per lane, compiled tap count, row groups per wavefront, grid.  Writes nothing on a refusal. */
int emo_wav_conv0_ln_act_plan(int64_t n, int C, int k, int stride, int64_t plan[6]);
int emo_wav_conv0_ln_act(const float* wave, int64_t n, const float* w, const float* bias, const float* gamma, const float* beta, void* y,
                         int64_t ldy, int C, int k, int stride, float eps, int act, int dtype, void* stream);
/* emo_audio_resample: the sf.read / librosa.resample / mean(axis=1) of Wav2VecFeatureExtractor.extract_features_from_wav (Net.py:627-640)
 *   as one pass - channel downmix + rational polyphase resampling, f32.  With g = gcd(in_rate, out_rate), up = out_rate / g,
 *   down = in_rate / g, half = 10 * max(up, down) and f32 taps h[-half .. half] (a Kaiser-windowed sinc designed on the host in f64,
 *   emote_hack_amd.audio_io.resample_taps), global output sample n is
 *     y[n] = sum_j h[n * down - j * up] * x[j]   over every j with |n * down - j * up| <= half, accumulated in ASCENDING j by fmaf,
 *     x[j] = (in[j][0] + ... + in[j][channels - 1]) / channels, summed in channel order; x[j] = 0 outside the slice.
 *   in: interleaved frames [n_in][channels] holding GLOBAL frames in_start .. in_start + n_in - 1; out[i] = y[out_start + i],
 *   i < n_out.  A long recording is resampled in pieces: a sample has the same bits whichever piece produced it, given a slice that
 *   covers its taps.  All sample indices are 64-bit.  taps: the phase table [up][tpp], tpp = emo_audio_resample_taps_per_phase(up, half)
 *   = ceil(half / up) + floor(half / up) + 1, entry [p][c] = h[p + up * (c - ceil(half / up))] (0 where that lies outside
 *   +-half); n_taps = up * tpp is checked.  up, down <= 65536, channels <= 64.
 * emo_waveform_normalize: the utterance normalisation of `self.processor(...)` (Net.py:639; Wav2Vec2FeatureExtractor do_normalize):
 *   y = (x - mean) / sqrt(var + eps) over n f32 samples, population variance, TWO passes (the mean, then the centred squares - a
 *   recording with a DC offset does not cancel).  Block partials in the workspace are combined in index order in f64: the result is
 *   bit-reproducible from run to run.  workspace_bytes must be >= emo_waveform_normalize_workspace_bytes(n), else EMO_ERR_BAD_SHAPE.
 *   y must not alias x. */
int emo_audio_resample_taps_per_phase(int up, int half);
int emo_audio_resample(const float* in, int64_t in_start, int64_t n_in, int channels, const float* taps, int64_t n_taps, int up, int down,
                       int half, float* out, int64_t out_start, int64_t n_out, void* stream);
size_t emo_waveform_normalize_workspace_bytes(int64_t n);
int emo_waveform_normalize(const float* x, float* y, int64_t n, float eps, void* workspace, size_t workspace_bytes, void* stream);
/* FaceLocator (Net.py:819-855): nn.MaxPool2d(2, 2) over NHWC rows (H, W -> H/2, W/2), and
 * F.interpolate(logits, size=(Ho, Wo), mode='bilinear', align_corners=False) of rows ((n) h w, ld) into (n, C, Ho, Wo) f32. */
int emo_maxpool2x2(const void* x, int64_t ldx, void* y, int64_t ldy, int n_img, int H, int W, int C, int dtype, void* stream);
int emo_bilinear_to_nchw(const void* x, int64_t ld, float* y, int n_img, int C, int h, int w, int Ho, int Wo, int dtype, void* stream);
/* emo_interp_frames: `interpolate_latents` (EMOAnimationPipeline.py:479-512) with the slerp / linear of magicanimate/utils/util.py:125-138
 *   for a whole clip in TWO launches and no host read.  x f32 [B][C][F][HW] contiguous, F >= 2; y f32 [B][C][(F-1)*k + 1][HW], k >= 2.
 *   Output frame j (p = j / k, r = j % k): r == 0 is input frame p copied bit for bit; otherwise w0 * frame p + w1 * frame p+1 at t = r / k.
 *   A frame is the whole x[:, :, i] slice as ONE vector of B*C*HW values (batch included, as upstream).
 *     method 0 (linear): w0 = 1 - t, w1 = t.
 *     method 1 (slerp):  d = <v0, v1> / (|v0| |v1|); |d| > dot_threshold (either sign: upstream takes abs) -> the linear weights; else
 *                        w = acos(d), w0 = sin((1 - t) w) / sin(w), w1 = sin(t w) / sin(w).  A zero-norm frame makes d NaN, and the frames
 *                        strictly between that pair NaN (upstream's behaviour, kept); nothing else is touched.
 *   Pass 1: block (pair, slice of the frame) -> f32 partials of <v0, v1>, |v0|^2, |v1|^2 in the workspace.  Pass 2: every block that
 *   writes an interpolated frame re-reduces its pair's partials in index order in f64, derives w0 / w1 (f64, rounded once to f32) and
 *   writes fmaf(w0, v0, w1 * v1).  No atomics, no counters: the same bits every run; the threshold branch is taken on the device.
 *   16-byte accesses when HW % 4 == 0 and x, y are 16-byte aligned, scalar otherwise.  workspace_bytes must be >=
 *   emo_interp_frames_workspace_bytes(B, C, F, HW), else EMO_ERR_BAD_SHAPE; so are F < 2, k < 2, an unknown method and y overlapping x.
 * emo_rows_to_frames_u8: decoded NHWC rows ((b f) h w, ld >= C) in dtype -> packed uint8 [B][F][HW][C]: the `/ 2 + 0.5`, `clamp(0, 1)` of
 *   decode_latents followed by the `(x * 255).astype(uint8)` of save_videos_grid (magicanimate/utils/util.py:21-33), per element
 *     t = fminf(fmaxf(fmaf(x, mul, add), lo), hi);  y = (uint8_t)(t * 255.0f)      (x widened exactly to f32; truncation toward zero)
 *   Columns >= C of a wide row are never read; the output is dense, stored as 16-byte vectors / dwords with a bytewise ragged tail. */
size_t emo_interp_frames_workspace_bytes(int B, int C, int F, int64_t HW);
int emo_interp_frames(const float* x, float* y, int B, int C, int F, int64_t HW, int k, int method, float dot_threshold, void* workspace,
                      size_t workspace_bytes, void* stream);
int emo_rows_to_frames_u8(const void* x, int64_t ld, uint8_t* y, int B, int C, int F, int HW, float mul, float add, float lo, float hi,
                          int dtype, void* stream);

/* ---- Motion-JPEG output: the device half of the writer that stands in for `imageio.mimsave` at the end of `save_videos_grid`
 * (magicanimate/utils/util.py:21-33).  Baseline sequential JPEG, ITU-T T.81; the host half (tables, markers, byte stuffing, the AVI
 * container) is emote_hack_amd/video_io.py.
 * emo_jpeg_blocks (util.py:21-33; T.81 A.3.3 FDCT, A.3.4 quantisation, A.3.6 zig-zag, A.2.3 / A.2.4 interleaved MCUs): packed uint8 RGB
 *   frames [n][H][W][3], any H, W in 1 .. 65535 -> quantised coefficients int16 [n][mcu_rows * mcu_cols][6][64], mcu_rows = ceil(H / 16),
 *   mcu_cols = ceil(W / 16); MCUs in raster order.  4:2:0: the six blocks of a 16x16 MCU in scan order Y00 Y01 Y10 Y11 Cb Cr (Yrc = the
 *   8x8 luma block at row r, column c of the MCU); 64 coefficients per block in ZIG-ZAG order, the DC term UNDIFFERENCED.  Pixels beyond
 *   the right and the bottom edge repeat the edge pixel.  All arithmetic in f32 (sums may be fused multiply-adds):
 *     Y  =  0.299 R + 0.587 G + 0.114 B - 128        Cb = -0.168736 R - 0.331264 G + 0.5 B        Cr = 0.5 R - 0.418688 G - 0.081312 B
 *     chroma sample = 0.25 * ((a + b) + (c + d)) over each 2x2 of the (edge-replicated) full-resolution Cb / Cr
 *     S[v][u] = sum_y sum_x C[v][y] C[u][x] s[y][x],  C[u][x] = 0.5 c(u) cos((2x + 1) u pi / 16), c(0) = 1 / sqrt 2, c(u > 0) = 1
 *       (rows first, then columns; C rounded once to f32)
 *     coefficient = (int16) rintf(S[v][u] / q[v * 8 + u])
 *   quant: device uint16 [2][64], luma then chroma, NATURAL order (a 0 entry is taken as 1).  With 8-bit samples |S| <= 1024, so DC
 *   differences stay inside size category 11 and AC coefficients inside category 10 for every q >= 1.  coefs 4-byte aligned.
 * emo_jpeg_count_bits (T.81 F.1.2 Huffman encoding procedures, F.1.2.1 DC, F.1.2.2 AC): the exact coded size in bits of every block,
 *   counts int32 [n][n_mcu * 6].  DC: the difference from the previous block of the same component in the SAME frame (predictor 0 at every
 *   frame's start, F.1.1.5.1), coded as its size category followed by that many magnitude bits (a negative value v as v - 1).  AC: one
 *   run / size symbol per non-zero coefficient, one ZRL (0xF0) per 16 zeros of a longer run, EOB (0x00) when the last coefficient is zero.
 *   huff: device uint32 [4][256] in the order DC luma, AC luma, DC chroma, AC chroma, entry [symbol] = code length << 16 | code
 *   (length 0: the symbol has no code and contributes nothing - the tables must cover categories 0 .. 11 and every AC symbol).
 * emo_jpeg_emit_bits (T.81 F.1.2, bit order of F.1.2.3 / figure F.1.2: most significant bit first): the codes counted above, block b
 *   starting at bit bit_offsets[b] (int64 [n][n_mcu * 6], counted from the first bit of out) - the caller lays the blocks of a frame end
 *   to end and starts every frame on a byte.  The stream is UNSTUFFED and unpadded: the host adds the 0x00 after every 0xFF and the
 *   1-bits that fill the last byte.  out must be zeroed up to the last stream byte, 4-byte aligned, out_bytes a multiple of 4: codes
 *   are OR-ed in as byte-swapped 32-bit words (atomicOr - blocks share words; OR commutes, so the result is the same every run), a word
 *   is touched only where a code has a 1-bit in it, and never at or beyond out_bytes.
 * emo_jpeg_count_bits_ri / emo_jpeg_emit_bits_ri (T.81 B.2.4.4 DRI, E.1.4 restart intervals, F.1.1.5.1: "at the beginning of each
 *   restart interval, the prediction for the DC coefficient is initialized to 0"): the two entries above for a scan with a restart
 *   interval of restart_mcus > 0 MCUs.  The one difference: the DC predictor is 0 at the first MCU of every interval (MCUs 0, Ri, 2 Ri, ...
 *   of each frame), not of every frame alone.  The caller starts every interval on a byte; the host pads each, stuffs it and puts the
 *   RSTm markers between them.  restart_mcus >= n_mcu gives what the entries above give. */
int emo_jpeg_blocks(const uint8_t* frames, int16_t* coefs, int n, int H, int W, const uint16_t* quant, void* stream);
int emo_jpeg_count_bits(const int16_t* coefs, int32_t* counts, int n, int n_mcu, const uint32_t* huff, void* stream);
int emo_jpeg_emit_bits(const int16_t* coefs, const int64_t* bit_offsets, uint8_t* out, int64_t out_bytes, int n, int n_mcu,
                       const uint32_t* huff, void* stream);
int emo_jpeg_count_bits_ri(const int16_t* coefs, int32_t* counts, int n, int n_mcu, int restart_mcus, const uint32_t* huff, void* stream);
int emo_jpeg_emit_bits_ri(const int16_t* coefs, const int64_t* bit_offsets, uint8_t* out, int64_t out_bytes, int n, int n_mcu,
                          int restart_mcus, const uint32_t* huff, void* stream);

/* ---- Animated GIF output: the device half of the second container `imageio.mimsave(path, frames, fps)` is used for at the end of
 * `save_videos_grid` (magicanimate/utils/util.py:33).  GIF89a; the host half (median cut over the histogram, the header, the colour
 * tables, the extensions, the sub-blocks of at most 255 bytes) is emote_hack_amd/video_io.py.  The kernels live in csrc/gif_out.hip.
 * emo_gif_histogram (util.py:33; the colours a GIF89a colour table, section 19 / 21, is chosen from): packed uint8 RGB frames
 *   [n][H][W][3] -> hist uint64 [per_frame ? n : 1][32768][4]: per bin (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3) the pixel count and the
 *   sums of R, G and B.  The figures are ADDED to hist (the caller zeroes it) with 64-bit integer atomics only, so the result does not
 *   depend on the order of execution.  Exact without wrap-around while n * H * W <= 2^55 (255 * 2^55 < 2^63), which the entry enforces;
 *   H, W in 1 .. 65535 (the logical screen descriptor, section 18, holds 16 bits).
 * emo_gif_map (util.py:33; GIF89a section 22, table based image data: one colour table index per pixel): indices uint8 [n][H][W] =
 *   the k in 0 .. n_colors - 1 that minimises (R - pr[k])^2 + (G - pg[k])^2 + (B - pb[k])^2 on the 8-bit integers, the LOWEST k on a
 *   tie; an exact search.  palettes uint8 [per_frame ? n : 1][256][3]; entries from n_colors up are never read.  dither_strength 0:
 *   none; 1 .. 128: before the search every channel v becomes clamp(v + floor((2 * B8[y & 7][x & 7] - 63) * strength / 128), 0, 255), B8
 *   the 8x8 Bayer matrix of B1 = [[0]], B2k = [[4B, 4B + 2], [4B + 3, 4B + 1]].
 * emo_gif_lzw_count / emo_gif_lzw_emit (util.py:33; GIF89a Appendix F, variable-length-code LZW compression, with code size 8:
 *   Clear = 256, End of Information = 257, first free code 258, codes of 9 .. 12 bits packed least significant bit first).  A frame is
 *   cut into strips of strip_rows rows (the last may be shorter; strip_rows >= H: one strip), at most 2^26 pixels each.  Every strip
 *   is coded from an empty dictionary at 9 bits and is laid out as
 *     [Clear, 9 bits: the frame's first strip only]  codes ...  Clear (End of Information behind the frame's last strip)
 *   so its bits depend on its own pixels only.  The width of a code is the decoder's: it grows when the decoder's next free code
 *   reaches 1 << width, the closing Clear / End of Information included.  Code 3838 behind a Clear finds the table full (4096): a Clear
 *   follows it and the dictionary starts again.
 *   emo_gif_lzw_count walks every strip once: codes uint16 [n * strips][emo_gif_lzw_codes_per_strip(H, W, strip_rows)] takes the
 *   strip's codes (Clears inside the strip included, the opening and the closing code not), n_codes int32 [n * strips] their number,
 *   bits int32 [n * strips] the strip's exact size in bits, opening and closing code included.
 *   emo_gif_lzw_emit ORs them into out at bit_offsets[strip] (int64 [n * strips], from the first bit of out: the caller lays a
 *   frame's strips end to end and starts every frame on a byte).  out must be zeroed, 4-byte aligned, out_bytes a multiple of 4:
 *   32-bit atomicOr, since strips and frames share words; a word is touched only where a code has a 1-bit in it and never at or beyond
 *   out_bytes. */
int emo_gif_histogram(const uint8_t* frames, uint64_t* hist, int n, int H, int W, int per_frame, void* stream);
int emo_gif_map(const uint8_t* frames, const uint8_t* palettes, uint8_t* indices, int n, int H, int W, int n_colors, int per_frame,
                int dither_strength, void* stream);
int64_t emo_gif_lzw_codes_per_strip(int H, int W, int strip_rows);
int emo_gif_lzw_count(const uint8_t* indices, uint16_t* codes, int32_t* n_codes, int32_t* bits, int n, int H, int W, int strip_rows,
                      void* stream);
int emo_gif_lzw_emit(const uint16_t* codes, const int32_t* n_codes, const int64_t* bit_offsets, uint8_t* out, int64_t out_bytes, int n,
                     int H, int W, int strip_rows, void* stream);

/* ---- PNG / APNG output: the device half of the lossless writer, what `save_images_grid` (magicanimate/utils/util.py:35-41,
 * `Image.fromarray(grid).save(path)`) and the numbered stills of ExtractFrames.py:51 ask Pillow for.  PNG is ISO/IEC 15948 (RFC 2083;
 * filtering: its section 6), the image data a zlib stream (RFC 1950) holding ONE deflate block with dynamic Huffman codes (RFC 1951
 * 3.2.7) per frame.  The host half (the Huffman tables and the block header, the combination of the rows' checksums, the chunks and
 * their CRCs) is emote_hack_amd/video_io.py.  The kernels live in csrc/png_out.hip.  Shapes common to all entries: n, H, W >= 1, C in
 * {1, 3, 4} (grey, RGB, RGBA at bit depth 8), a filtered scanline has R = 1 + W * C bytes, and H * R <= 2^31 - 1.
 * emo_png_filter (PNG section 6): packed uint8 frames [n][H][W][C] -> filtered uint8 [n][H][R]: per scanline the filter type byte t and
 *   then, for byte j = 0 .. W * C - 1 of the raw row, (x - pred_t) mod 256 with x = raw[y][j], a = raw[y][j - C] (0 where j < C),
 *   b = raw[y - 1][j] (0 in the frame's row 0), c = raw[y - 1][j - C] (0 where either is) and pred_0 = 0 (None), pred_1 = a (Sub),
 *   pred_2 = b (Up), pred_3 = floor((a + b) / 2) (Average), pred_4 = Paeth: with p = a + b - c, pa = |p - a|, pb = |p - b|,
 *   pc = |p - c|, it is a if pa <= pb and pa <= pc, else b if pb <= pc, else c.  Every row is computed from the RAW rows.  filter 0 .. 4
 *   forces t for all rows; filter 5 picks per row the t with the smallest sum over the row's W * C filtered bytes v of min(v, 256 - v)
 *   (libpng's heuristic), the LOWEST t on a tie.  adler uint32 [n][H][2] takes per row (s1, s2) = the Adler-32 state (RFC 1950 8.2)
 *   after the row's R filtered bytes d_0 .. d_(R-1) from the state (1, 0): s1 = (1 + sum d_i) mod 65521, s2 = (R + sum (R - i) d_i)
 *   mod 65521.  The host chains them: a stream in state (s1, s2) followed by a row (r1, r2) of R bytes is in
 *   ((s1 + r1 - 1) mod 65521, (s2 + r2 + R (s1 - 1)) mod 65521).
 * emo_png_lz_count: a frame's filtered bytes are cut into strips of strip_rows scanlines (the last may be shorter; strip_rows > H
 *   counts as H); a strip holds at most 65535 bytes, more is refused.  Each strip, a byte string s of P bytes, is tokenised on its own
 *   by a deterministic greedy LZ77 over a table T of 4096 strip offsets, all empty at the strip's start.  From pos = 0, while pos < P:
 *   if pos + 3 <= P, then h = ((s[pos] | s[pos + 1] << 8 | s[pos + 2] << 16) * 0x9E3779B1 mod 2^32) >> 20, cand = T[h], T[h] = pos; if
 *   cand is not empty and pos - cand <= 32768, L = the number of leading bytes on which s[cand ..] and s[pos ..] agree, counted up to
 *   min(258, P - pos) (the two ranges may overlap); if L >= 3 the token is the match (length L, distance pos - cand) and pos += L.  In
 *   every other case the token is the literal s[pos] and pos += 1.  The table is read and written at token starts only, and one slot
 *   is probed: a slot taken by another triple with the same hash gives L < 3 and a literal.
 *   tokens uint32 [n * strips][emo_png_tokens_per_strip(H, W, C, strip_rows)] (= the bytes of a full strip: one token per byte at
 *   worst) takes them packed as length << 16 | distance for a match (3 .. 258, 1 .. 32768) and as the byte alone for a literal (bits
 *   16 .. 31 zero); entries behind a strip's tokens are not written.  n_tokens int32 [n * strips] their number.  hist uint32 [n][320]:
 *   the symbols of RFC 1951 3.2.5 are ADDED with integer atomics (the caller zeroes it): slot v for a literal v, slot 257 .. 285 for a
 *   match's length symbol, slot 288 + d for its distance symbol d = 0 .. 29, and slot 256 once per frame, the end-of-block.
 * emo_png_deflate_bits: codes uint32 [n][320] holds per frame and per slot of hist `code length << 16 | the canonical code with its
 *   bits reversed` (length 1 .. 15; packed least significant bit first, a reversed code is on the wire most significant bit first as
 *   RFC 1951 3.1.1 wants).  bits int32 [n * strips] = the exact size of every strip's tokens: per literal its code's length, per match
 *   the length symbol's code, its extra bits, the distance symbol's code, its extra bits.  Block header and end-of-block are not in it.
 * emo_png_deflate_emit ORs every strip's tokens in that order - codes, then extra bits as plain integers above them - into out from
 *   bit_offsets[strip] (int64 [n * strips], from the first bit of out) on, least significant bit first.  out must be zeroed, 4-byte
 *   aligned, out_bytes a multiple of 4: 32-bit atomicOr, since strips and frames share words; a word is touched only where a token
 *   has a 1-bit in it and never at or beyond out_bytes.  A strip whose n_tokens is outside 0 .. the buffer's entries writes nothing.
 *   THE HOST places everything else after the one copy back: per frame, starting on a byte, the zlib header 78 01, the block header
 *   (BFINAL = 1, BTYPE = 2, HLIT, HDIST, HCLEN, the code lengths) right behind it, the strips' tokens end to end behind that (the
 *   caller's bit_offsets leave exactly that room), the end-of-block code, zero bits up to the next byte and the Adler-32 as s2 << 16 |
 *   s1, big-endian. */
int emo_png_filter(const uint8_t* frames, uint8_t* filtered, uint32_t* adler, int n, int H, int W, int C, int filter, void* stream);
int64_t emo_png_tokens_per_strip(int H, int W, int C, int strip_rows);
int emo_png_lz_count(const uint8_t* filtered, uint32_t* tokens, int32_t* n_tokens, uint32_t* hist, int n, int H, int W, int C,
                     int strip_rows, void* stream);
int emo_png_deflate_bits(const uint32_t* tokens, const int32_t* n_tokens, const uint32_t* codes, int32_t* bits, int n, int H, int W, int C,
                         int strip_rows, void* stream);
int emo_png_deflate_emit(const uint32_t* tokens, const int32_t* n_tokens, const uint32_t* codes, const int64_t* bit_offsets, uint8_t* out,
                         int64_t out_bytes, int n, int H, int W, int C, int strip_rows, void* stream);

/* ---- PNG / APNG input: the device half of the reader of what the block above writes and of what Pillow and libpng write: the numbered
 * stills of ExtractFrames.py:51, the portrait `Image.open` reads (EMOAnimationPipeline.py:688, animation.py:185, inference.py:41), lossless
 * pose / depth / mask clips.  PNG is ISO/IEC 15948: section 7 the scanline serialisation, section 9 filtering (9.2 the filter types, 9.3
 * Average, 9.4 Paeth), section 10 the image data as a zlib stream (RFC 1950) of deflate blocks (RFC 1951).  The host half (signature,
 * chunks and CRCs, IHDR / acTL / fcTL / fdAT, the zlib header, the Adler-32 trailer) is emote_hack_amd/video_io.py.  The kernels live in
 * csrc/png_in.hip.  Shapes common to both entries: n, H, W >= 1, C in {1, 2, 3, 4} (grey, grey + alpha, RGB, RGBA at bit depth 8, no
 * interlace), a filtered scanline has R = 1 + W * C bytes, and H * R <= 2^31 - 1; anything else is EMO_ERR_BAD_SHAPE before any launch.
 * emo_png_inflate (RFC 1951): the RAW deflate streams of n frames - the host has taken off and checked the two zlib header bytes (RFC
 *   1950 2.2) and the four of the Adler-32 - lie in `streams` (stream_bytes bytes, a multiple of 4, 4-byte aligned; bytes behind the last
 *   frame are never used), frame i in bytes offsets[i] .. offsets[i + 1] (int64 [n + 1], 8-byte aligned).  Output: filtered uint8
 *   [n][H * R], produced int32 [n] (the bytes the frame gave, at most H * R) and status int32 [n].  All three block types (3.2.4 stored,
 *   3.2.6 fixed, 3.2.7 dynamic), any number of blocks, a stored block from any bit position.  Status:
 *     EMO_PNG_OK            the final block ended with exactly H * R bytes produced (bytes behind it in the frame are not looked at)
 *     EMO_PNG_BAD_BLOCK     block type 3
 *     EMO_PNG_BAD_STORED    a stored block's NLEN is not the complement of its LEN
 *     EMO_PNG_BAD_LENGTHS   a dynamic block's code lengths, decided as zlib's inflate decides: HLIT above 286 or HDIST above 30; an
 *                           over-subscribed set; an incomplete set - other than a set of one single code of one bit (a distance set of
 *                           one code), or no distance code at all, which are accepted, never for the code-length code -; a repeat (16)
 *                           with no length in front of it; a repeat that runs past HLIT + HDIST (one that crosses from the literal /
 *                           length lengths into the distance lengths is allowed); no code for the end-of-block symbol
 *     EMO_PNG_BAD_SYMBOL    literal / length symbol 286 or 287, distance symbol 30 or 31, or 15 bits that begin no code of the set
 *     EMO_PNG_BAD_DISTANCE  a distance that reaches in front of the frame's first byte
 *     EMO_PNG_PAST_END      the frame's bytes end inside a block (a cut file, an empty frame; offsets that run backwards or leave the
 *                           buffer are taken as an empty frame)
 *     EMO_PNG_OVERFLOW      a literal, a match or a stored block would carry the output past H * R (none of it is written)
 *     EMO_PNG_SHORT         the final block ended before H * R bytes
 *   A frame with an error stops there: what it produced up to then is in filtered, produced says how much; other frames are not
 *   touched.  One wavefront per frame.  Bounds: every read of the streams is masked to the frame's own bytes (past them the reader sees
 *   zeros and the frame ends with EMO_PNG_PAST_END), every write to filtered is masked to the frame's own H * R, every table index to
 *   its table; every loop is counted by input bits or output bytes - each turn takes at least one bit or ends the frame.  A damaged
 *   file gives a status, never a hang or an access outside the buffers.
 * emo_png_unfilter (PNG 9.2 - 9.4): filtered [n][H][R] -> packed uint8 frames [n][H][W][C]: per scanline, t its first byte, byte j of
 *   the raw row is (filtered[1 + j] + pred_t) mod 256 with the pred_t of emo_png_filter over the RECONSTRUCTED a, b, c (a = raw[y][j - C],
 *   b = raw[y - 1][j], c = raw[y - 1][j - C], 0 where there is none).  adler uint32 [n][H][2]: per row the Adler-32 pair of its R
 *   filtered bytes in exactly the form emo_png_filter writes, for the host to combine and compare with the stream's trailer.  status
 *   int32 [n]: EMO_PNG_OK, or EMO_PNG_BAD_FILTER for a type byte above 4 - the frame stops at the band of 64 rows that holds it (rows
 *   in front of the band are written, their Adler pairs too).  A row holds at most 98304 bytes (W * C), more is EMO_ERR_BAD_SHAPE.
 *   One wavefront per frame; reads and writes stay inside the frame's own rows whatever the bytes say. */
enum { EMO_PNG_OK = 0, EMO_PNG_BAD_BLOCK = 1, EMO_PNG_BAD_STORED = 2, EMO_PNG_BAD_LENGTHS = 3, EMO_PNG_BAD_SYMBOL = 4, EMO_PNG_BAD_DISTANCE = 5,
       EMO_PNG_PAST_END = 6, EMO_PNG_OVERFLOW = 7, EMO_PNG_SHORT = 8, EMO_PNG_BAD_FILTER = 9 };
int emo_png_inflate(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, uint8_t* filtered, int32_t* produced,
                    int32_t* status, int n, int H, int W, int C, void* stream);
int emo_png_unfilter(const uint8_t* filtered, uint8_t* frames, uint32_t* adler, int32_t* status, int n, int H, int W, int C, void* stream);

/* ---- GIF input: the device half of the reader of what the GIF output block writes (`imageio.mimsave(path.gif)`, magicanimate/utils/
 * util.py:33) and of what Pillow, imageio and browsers' tools write: pose, depth and mask clips handed round as GIFs, which the
 * reference would read through `VideoReader(path).read()` (magicanimate/pipelines/animation.py:174-185).  GIF89a: section 18 the logical
 * screen descriptor, 19 the global colour table, 20 the image descriptor (sub-rectangle, interlace flag), 21 the local colour table, 22
 * the table-based image data, 23 the graphic control extension (delay, transparent index, disposal), Appendix E interlacing, Appendix F
 * the variable-length-code LZW.  The host half (header, blocks and sub-blocks, the extensions, the sticky disposal, the refusals) is
 * emote_hack_amd/video_io.py parse_gif.  The kernels live in csrc/gif_in.hip.
 * emo_gif_lzw_decode (Appendix F): the image data of n frames, sub-blocks joined by the host, lie in `streams` (stream_bytes bytes, a
 *   multiple of 4, 4-byte aligned; bytes behind the last frame are never used), frame i in bytes offsets[i] .. offsets[i + 1] (int64
 *   [n + 1], 8-byte aligned) with LZW minimum code size code_size[i] (int32 [n], 2 .. 8).  Frame i writes its colour indices in STREAM
 *   order (an interlaced frame's rows stay in pass order) to indices[out_offsets[i] .. out_offsets[i + 1]) (int64 [n + 1], 8-byte
 *   aligned): exactly w * h of them.  produced int32 [n]: how many the frame gave; status int32 [n].  With c the code size: Clear is
 *   1 << c, End of Information Clear + 1, the first free code Clear + 2; codes have c + 1 .. 12 bits, least significant bit first, and
 *   widen when the next free code reaches 1 << width.  Taken, as Pillow 12.2 takes them: a stream that does not open with a Clear; a
 *   full table (4096) with no Clear behind it - decoding goes on at 12 bits and adds no entries; several Clears in a row; the code equal
 *   to the next free one (KwKwK); no End of Information once w * h indices are out; data behind the w * h-th index (decoding stops
 *   there, a last string is cut, nothing further is looked at).  Status:
 *     EMO_GIF_OK         w * h indices decoded
 *     EMO_GIF_BAD_CODE   a code above the next free code; a code above Clear as the first code of a table (at the start, right behind
 *                        a Clear); the next free code when the table is full (no 12-bit code is); a code size outside 2 .. 8
 *     EMO_GIF_PAST_END   the frame's bytes end before w * h indices and before an End of Information (a cut file, an empty frame;
 *                        offsets that run backwards or leave the buffer are taken as an empty frame)
 *     EMO_GIF_SHORT      End of Information before w * h indices
 *   A frame with an error stops there: what it produced up to then is in indices, produced says how much; other frames are not
 *   touched.  One wavefront per frame.  Bounds: every read of the streams is masked to the frame's own bytes (past them the reader sees
 *   zeros and the frame ends with EMO_GIF_PAST_END), every write and every read of indices is masked to the frame's own w * h, every
 *   table index to 4096; the loop is counted by input bits - each turn takes at least 3 - and ends at w * h indices.  A damaged file
 *   gives a status, never a hang or an access outside the buffers.  n < 1, null or misaligned pointers and a stream_bytes that is no
 *   positive multiple of 4 are EMO_ERR_BAD_SHAPE / EMO_ERR_NULL before any launch.  offsets, code_size and out_offsets live on the
 *   device, where this entry cannot read them before a launch: the caller checks them on the host (emote_hack_amd/ops.py
 *   gif_layout_check: ascending offsets inside the stream buffer, code sizes 2 .. 8, ascending out_offsets from 0 whose sum stays at or
 *   below 2^31 - 1; the indices buffer holds out_offsets[n] bytes) - the kernel itself treats out_offsets that run backwards as a frame
 *   of no pixels and a code size out of range as EMO_GIF_BAD_CODE with nothing produced.
 * emo_gif_compose (sections 18 - 23, Appendix E): replays the n frames in file order on a canvas of H x W pixels and stores the frames
 *   asked for as packed RGB, rgb uint8 [n_out][H][W][3] (4-byte aligned).  frames int32 [n][EMO_GIF_FRAME_INTS]: left, top, w, h (the
 *   rectangle, inside the canvas), the transparent index or -1, the effective disposal 0 .. 3, the index a disposal 2 fills with, the
 *   interlace flag, the row of `tables` the frame reads, that table's entry count (1 .. 256), the output slot 0 .. n_out - 1 or -1 for a
 *   frame that is composited but not returned.  tables uint8 [n_tables][256][3], unused entries zero.  indices and out_offsets as
 *   emo_gif_lzw_decode leaves them (out_offsets[k + 1] - out_offsets[k] = w * h of frame k).  With pal_k the frame's table and t_k its
 *   transparent index: the canvas starts as pal_0[t_0], or pal_0[0] without t_0; frame 0 draws EVERY pixel of its rectangle, the
 *   transparent index too; frame k >= 1 draws pal_k[index] where index != t_k.  Immediately before frame k + 1 is drawn, frame k's
 *   rectangle is filled with pal_k[fill index] when its disposal is 2, or set back to what it held right before frame k was drawn
 *   when it is 3; 0 and 1 leave it.  (THE HOST resolves what GIF leaves open, as Pillow's GifImagePlugin does: a frame without
 *   disposal bits inherits the last non-zero ones; the fill index is t_k, else the background index, else 0; disposal 3 on frame 0
 *   becomes a fill with t_0 or nothing.)  The frame returned for k is the canvas right after frame k is drawn.  An interlaced frame of
 *   h rows reads, for its canvas row y, stream row y / 8 (y % 8 == 0), a + (y - 4) / 8 (y % 8 == 4), a + b + (y - 2) / 4 (y % 4 == 2),
 *   else a + b + c + (y - 1) / 2, with a = ceil(h / 8), b = ceil((h - 4) / 8), c = ceil((h - 2) / 4), a negative h - k counting as 0.
 *   status int32 [n], zeroed by the entry, then ORed: EMO_GIF_BAD_INDEX for a frame that draws an index at or beyond its table's entry
 *   count (the pixel takes the zero entry behind the table; one atomic per offending wavefront), EMO_GIF_BAD_FRAME for a descriptor
 *   that does not fit - a rectangle outside the canvas, w * h other than the frame's room in indices, a table row or a slot out of
 *   range: such a frame is left out, so no read or write leaves the buffers.  n, n_tables, n_out, H, W < 1, n_out > n, H or W above
 *   65535 and n_out * H * W * 3 above 2^31 - 1 are EMO_ERR_BAD_SHAPE before any launch.  One thread per 4 neighbouring pixels; no
 *   canvas goes to memory except the frames asked for. */
#define EMO_GIF_FRAME_INTS 11
enum { EMO_GIF_OK = 0, EMO_GIF_BAD_CODE = 1, EMO_GIF_PAST_END = 2, EMO_GIF_SHORT = 3, EMO_GIF_BAD_INDEX = 4, EMO_GIF_BAD_FRAME = 8 };
int emo_gif_lzw_decode(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, const int32_t* code_size,
                       const int64_t* out_offsets, uint8_t* indices, int32_t* produced, int32_t* status, int n, void* stream);
int emo_gif_compose(const uint8_t* indices, const int64_t* out_offsets, const int32_t* frames, const uint8_t* tables, uint8_t* rgb,
                    int32_t* status, int n, int n_tables, int n_out, int H, int W, void* stream);

/* ---- Motion-JPEG input: the device half of the reader that stands in for `VideoReader(path).read()`
 * (magicanimate/utils/videoreader.py; magicanimate/pipelines/animation.py:174-180 the control sequence, :182-185 the source image taken
 * from a video's first frame).  Baseline sequential JPEG, ITU-T T.81, 8-bit, one scan; the host half (marker segments of Annex B, the
 * removal of the stuffed 0x00 bytes, the decoding tables of Annex C / F.2.2.3, the AVI container) is emote_hack_amd/video_io.py.  The
 * kernels give the bytes libjpeg's default decoder gives (jidctint.c islow, jdsample.c fancy up-sampling, jdcolor.c); they live in
 * csrc/video_in.hip.
 * Every entry takes the scan's LAYOUT as three small ints: ncomp, the number of components, and hs x vs, the sampling factors of the
 * first (luminance) component; chrominance is always 1 x 1 (T.81 A.1.1).  An MCU of an interleaved scan holds hs * vs luminance blocks,
 * row by row, then one Cb and one Cr block (T.81 A.2.3); a one-component scan is not interleaved and its MCU is one block, whatever
 * factors the frame header states (T.81 A.2.2):
 *     ncomp hs vs   MCU       blocks per MCU (bpm)           chroma step, colour (libjpeg)
 *     3     2  2    16 x 16   6: Y00 Y01 Y10 Y11 Cb Cr      jdsample.c h2v2_fancy_upsample, jdcolor.c ycc_rgb_convert
 *     3     2  1    16 x 8    4: Y0 Y1 Cb Cr                jdsample.c h2v1_fancy_upsample, ycc_rgb_convert
 *     3     1  1    8 x 8     3: Y Cb Cr                    jdsample.c fullsize_upsample (chroma as it is), ycc_rgb_convert
 *     1     1  1    8 x 8     1                             jdcolor.c gray_rgb_convert: R = G = B = the sample
 *   Anything else (4:4:0, 4:1:1, four components) is EMO_ERR_BAD_SHAPE.  mcu_cols = ceil(W / (8 hs)), mcu_rows = ceil(H / (8 vs)),
 *   n_mcu their product; H, W in 1 .. 65535 as in emo_jpeg_blocks; n * n_mcu * bpm < 2^31.
 * emo_jpeg_decode_bits (T.81 F.2.2 Huffman decoding procedures: F.2.2.1 DC, F.2.2.2 AC, F.2.2.3 DECODE, F.2.2.4 RECEIVE, figure F.12
 *   EXTEND; A.2.3 the order of blocks in an MCU): the UNSTUFFED scans of n frames lie in `scan` (scan_bytes bytes, a multiple of 4,
 *   4-byte aligned; bytes behind the last frame are never used), frame i in bytes offsets[i] .. offsets[i + 1] (int64 [n + 1]).
 *   Output: coefs int16 [n][n_mcu][bpm][64] (MCUs in raster order, zig-zag order, the DC term UNDIFFERENCED: the differences are summed
 *   per component from 0 at every frame's first MCU; at 4:2:0 the layout emo_jpeg_blocks writes), 16-byte aligned, and status int32 [n]:
 *     EMO_JPEG_OK        the frame decoded: n_mcu * bpm blocks inside its bytes (what is left of them - the 1-bits that fill the last
 *                        byte, anything else - is not looked at)
 *     EMO_JPEG_BAD_CODE  the next 16 bits start with no code of the table, or with the code of a symbol a baseline scan of 8-bit samples
 *                        cannot hold: a DC category above 11, an AC category above 10, a run with category 0 other than EOB / ZRL
 *     EMO_JPEG_PAST_END  a code or its magnitude bits reach past the frame's last byte (a cut file, an empty frame; offsets that run
 *                        backwards or leave the buffer are taken as an empty frame)
 *     EMO_JPEG_BAD_RUN   a zero run carries the position past coefficient 63
 *   A frame with an error stops there: its blocks up to the faulty one are written, the rest of ITS coefficients are zeroed, other
 *   frames are not touched.  One workgroup per frame; every loop is counted by n_mcu * bpm blocks and 64 coefficients, every read of
 *   the stream is masked to the frame's own bytes.
 *   Block k % bpm of an MCU belongs to component 0 for k < bpm - 2 (all of them when bpm is 1), then to Cb, then to Cr; the component
 *   selects the DC prediction and the table pair.  tables: device int32 [4][EMO_JPEG_DECODE_TABLE_INTS] in the order DC luma, AC luma,
 *   DC chroma, AC chroma - [0], [1] for component 0, [2], [3] for Cb and Cr, which share theirs (a grey scan never reads those) - each
 *   table = MINCODE[16] | MAXCODE[16] | VALPTR[16] | 16 unused | HUFFVAL[256] of T.81 F.2.2.3 / figure F.15, entry l - 1 for code
 *   length l, MAXCODE -1 where no code has that length.  (The kernel expands them into an 8-bit look-up in LDS.)
 * emo_jpeg_decode_segments (T.81 B.2.4.4 DRI, E.1.4 restart intervals, F.1.1.5.1 / F.2.1.3.1 the DC predictions return to 0 at every
 *   restart; the decoding procedures of F.2.2 as above): the same decoding, one wavefront per SEGMENT.  A segment is a run of whole MCUs
 *   that starts on a byte with DC predictions 0: one restart interval (the bytes between two RSTm markers, the markers themselves and
 *   the stuffed 0x00 bytes taken out by the host), or a whole frame that has no restart markers.  Segment s lies in bytes
 *   seg_offsets[s] .. seg_offsets[s + 1] of `scan` (int64 [n_seg + 1], 8-byte aligned; scan as above) and fills seg_blocks[s] blocks (a
 *   multiple of bpm: whole MCUs) from block seg_first_block[s] on of coefs, blocks counted over the whole buffer of coef_blocks blocks
 *   of 64 int16 - for interval k of frame f with restart interval Ri: (f * n_mcu + k * Ri) * bpm and (min((k + 1) * Ri, n_mcu) - k * Ri)
 *   * bpm, so the buffer is the [n][n_mcu][bpm][64] emo_jpeg_decode_bits fills and emo_jpeg_idct reads.  Frames with different Ri, and
 *   frames without markers, may share a launch.  Blocks no segment names are not written.  status int32 [n_seg], PER SEGMENT, the values
 *   above with "segment" for "frame"; a segment with an error stops there, its blocks from the faulty one on are zeroed, other segments
 *   are not touched.  seg_first_block and seg_blocks are clamped to coef_blocks (a segment that reaches past the buffer decodes the
 *   blocks that fit and reports on those), seg_offsets to 0 .. scan_bytes and to run forwards: a bad table decodes wrong data or reports
 *   a status, it never reads or writes outside the buffers.  Every loop is counted by the segment's blocks and 64 coefficients; behind
 *   the set-up of the shared tables the waves of a workgroup meet no common barrier.
 * emo_jpeg_idct (T.81 A.3.4 dequantisation, A.3.3 IDCT in libjpeg's integer form jidctint.c jpeg_idct_islow): coefficient * quantiser,
 *   an 8-point pass over columns descaled by 11 bits, the same pass over rows descaled by 18, sample = clamp(value + 128, 0, 255).
 *   quant: device uint16 [3][64], one quantiser PER COMPONENT, NATURAL order (a grey frame reads the first only; its caller passes the
 *   one table three times).  Output, planes padded to whole MCUs: y_plane uint8 [n][mcu_rows * 8 vs][mcu_cols * 8 hs] and c_planes
 *   uint8 [n][2][mcu_rows * 8][mcu_cols * 8] (Cb, Cr; not touched and may be NULL when ncomp is 1), both 8-byte aligned.  32-bit sums
 *   that coefficients of no 8-bit image reach wrap.
 * emo_jpeg_rgb (jdsample.c, jdcolor.c): the planes above -> packed uint8 RGB [n][H][W][3], 4-byte aligned.
 *   4:2:0 (h2v2_fancy_upsample): the chroma plane of ceil(H / 2) x ceil(W / 2) real samples (the padded samples behind it are not
 *   read), s = 3 * c(r) + c(r -+ 1) down the rows for output rows 2 r / 2 r + 1, o(2 x) = (3 s(x) + s(x - 1) + 8) >> 4 and o(2 x + 1) =
 *   (3 s(x) + s(x + 1) + 7) >> 4 along them, neighbours clamped to the plane.  4:2:2 (h2v1_fancy_upsample): no filter down the columns;
 *   along a row of cw = ceil(W / 2) real chroma samples, p the sample at column x >> 1, o(x) = (3 p + p(left) + 1) >> 2 for even x and
 *   (3 p + p(right) + 2) >> 2 for odd x, the neighbour clamped to 0 .. cw - 1 - which is libjpeg's special case for the first and the
 *   last column; the padded samples behind cw are not read.  (libjpeg replicates samples instead when the chroma plane is at most 2
 *   wide, W <= 4: the host refuses such frames at 4:2:2 and 4:2:0.)  4:4:4 (fullsize_upsample): the chroma sample of the pixel itself.
 *   Colour (ycc_rgb_convert), cb and cr less 128: R = y + ((91881 cr + 32768) >> 16), G = y + ((-22554 cb - 46802 cr + 32768) >> 16),
 *   B = y + ((116130 cb + 32768) >> 16), each clamped to 0 .. 255.  Grey (gray_rgb_convert): the sample in all three channels, no
 *   transform; c_planes is not read and may be NULL.  Any W from 1 at 4:4:4 and grey. */
#define EMO_JPEG_DECODE_TABLE_INTS 320
enum { EMO_JPEG_OK = 0, EMO_JPEG_BAD_CODE = 1, EMO_JPEG_PAST_END = 2, EMO_JPEG_BAD_RUN = 3 };
int emo_jpeg_decode_bits(const uint8_t* scan, int64_t scan_bytes, const int64_t* offsets, const int32_t* tables, int16_t* coefs,
                         int32_t* status, int n, int n_mcu, int ncomp, int hs, int vs, void* stream);
int emo_jpeg_decode_segments(const uint8_t* scan, int64_t scan_bytes, const int64_t* seg_offsets, const int32_t* seg_first_block,
                             const int32_t* seg_blocks, const int32_t* tables, int16_t* coefs, int64_t coef_blocks, int32_t* status,
                             int n_seg, int ncomp, int hs, int vs, void* stream);
int emo_jpeg_idct(const int16_t* coefs, const uint16_t* quant, uint8_t* y_plane, uint8_t* c_planes, int n, int H, int W, int ncomp, int hs,
                  int vs, void* stream);
int emo_jpeg_rgb(const uint8_t* y_plane, const uint8_t* c_planes, uint8_t* rgb, int n, int H, int W, int ncomp, int hs, int vs, void* stream);

/* ---- Progressive JPEG input (T.81 Annex G, SOF2, Huffman coding): the entropy decoder behind decode_mjpeg(progressive=True);
 * csrc/video_in_progressive.hip.  A progressive file codes its coefficients in several scans - spectral selection (a scan holds the
 * band Ss .. Se of the zig-zag sequence) and successive approximation (a scan holds the bits down to Al, a later one refines by one
 * bit) - and the host (emote_hack_amd/video_io.py parse_jpeg(progressive=True)) walks them, keeps the tables and the restart interval
 * each scan saw, and takes only COMPLETE progressions, which libjpeg decodes without inter-block smoothing (jdcoefct.c smoothing_ok):
 * the coefficients are then those of the baseline file, and emo_jpeg_idct / emo_jpeg_rgb give libjpeg's bytes from them.
 * emo_jpeg_progressive_scan (T.81 G.1.1.1.1 the scans of a progression, G.1.2 / G.2 the Huffman procedures, A.2.2 / A.2.3 the order of
 *   the units, E.1.4 restart intervals; jdphuff.c decode_mcu_DC_first, decode_mcu_DC_refine, decode_mcu_AC_first, decode_mcu_AC_refine):
 *   ONE scan of a progression for many frames at once, into coefs int16 [n][n_mcu][bpm][64] (zig-zag order, the buffer
 *   emo_jpeg_decode_bits fills), which the caller zeroes before the first scan.  One wavefront per segment, a restart interval of the
 *   scan in one frame or the frame's whole scan: segment s holds bytes seg_offsets[s] .. seg_offsets[s + 1] of scan (int64 [n_seg + 1];
 *   unstuffed, markers taken out, scan_bytes a multiple of 4), belongs to frame seg_frame[s] and codes seg_units[s] units from unit
 *   seg_first_unit[s] on (int32 [n_seg] each).  ncomp, hs, vs: the layout; H, W: the frame.  Ss, Se, Ah, Al: the scan header's; Ss = 0
 *   needs Se = 0 (a DC scan), Ss > 0 a band inside 1 .. 63 of ONE component; Ah = 0 is a first scan, Ah > 0 a refinement with
 *   Al = Ah - 1; Al <= 13.  scan_comp: -1 for a scan interleaved over all components (DC scans only), else the one component 0 .. ncomp - 1.
 *   Units: in an interleaved scan a unit is an MCU, its bpm blocks in the buffer's order.  In a one-component scan a unit is one block
 *     of the component's OWN grid, bw = ceil(ceil(W h_c / hs) / 8) by bh = ceil(ceil(H v_c / vs) / 8) blocks in raster order - for
 *     luminance ceil(W / 8) x ceil(H / 8), not the grid padded to whole MCUs: block (by, bx) lives in MCU (by / vs) * mcu_cols + bx / hs
 *     as block (by % vs) * hs + bx % hs.  Padding blocks no one-component scan visits keep what they hold, as in libjpeg.
 *   Tables: device int32 [n_tables][EMO_JPEG_DECODE_TABLE_INTS] as above; seg_tables int32 [n_seg][3] names, by index, the DC table of
 *     each component of an interleaved scan, or in [s][0] the one DC or AC table of a one-component scan (a DC refinement reads none).
 *     An index is clamped to the array.  A wave loads the tables its segment names into LDS.
 *   The procedures: DC first - the difference of F.2.2.1 added to the component's prediction, which starts at 0 with every segment;
 *     the coefficient is the prediction << Al.  DC refine - one bit per block, OR-ed in at 1 << Al.  AC first - RRRRSSSS with SSSS = 0
 *     and R < 15 is EOBn: EOBRUN = (1 << R) + RECEIVE(R) ends this block's band and those of the next EOBRUN - 1 units; R = 15 is ZRL;
 *     else R zeros are skipped and the value << Al is stored.  AC refine - the new coefficient (SSSS = 1, one sign bit) of +-(1 << Al)
 *     goes behind R coefficients with a zero history; every coefficient with a nonzero history that is passed takes one correction bit,
 *     added towards its sign where bit Al is not yet set; an EOB run corrects the rest of the band's nonzero coefficients.
 *   Writes: positions Ss .. Se of the blocks of the segment's units, nothing else; a first scan (Ah = 0) stores zeros where it codes
 *     none, a refinement reads what is there.  The scans of a progression are launched in file order on one stream.
 *   status int32 [n_seg], the values above: EMO_JPEG_BAD_CODE also for a category above 11 (DC) or 10 (AC first) and SSSS other than 0
 *     or 1 in an AC refinement; EMO_JPEG_BAD_RUN also for a zero run that leaves the band and an EOBRUN longer than the units the
 *     segment has left; EMO_JPEG_PAST_END when the bits read reach past the segment's last byte.  A segment with an error stops: the
 *     block the error is in and those behind it are not written.  Segment offsets, frame, units are clamped to the buffers, every read
 *     of scan is masked to the segment's bytes, every loop is counted.  n * n_mcu * bpm < 2^31. */
int emo_jpeg_progressive_scan(const uint8_t* scan, int64_t scan_bytes, const int64_t* seg_offsets, const int32_t* seg_frame,
                              const int32_t* seg_first_unit, const int32_t* seg_units, const int32_t* seg_tables, const int32_t* tables,
                              int n_tables, int16_t* coefs, int32_t* status, int n_seg, int n, int H, int W, int ncomp, int hs, int vs, int Ss,
                              int Se, int Ah, int Al, int scan_comp, void* stream);

/* ---- Resizing 8-bit frames: `Image.fromarray(c).resize((size, size))` of every control frame and of the source image
 * (magicanimate/pipelines/animation.py:174-185) and `Image.open(source_image).resize((width, height))` (EMOAnimationPipeline.py:688),
 * byte for byte as Pillow's ImagingResample computes it for 8-bit pixels; csrc/image_resize.hip.
 * emo_image_resize: frames uint8 [n][H][W][3] -> out uint8 [n][h][w][3], 4-byte aligned, not overlapping the frames.  Integer
 *   arithmetic, two passes: the horizontal one writes 8-bit pixels [n][H][w][3] into the workspace, the vertical one reads those - the
 *   intermediate image is rounded to 8 bits as Pillow's is.  Per output index o of a pass, with (first, count) = bounds[o]:
 *     acc = 1 << 21;   acc += pixel[first + t] * coef[o][t]  for t < count;   result = clamp(acc >> 22, 0, 255)      (int32, arithmetic shift)
 *   xbounds / ybounds: device int32 [w][2] / [h][2] = (first input column / row, tap count); xcoef / ycoef: device int32 [w][kx] /
 *   [h][ky], 22-bit fixed point, zero behind the taps - the tables emote_hack_amd.video_io.resize_taps builds on the host in doubles, as
 *   Resample.c's precompute_coeffs and normalize_coeffs_8bpc do.  `first` is clamped to the axis and `count` to kx / ky and to what the
 *   axis has left behind `first`, so a bad table reads wrong pixels, never out of bounds.
 *   A pass whose axis keeps its size is skipped and its tables may be NULL; with both skipped the frames are copied.  The workspace is
 *   used only when both passes run: workspace_bytes must be >= emo_image_resize_workspace_bytes(n, H, W, h, w) (= n * H * w * 3 then, 0
 *   otherwise), 4-byte aligned and apart from the frames and out, else EMO_ERR_BAD_SHAPE / EMO_ERR_NULL before anything is launched;
 *   so are sizes below 1 and a frame (in, out or intermediate) of 2^31 bytes or more.  Every launch strides over its work: no size is
 *   capped by a grid limit. */
size_t emo_image_resize_workspace_bytes(int n, int H, int W, int h, int w);
int emo_image_resize(const uint8_t* frames, uint8_t* out, int n, int H, int W, int h, int w, const int32_t* xbounds, const int32_t* xcoef,
                     int kx, const int32_t* ybounds, const int32_t* ycoef, int ky, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CLIP vision encoder front (transformers CLIPVisionModelWithProjection: the `image_encoder` EMOAnimationPipeline.py:867 loads and
 * :909-917 hands to the pipeline; its image_embeds are the `clip_condition_embeddings` of models/videonet.py:255) -----------------------
 * emo_image_preprocess: transformers CLIPImageProcessor (resize to the shortest edge, centre crop, rescale, normalise) in one launch.
 *   img uint8 [n][H][W][3] RGB -> out f32 [n][3][S][S].  Replaces
 *     torch.nn.functional.interpolate(x.float(), size, mode="bicubic", antialias=True, align_corners=False), the crop,
 *     .clamp(0, 255) * rescale, (x - mean[c]) / std[c]
 *   in f32 with no intermediate rounding to uint8 (Keys kernel a = -0.5, support widened by the scale when shrinking, weights
 *   renormalised to sum 1, half-pixel centres).  The resize is separable; the host hands over one tap table per axis FOR THE CROP WINDOW
 *   (so only the window is computed, and the resize size / crop offsets live in the tables): ytap / xtap device int32 [S][2] = (first
 *   input row / column, tap count <= ky / kx), yw / xw device f32 [S][ky] / [S][kx].  span_max = the most input columns any tile of 64
 *   output columns touches (it sizes the LDS buffer; <= 5461).  mean / stddev: HOST float[3]; rescale: 1/255 for CLIP.  Table entries
 *   are clamped to the frame, so a bad table reads wrong pixels, never out of bounds.
 * emo_patch_rows: the im2col of CLIPVisionEmbeddings.patch_embedding (nn.Conv2d(3, hidden, kernel_size=P, stride=P, bias=False)):
 *   pix f32 [B][3][S][S] -> out [B * (S/P)^2][ld] in dtype, column (c * P + py) * P + px = pix[b][c][gy * P + py][gx * P + px], so the
 *   rows multiply patch_embedding.weight.reshape(hidden, 3 * P * P) (padded to ld with zeros); columns [3 P P, ld) are written as zero.
 * emo_vision_embed: CLIPVisionEmbeddings.forward + CLIPVisionTransformer.pre_layrnorm in one read and one write:
 *   row b * (Np + 1) = cls + pos[0], row b * (Np + 1) + 1 + p = patch[b * Np + p] + pos[1 + p]  (torch.cat([class_embeds, patch_embeds], 1)
 *   + position_embedding(position_ids)), then nn.LayerNorm(C, eps) over the row with gamma / beta f32.  patch [B * Np][ldp], cls [C],
 *   pos [Np + 1][C], y [B * (Np + 1)][ldy] in dtype; sums and statistics in f32 (mean, then centred squares - emo_layernorm's
 *   convention), rounded once. */
int emo_image_preprocess(const uint8_t* img, float* out, int n, int H, int W, int S, const int32_t* ytap, const float* yw, int ky,
                         const int32_t* xtap, const float* xw, int kx, int span_max, float rescale, const float* mean,
                         const float* stddev, void* stream);
int emo_patch_rows(const float* pix, void* out, int B, int S, int P, int ld, int dtype, void* stream);
int emo_vision_embed(const void* patch, int64_t ldp, const void* cls, const void* pos, const float* gamma, const float* beta, void* y,
                     int64_t ldy, int B, int Np, int C, float eps, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMO_HIP_H */
