// frontend.hip - the small kernels either side of the denoising loop:
//   emo_softmax_rows   : softmax(scale * x) over the columns of a materialised score matrix - the single-head, 512-wide
//                        attention of the VAE mid block (diffusers AutoencoderKL, called at EMOAnimationPipeline.py:291-307,
//                        402-414) runs as two MFMA GEMMs around it (head dim 512 is outside the flash kernel's register
//                        budget, and at one frame per call the 32 MB score matrix is cheap)
//   emo_audio_windows  : per audio frame, the wav2vec features of frames [f-m, f+n] zero-padded at the ends
//                        (Net.py:649-667 Wav2VecFeatureExtractor.extract_features_from_wav) - pure indexing, bit-exact
//   emo_rows_to_video  : decoded NHWC rows -> (B, C, F, H, W) f32 with video = (x / 2 + 0.5).clamp(0, 1)
//                        (EMOAnimationPipeline.py:303-306)
//   emo_channelnorm    : per-CHANNEL normalisation over the rows of a sequence (nn.GroupNorm(C, C) on (1, C, T): the first conv
//                        layer of the wav2vec2 feature extractor, transformers Wav2Vec2GroupNormConvLayer) + affine + optional
//                        erf-GELU; chunk partials in f32, re-reduced in f64 in a fixed order by every apply block (deterministic)
//   emo_audio_resample : channel downmix + rational polyphase resampling of an utterance to the processor's rate (the sf.read /
//                        librosa.resample / mean(axis=1) of Net.py:627-640), f32, one output sample per lane, 64-bit sample indices
//   emo_waveform_normalize : the processor's utterance normalisation (Net.py:639), two passes (mean, then centred squares), block
//                        partials combined in f64 in index order by every block (deterministic)
//   emo_interp_frames  : interpolate_latents (EMOAnimationPipeline.py:479-512) with util.py:125-138's slerp / linear for a whole clip:
//                        per-pair dot / norm partials, then every writing block re-reduces them in f64 and takes the threshold branch
//                        on the device (two launches, no host read, deterministic)
//   emo_rows_to_frames_u8 : decoded NHWC rows -> packed uint8 (B, F, H, W, C) frames, (x / 2 + 0.5).clamp(0, 1) * 255 truncated
//                        (decode_latents' tail + save_videos_grid, util.py:21-33)
// All HBM-bound and tiny; 16-byte accesses where the geometry allows.
#include "common.h"

static inline int fgrid(int64_t work, int block) {
  int64_t g = (work + block - 1) / block;
  if (g > 256 * 8) g = 256 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

// one wavefront per row; two passes over the row (online max / sum, then normalise).  N is a few thousand (h*w of a latent)
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy, int64_t M,
                                                           int N, float scale) {
  constexpr int V = TT<T>::VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float c = scale * 1.4426950408889634f;
  for (int64_t m = (int64_t)blockIdx.x * 4 + wave; m < M; m += (int64_t)gridDim.x * 4) {
    const T* xr = x + m * ldx;
    T* yr = y + m * ldy;
    float mx = -3.0e38f, sum = 0.f;
    const int NV = N / V;
    for (int i = lane; i < NV; i += 64) {
      float f[V];
      unpack16<T>(*(const uint4*)(xr + i * V), f);
      float lm = f[0];
#pragma unroll
      for (int e = 1; e < V; e++) lm = fmaxf(lm, f[e]);
      const float nm = fmaxf(mx, lm);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < V; e++) s += exp2f((f[e] - nm) * c);
      sum = sum * exp2f((mx - nm) * c) + s;
      mx = nm;
    }
    for (int i = NV * V + lane; i < N; i += 64) {   // ragged tail
      const float v = TT<T>::ld(xr + i), nm = fmaxf(mx, v);
      sum = sum * exp2f((mx - nm) * c) + exp2f((v - nm) * c);
      mx = nm;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sum, o, 64);
      const float nm = fmaxf(mx, om);
      sum = sum * exp2f((mx - nm) * c) + os * exp2f((om - nm) * c);
      mx = nm;
    }
    const float inv = 1.0f / sum;
    for (int i = lane; i < NV; i += 64) {
      float f[V];
      unpack16<T>(*(const uint4*)(xr + i * V), f);
#pragma unroll
      for (int e = 0; e < V; e++) f[e] = exp2f((f[e] - mx) * c) * inv;
      *(uint4*)(yr + i * V) = pack16<T>(f);
    }
    for (int i = NV * V + lane; i < N; i += 64) TT<T>::st(yr + i, exp2f((TT<T>::ld(xr + i) - mx) * c) * inv);
  }
}

extern "C" int emo_softmax_rows(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t M, int N, float scale, int dtype, void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_softmax_rows: null pointer");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_softmax_rows: dtype %d", dtype);
  const int V = emo_dtype_vec(dtype);
  EMO_CHECK(M > 0 && N > 0 && ldx >= N && ldy >= N && ldx % V == 0 && ldy % V == 0, EMO_ERR_BAD_SHAPE,
            "emo_softmax_rows: M=%lld N=%d ldx=%lld ldy=%lld", (long long)M, N, (long long)ldx, (long long)ldy);
  EMO_CHECK(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, EMO_ERR_BAD_SHAPE, "emo_softmax_rows: 16-byte alignment");
  EMO_DISPATCH(dtype, "emo_softmax_rows", (softmax_rows_kernel<T><<<fgrid(M, 4), 256, 0, as_stream(stream)>>>((const T*)x, ldx, (T*)y, ldy, M, N, scale)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// out[t][j][:] = feats[t - m + j][:] if 0 <= t - m + j < T else 0     (j = 0 .. m + n)
template <typename T>
__global__ __launch_bounds__(256) void audio_windows_kernel(const T* __restrict__ feats, T* __restrict__ out, int Tn, int D, int m, int n) {
  const int wlen = m + n + 1;
  const int64_t total = (int64_t)Tn * wlen * D;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    const int64_t r = i / D;
    const int j = (int)(r % wlen), t = (int)(r / wlen);
    const int src = t - m + j;
    out[i] = (src >= 0 && src < Tn) ? feats[(int64_t)src * D + d] : (T)0;
  }
}

extern "C" int emo_audio_windows(const void* feats, void* out, int T_, int D, int m, int n, int dtype, void* stream) {
  EMO_CHECK(feats && out, EMO_ERR_NULL, "emo_audio_windows: null pointer");
  EMO_CHECK(T_ > 0 && D > 0 && m >= 0 && n >= 0, EMO_ERR_BAD_SHAPE, "emo_audio_windows: T=%d D=%d m=%d n=%d", T_, D, m, n);
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_audio_windows: dtype %d", dtype);
  const int64_t total = (int64_t)T_ * (m + n + 1) * D;
  EMO_DISPATCH(dtype, "emo_audio_windows", (audio_windows_kernel<T><<<fgrid(total, 256), 256, 0, as_stream(stream)>>>((const T*)feats, (T*)out, T_, D, m, n)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// rows ((b f) h w, ld >= C) -> (B, C, F, H, W) f32, y = clamp(x * mul + add, lo, hi)
template <typename T>
__global__ __launch_bounds__(256) void rows_to_video_kernel(const T* __restrict__ x, int64_t ld, float* __restrict__ y, int B, int C, int F,
                                                            int HW, float mul, float add, float lo, float hi) {
  const int64_t total = (int64_t)B * C * F * HW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    int64_t r = i / HW;
    const int f = (int)(r % F); r /= F;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    const float v = TT<T>::ld(x + ((int64_t)(b * F + f) * HW + p) * ld + c) * mul + add;
    y[i] = fminf(fmaxf(v, lo), hi);
  }
}

extern "C" int emo_rows_to_video(const void* x, int64_t ld, float* y, int B, int C, int F, int HW, float mul, float add, float lo, float hi,
                                 int dtype, void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_rows_to_video: null pointer");
  EMO_CHECK(B > 0 && C > 0 && F > 0 && HW > 0 && ld >= C, EMO_ERR_BAD_SHAPE, "emo_rows_to_video: bad shape");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_rows_to_video: dtype %d", dtype);
  const int64_t total = (int64_t)B * C * F * HW;
  EMO_DISPATCH(dtype, "emo_rows_to_video", (rows_to_video_kernel<T><<<fgrid(total, 256), 256, 0, as_stream(stream)>>>((const T*)x, ld, y, B, C, F, HW, mul, add, lo, hi)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ---- FaceLocator pieces (Net.py:819-855): 2x2 max pooling over NHWC rows, bilinear upsampling of the logits map
template <typename T>
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy, int n_img, int H,
                                                         int W, int C) {
  const int Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)n_img * Ho * Wo * C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    int64_t r = i / C;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho);
    const int img = (int)(r / Ho);
    const T* p = x + (((int64_t)img * H + 2 * yo) * W + 2 * xo) * ldx + c;
    const float v = fmaxf(fmaxf(TT<T>::ld(p), TT<T>::ld(p + ldx)), fmaxf(TT<T>::ld(p + (int64_t)W * ldx), TT<T>::ld(p + (int64_t)(W + 1) * ldx)));
    TT<T>::st(y + (((int64_t)img * Ho + yo) * Wo + xo) * ldy + c, v);
  }
}

extern "C" int emo_maxpool2x2(const void* x, int64_t ldx, void* y, int64_t ldy, int n_img, int H, int W, int C, int dtype, void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_maxpool2x2: null pointer");
  EMO_CHECK(n_img > 0 && H >= 2 && W >= 2 && C > 0 && ldx >= C && ldy >= C, EMO_ERR_BAD_SHAPE, "emo_maxpool2x2: bad shape");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_maxpool2x2: dtype %d", dtype);
  const int64_t total = (int64_t)n_img * (H / 2) * (W / 2) * C;
  EMO_DISPATCH(dtype, "emo_maxpool2x2", (maxpool2x2_kernel<T><<<fgrid(total, 256), 256, 0, as_stream(stream)>>>((const T*)x, ldx, (T*)y, ldy, n_img, H, W, C)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// F.interpolate(mode='bilinear', align_corners=False) of rows ((n) h w, ld >= C) to (n, C, Ho, Wo) f32:
// src = (dst + 0.5) * in / out - 0.5 clamped at 0, neighbours i0 = floor(src), i1 = min(i0 + 1, in - 1)
template <typename T>
__global__ __launch_bounds__(256) void bilinear_kernel(const T* __restrict__ x, int64_t ld, float* __restrict__ y, int n_img, int C, int h, int w,
                                                       int Ho, int Wo) {
  const int64_t total = (int64_t)n_img * C * Ho * Wo;
  const float sy = (float)h / (float)Ho, sx = (float)w / (float)Wo;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wo);
    int64_t r = i / Wo;
    const int yo = (int)(r % Ho); r /= Ho;
    const int c = (int)(r % C);
    const int img = (int)(r / C);
    const float fy = fmaxf(((float)yo + 0.5f) * sy - 0.5f, 0.f), fx = fmaxf(((float)xo + 0.5f) * sx - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + 1 < h ? y0 + 1 : h - 1, x1 = x0 + 1 < w ? x0 + 1 : w - 1;
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const T* b = x + (int64_t)img * h * w * ld + c;
    const float v00 = TT<T>::ld(b + ((int64_t)y0 * w + x0) * ld), v01 = TT<T>::ld(b + ((int64_t)y0 * w + x1) * ld);
    const float v10 = TT<T>::ld(b + ((int64_t)y1 * w + x0) * ld), v11 = TT<T>::ld(b + ((int64_t)y1 * w + x1) * ld);
    y[i] = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  }
}

extern "C" int emo_bilinear_to_nchw(const void* x, int64_t ld, float* y, int n_img, int C, int h, int w, int Ho, int Wo, int dtype, void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_bilinear_to_nchw: null pointer");
  EMO_CHECK(n_img > 0 && C > 0 && h > 0 && w > 0 && Ho > 0 && Wo > 0 && ld >= C, EMO_ERR_BAD_SHAPE, "emo_bilinear_to_nchw: bad shape");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_bilinear_to_nchw: dtype %d", dtype);
  const int64_t total = (int64_t)n_img * C * Ho * Wo;
  EMO_DISPATCH(dtype, "emo_bilinear_to_nchw", (bilinear_kernel<T><<<fgrid(total, 256), 256, 0, as_stream(stream)>>>((const T*)x, ld, y, n_img, C, h, w, Ho, Wo)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}


// ---------------------------------------------------------------------------------------------------------------- channel norm
// x rows (S, C): y[s, c] = act((x[s, c] - mean_c) * rstd_c * gamma_c + beta_c), statistics over the S rows of each channel
// (biased variance, like nn.GroupNorm).  Pass 1: block (chunk, column slab of 64 channels) -> partial (sum, sumsq) per channel.
// Pass 2: every block re-reduces the chunk partials of its slab in f64 in chunk order, then normalises its rows.
// Both passes work on x - x[0, c] (the channel's first row; every chunk shifts alike, so the partials still add up): sum(x^2) / S - mean^2
// on the raw values loses the variance of a channel whose spread is small against its level (two rows 0.01 apart at level 3 in f32: off by
// 16 x the f32 tolerance), the shifted sums do not.
static constexpr int CN_COLS = 64, CN_ROWS_T = 4;   // 256 threads = 64 channels x 4 row lanes

template <typename T>
__global__ __launch_bounds__(256) void channelnorm_stats_kernel(const T* __restrict__ x, int64_t ldx, float* __restrict__ part, int64_t S, int C, int nchunk) {
  const int c = blockIdx.y * CN_COLS + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int64_t per = (S + nchunk - 1) / nchunk, s0 = blockIdx.x * per, s1 = s0 + per < S ? s0 + per : S;
  float sum = 0.f, sq = 0.f;
  if (c < C) {
    const float x0 = TT<T>::ld(x + c);
    for (int64_t s_ = s0 + rl; s_ < s1; s_ += CN_ROWS_T) {
      const float v = TT<T>::ld(x + s_ * ldx + c) - x0;
      sum += v; sq = fmaf(v, v, sq);
    }
  }
  __shared__ float sh[2][CN_ROWS_T][CN_COLS];
  sh[0][rl][threadIdx.x & 63] = sum; sh[1][rl][threadIdx.x & 63] = sq;
  __syncthreads();
  if (rl == 0 && c < C) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int r = 0; r < CN_ROWS_T; r++) { a += sh[0][r][threadIdx.x]; b += sh[1][r][threadIdx.x]; }
    part[((int64_t)blockIdx.x * C + c) * 2] = a;
    part[((int64_t)blockIdx.x * C + c) * 2 + 1] = b;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void channelnorm_apply_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ part,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ y,
                                                                int64_t ldy, int64_t S, int C, int nchunk, float eps, int act) {
  const int cl = threadIdx.x & 63, c = blockIdx.y * CN_COLS + cl, rl = threadIdx.x >> 6;
  __shared__ float sc[CN_COLS], sf[CN_COLS];
  if (rl == 0 && c < C) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < nchunk; k++) { a += (double)part[((int64_t)k * C + c) * 2]; b += (double)part[((int64_t)k * C + c) * 2 + 1]; }
    const double mean = a / (double)S;          // of x - x[0, c]
    double var = b / (double)S - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    sc[cl] = rstd * gamma[c];
    sf[cl] = (float)mean;
  }
  __syncthreads();
  if (c >= C) return;
  const float k = sc[cl], ms = sf[cl], o = beta[c], x0 = TT<T>::ld(x + c);
  for (int64_t s_ = (int64_t)blockIdx.x * CN_ROWS_T + rl; s_ < S; s_ += (int64_t)gridDim.x * CN_ROWS_T) {
    float v = fmaf((TT<T>::ld(x + s_ * ldx + c) - x0) - ms, k, o);
    if (act == 1) v = gelu_for<T>(v);
    TT<T>::st(y + s_ * ldy + c, v);
  }
}

extern "C" size_t emo_channelnorm_workspace_bytes(int64_t S, int C) {
  int64_t n = (S + 255) / 256;
  if (n > 64) n = 64;
  if (n < 1) n = 1;
  return (size_t)n * C * 2 * sizeof(float);
}
extern "C" int emo_channelnorm(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy, int64_t S, int C, float eps,
                               int act, void* workspace, int dtype, void* stream) {
  EMO_CHECK(x && gamma && beta && y && workspace, EMO_ERR_NULL, "emo_channelnorm: null pointer");
  EMO_CHECK(S > 0 && C > 0 && ldx >= C && ldy >= C && (act == 0 || act == 1), EMO_ERR_BAD_SHAPE, "emo_channelnorm: S=%lld C=%d act=%d", (long long)S, C, act);
  int64_t n = (S + 255) / 256;
  if (n > 64) n = 64;
  if (n < 1) n = 1;
  const dim3 g1((unsigned)n, (unsigned)((C + CN_COLS - 1) / CN_COLS));
  int64_t nb = (S + CN_ROWS_T * 16 - 1) / (CN_ROWS_T * 16);
  if (nb > 512) nb = 512;
  if (nb < 1) nb = 1;
  const dim3 g2((unsigned)nb, g1.y);
  hipStream_t st = as_stream(stream);
  EMO_DISPATCH(dtype, "emo_channelnorm", (channelnorm_stats_kernel<T><<<g1, 256, 0, st>>>((const T*)x, ldx, (float*)workspace, S, C, (int)n)));
  EMO_LAUNCH_CHECK();
  EMO_DISPATCH(dtype, "emo_channelnorm", (channelnorm_apply_kernel<T><<<g2, 256, 0, st>>>((const T*)x, ldx, (const float*)workspace, gamma, beta, (T*)y, ldy, S, C,
                                                                                               (int)n, eps, act)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}


// ------------------------------------------------------------------------------------------------- wav conv 0 + LayerNorm + act
// Feature-encoder layer 0 of the layer-norm wav2vec2 family (transformers Wav2Vec2LayerNormConvLayer with Cin = 1) straight from the
// f32 waveform:  y[t, c] = act(LN_c(bias[c] + sum_{j<k} w[c][j] * wave[t * stride + j])).  Neither the (T0, k) window matrix nor the
// pre-norm (T0, C) tensor exists in memory: the kernel reads 4 * stride bytes and writes one output row per time step.
//   lane mapping   a row is held by LPR adjacent lanes, 8 channels (NV = 1) or 2 x 8 channels (NV = 2, C > 512) per lane; a wavefront
//                  holds 64 / LPR rows at a time and owns `run` consecutive such row groups
//   weights        NV = 1: the lane's 8 x k taps, its bias and its affine sit in registers for the whole run (C = 512, k = 10: 80 + 24);
//                  NV = 2 (no checkpoint has it; served for completeness): the taps are re-read per row (L1 / L2 hits)
//   samples        the k samples of a row are one address per row group (LPR = 64: wave-uniform)
//   arithmetic     taps in ascending j with fmaf from the bias, f32; two-pass statistics with layernorm_kernel's shuffle pattern
//                  and output expression; one rounding to T
// KP is the compile-time tap count the register array is sized and unrolled for (k <= KP; steps j >= k are skipped by a uniform test).
static constexpr int WC0_MAXC = 1024, WC0_MAXK = 16, WC0_WAVES = 2048;

struct Wc0Geom { int ok, lpr, nv, kp, run, grid; int64_t T0; };
static inline Wc0Geom wc0_geom(int64_t n, int C, int k, int stride) {
  Wc0Geom g{0, 0, 0, 0, 0, 0, 0};
  if (C <= 0 || C % 8 || C > WC0_MAXC || k < 1 || k > WC0_MAXK || stride < 1 || n < k) return g;
  g.T0 = (n - k) / stride + 1;
  const int CV = C / 8;
  g.nv = CV > 64 ? 2 : 1;
  g.lpr = CV <= 8 ? 8 : 64;
  g.kp = g.nv == 2 ? 16 : k <= 4 ? 4 : k <= 10 ? 10 : 16;
  const int rpw = 64 / g.lpr;
  const int64_t groups = (g.T0 + rpw - 1) / rpw;
  // a run amortises the lane's weight load (k * C * 4 bytes per wavefront against C * sizeof(T) per row): >= 8 row groups, more once
  // WC0_WAVES wavefronts (8 per CU) are in flight
  int64_t run = (groups + WC0_WAVES - 1) / WC0_WAVES;
  if (run < 8) run = 8;
  const int64_t waves = (groups + run - 1) / run;
  g.run = (int)run;
  g.grid = (int)((waves + 3) / 4);
  g.ok = 1;
  return g;
}

template <typename T> __device__ __forceinline__ void wc0_store8(T* p, const float* f) { *(uint4*)p = pack16<T>(f); }
template <> __device__ __forceinline__ void wc0_store8<float>(float* p, const float* f) {
  *(float4*)p = make_float4(f[0], f[1], f[2], f[3]);
  *(float4*)(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

template <typename T, int KP, int LPR, int NV>
__global__ __launch_bounds__(256) void wav_conv0_ln_act_kernel(const float* __restrict__ wave, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, T* __restrict__ y, int64_t ldy, int64_t T0,
                                                               int C, int k, int stride, float eps, int act, int run) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane % LPR, rsel = lane / LPR;
  const int CV = C / 8;
  const float invC = 1.0f / (float)C;
  bool on[NV];
  int c0[NV];
  float bs[NV][8], gm[NV][8], bt[NV][8];
  float wr[NV == 1 ? KP : 1][8];
#pragma unroll
  for (int v = 0; v < NV; v++) {
    const int cv = sub + LPR * v;
    on[v] = cv < CV;
    c0[v] = on[v] ? cv * 8 : 0;       // (an idle lane reads channel 0's constants and stores nothing)
#pragma unroll
    for (int e = 0; e < 8; e += 4) {
      *(float4*)&bs[v][e] = *(const float4*)(bias + c0[v] + e);
      *(float4*)&gm[v][e] = *(const float4*)(gamma + c0[v] + e);
      *(float4*)&bt[v][e] = *(const float4*)(beta + c0[v] + e);
    }
  }
  if constexpr (NV == 1) {
#pragma unroll
    for (int j = 0; j < KP; j++)
#pragma unroll
      for (int e = 0; e < 8; e++) wr[j][e] = j < k ? w[(int64_t)(c0[0] + e) * k + j] : 0.f;
  }
  const int64_t g0 = ((int64_t)blockIdx.x * 4 + wv) * run;
  for (int r = 0; r < run; r++) {
    const int64_t tg = (g0 + r) * RPW;
    if (tg >= T0) break;              // wave-uniform: the shuffles below stay whole
    const int64_t t = tg + rsel;
    const bool ok = t < T0;
    const float* xs = wave + (ok ? t : T0 - 1) * stride;   // a row past the end re-reads the last one and stores nothing
    float acc[NV][8];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
      for (int e = 0; e < 8; e++) acc[v][e] = bs[v][e];
    if constexpr (NV == 1) {
#pragma unroll
      for (int j = 0; j < KP; j++) {
        if (j < k) {
          const float xj = xs[j];
#pragma unroll
          for (int e = 0; e < 8; e++) acc[0][e] = fmaf(wr[j][e], xj, acc[0][e]);
        }
      }
    } else {
      for (int j = 0; j < k; j++) {
        const float xj = xs[j];
#pragma unroll
        for (int v = 0; v < NV; v++)
#pragma unroll
          for (int e = 0; e < 8; e++) acc[v][e] = fmaf(w[(int64_t)(c0[v] + e) * k + j], xj, acc[v][e]);
      }
    }
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++)
      if (on[v]) {
#pragma unroll
        for (int e = 0; e < 8; e++) s += acc[v][e];
      }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s * invC;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < NV; v++)
      if (on[v]) {
#pragma unroll
        for (int e = 0; e < 8; e++) { const float d = acc[v][e] - mean; q += d * d; }
      }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = rsqrtf(q * invC + eps);
#pragma unroll
    for (int v = 0; v < NV; v++) {
      if (ok && on[v]) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const float u = (acc[v][e] - mean) * rstd * gm[v][e] + bt[v][e];
          o[e] = act == 1 ? gelu_for<T>(u) : u;
        }
        wc0_store8<T>(y + t * ldy + c0[v], o);
      }
    }
  }
}

static int wc0_check(const char* who, int64_t n, int C, int k, int stride) {
  EMO_CHECK(wc0_geom(n, C, k, stride).ok, EMO_ERR_UNSUPPORTED,
            "%s: n=%lld C=%d k=%d stride=%d (served: C %% 8 == 0, C <= %d, 1 <= k <= %d, stride >= 1, n >= k)", who, (long long)n, C, k, stride,
            WC0_MAXC, WC0_MAXK);
  return EMO_OK;
}

extern "C" int emo_wav_conv0_ln_act_plan(int64_t n, int C, int k, int stride, int64_t plan[6]) {
  EMO_CHECK(plan, EMO_ERR_NULL, "emo_wav_conv0_ln_act_plan: null pointer");
  int rc = wc0_check("emo_wav_conv0_ln_act_plan", n, C, k, stride);
  if (rc) return rc;
  const Wc0Geom g = wc0_geom(n, C, k, stride);
  plan[0] = g.T0; plan[1] = g.lpr; plan[2] = g.nv; plan[3] = g.kp; plan[4] = g.run; plan[5] = g.grid;
  return EMO_OK;
}

extern "C" int emo_wav_conv0_ln_act(const float* wave, int64_t n, const float* w, const float* bias, const float* gamma, const float* beta,
                                    void* y, int64_t ldy, int C, int k, int stride, float eps, int act, int dtype, void* stream) {
  EMO_CHECK(wave && w && bias && gamma && beta && y, EMO_ERR_NULL, "emo_wav_conv0_ln_act: null pointer");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_wav_conv0_ln_act: dtype %d", dtype);
  int rc = wc0_check("emo_wav_conv0_ln_act", n, C, k, stride);
  if (rc) return rc;
  EMO_CHECK(ldy >= C && ldy % emo_dtype_vec(dtype) == 0 && (act == 0 || act == 1), EMO_ERR_BAD_SHAPE, "emo_wav_conv0_ln_act: ldy=%lld C=%d act=%d",
            (long long)ldy, C, act);
  EMO_CHECK(((uintptr_t)bias % 16) == 0 && ((uintptr_t)gamma % 16) == 0 && ((uintptr_t)beta % 16) == 0 && ((uintptr_t)y % 16) == 0 &&
            ((uintptr_t)wave % 4) == 0 && ((uintptr_t)w % 4) == 0, EMO_ERR_BAD_SHAPE, "emo_wav_conv0_ln_act: operand alignment");
  const Wc0Geom g = wc0_geom(n, C, k, stride);
  hipStream_t st = as_stream(stream);
#define EMO_WC0(KP_, LPR_, NV_)                                                                                                          \
  EMO_DISPATCH(dtype, "emo_wav_conv0_ln_act", (wav_conv0_ln_act_kernel<T, KP_, LPR_, NV_><<<g.grid, 256, 0, st>>>(                        \
                                                  wave, w, bias, gamma, beta, (T*)y, ldy, g.T0, C, k, stride, eps, act, g.run)))
  if (g.nv == 2) { EMO_WC0(16, 64, 2); }
  else if (g.lpr == 8) {
    if (g.kp == 4) { EMO_WC0(4, 8, 1); } else if (g.kp == 10) { EMO_WC0(10, 8, 1); } else { EMO_WC0(16, 8, 1); }
  } else {
    if (g.kp == 4) { EMO_WC0(4, 64, 1); } else if (g.kp == 10) { EMO_WC0(10, 64, 1); } else { EMO_WC0(16, 64, 1); }
  }
#undef EMO_WC0
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}


// -------------------------------------------------------------------------------------------------------------- audio resampling
// y[n] = sum_j h[n*down - j*up] * x[j] over |n*down - j*up| <= half, x[j] = mean over channels of frame j (0 outside the utterance).
// With t = n*down = T0*up + p the taps of output n are h[p + up*i] at j = T0 - i: row p of the phase table, column c = i + i0
// (i0 = ceil(half / up) rounded so that every i fits; entries past +-half are 0).  Ascending j = descending c.
__global__ __launch_bounds__(256) void audio_resample_kernel(const float* __restrict__ in, int64_t in_start, int64_t n_in, int channels,
                                                             const float* __restrict__ tab, int tpp, int i0, int64_t up, int64_t down,
                                                             float* __restrict__ out, int64_t out_start, int64_t n_out) {
  for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < n_out; o += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = (out_start + o) * down, T0 = t / up, p = t - T0 * up;
    const float* w = tab + p * tpp;
    float acc = 0.f;
    for (int c = tpp - 1; c >= 0; c--) {
      const int64_t j = T0 - (c - i0) - in_start;          // index into the slice; global frame T0 - (c - i0)
      float x = 0.f;
      if (j >= 0 && j < n_in) {
        const float* f = in + j * channels;
        float s = f[0];
        for (int ch = 1; ch < channels; ch++) s += f[ch];
        x = s / (float)channels;
      }
      acc = fmaf(w[c], x, acc);
    }
    out[o] = acc;
  }
}

extern "C" int emo_audio_resample_taps_per_phase(int up, int half) {
  if (up < 1 || half < 0) return 0;
  return (int)(((int64_t)half + up - 1) / up + (int64_t)half / up + 1);
}
extern "C" int emo_audio_resample(const float* in, int64_t in_start, int64_t n_in, int channels, const float* taps, int64_t n_taps, int up,
                                  int down, int half, float* out, int64_t out_start, int64_t n_out, void* stream) {
  EMO_CHECK(in && taps && out, EMO_ERR_NULL, "emo_audio_resample: null pointer");
  EMO_CHECK(up >= 1 && down >= 1 && up <= 65536 && down <= 65536 && half >= 0 && half <= 10 * 65536, EMO_ERR_BAD_SHAPE,
            "emo_audio_resample: up=%d down=%d half=%d", up, down, half);
  const int tpp = emo_audio_resample_taps_per_phase(up, half);
  EMO_CHECK(n_taps == (int64_t)up * tpp, EMO_ERR_BAD_SHAPE, "emo_audio_resample: the phase table has %lld entries, up * taps_per_phase = %lld",
            (long long)n_taps, (long long)up * tpp);
  EMO_CHECK(n_in > 0 && channels >= 1 && channels <= 64 && n_out > 0 && in_start >= 0 && out_start >= 0, EMO_ERR_BAD_SHAPE,
            "emo_audio_resample: n_in=%lld channels=%d n_out=%lld in_start=%lld out_start=%lld", (long long)n_in, channels, (long long)n_out,
            (long long)in_start, (long long)out_start);
  const int64_t lim = (int64_t)1 << 44;      // (out_start + n_out) * down and in_start + n_in stay far inside int64
  EMO_CHECK(n_in < lim && in_start < lim && n_out < lim && out_start < lim, EMO_ERR_BAD_SHAPE, "emo_audio_resample: index range");
  audio_resample_kernel<<<fgrid(n_out, 256), 256, 0, as_stream(stream)>>>(in, in_start, n_in, channels, taps, tpp, (half + up - 1) / up, up, down,
                                                                         out, out_start, n_out);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ---------------------------------------------------------------------------------------------------------- waveform normalisation
// y = (x - mean) / sqrt(var + eps), population variance.  Block b owns the contiguous chunk [b*per, (b+1)*per).  Pass 1: chunk sums ->
// part[b].  Pass 2: every block combines part[0..nb) in index order (f64) into the mean, then sums the squared deviations of its
// chunk -> part[nb + b].  Pass 3: every block combines both lists the same way and normalises.  No atomics: the same bits every run.
static constexpr int WN_T = 256, WN_MAXB = 512;

static inline int wn_blocks(int64_t n) {
  int64_t b = (n + WN_T - 1) / WN_T;
  return (int)(b > WN_MAXB ? WN_MAXB : (b < 1 ? 1 : b));
}

__device__ __forceinline__ float wn_block_sum(float v, float* sh) {      // fixed-order tree over the 256 lanes
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = WN_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

__device__ __forceinline__ double wn_combine(const float* part, int nb, double* bc) {   // every thread gets sum(part[0..nb)) in index order
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int k = 0; k < nb; k++) a += (double)part[k];
    *bc = a;
  }
  __syncthreads();
  return *bc;
}

__global__ __launch_bounds__(WN_T) void wavenorm_sum_kernel(const float* __restrict__ x, float* __restrict__ part, int64_t n, int64_t per) {
  __shared__ float sh[WN_T];
  const int64_t s0 = blockIdx.x * per, s1 = s0 + per < n ? s0 + per : n;
  float a = 0.f;
  for (int64_t i = s0 + threadIdx.x; i < s1; i += WN_T) a += x[i];
  a = wn_block_sum(a, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = a;
}

__global__ __launch_bounds__(WN_T) void wavenorm_dev_kernel(const float* __restrict__ x, float* __restrict__ part, int64_t n, int64_t per, int nb) {
  __shared__ float sh[WN_T];
  __shared__ double bc;
  const float mean = (float)(wn_combine(part, nb, &bc) / (double)n);
  const int64_t s0 = blockIdx.x * per, s1 = s0 + per < n ? s0 + per : n;
  float a = 0.f;
  for (int64_t i = s0 + threadIdx.x; i < s1; i += WN_T) {
    const float d = x[i] - mean;
    a = fmaf(d, d, a);
  }
  a = wn_block_sum(a, sh);
  if (threadIdx.x == 0) part[nb + blockIdx.x] = a;
}

__global__ __launch_bounds__(WN_T) void wavenorm_apply_kernel(const float* __restrict__ x, const float* __restrict__ part, float* __restrict__ y,
                                                              int64_t n, int nb, float eps) {
  __shared__ double bc[2];
  const float mean = (float)(wn_combine(part, nb, &bc[0]) / (double)n);
  const float rstd = (float)(1.0 / sqrt(wn_combine(part + nb, nb, &bc[1]) / (double)n + (double)eps));
  for (int64_t i = blockIdx.x * (int64_t)WN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * WN_T) y[i] = (x[i] - mean) * rstd;
}

extern "C" size_t emo_waveform_normalize_workspace_bytes(int64_t n) { return (size_t)wn_blocks(n) * 2 * sizeof(float); }
extern "C" int emo_waveform_normalize(const float* x, float* y, int64_t n, float eps, void* workspace, size_t workspace_bytes, void* stream) {
  EMO_CHECK(x && y && workspace, EMO_ERR_NULL, "emo_waveform_normalize: null pointer");
  EMO_CHECK(n > 0 && eps >= 0.f, EMO_ERR_BAD_SHAPE, "emo_waveform_normalize: n=%lld eps=%g", (long long)n, (double)eps);
  EMO_CHECK(workspace_bytes >= emo_waveform_normalize_workspace_bytes(n), EMO_ERR_BAD_SHAPE,
            "emo_waveform_normalize: workspace of %llu bytes, emo_waveform_normalize_workspace_bytes(%lld) = %llu",
            (unsigned long long)workspace_bytes, (long long)n, (unsigned long long)emo_waveform_normalize_workspace_bytes(n));
  const int nb = wn_blocks(n);
  const int64_t per = (n + nb - 1) / nb;
  hipStream_t st = as_stream(stream);
  wavenorm_sum_kernel<<<nb, WN_T, 0, st>>>(x, (float*)workspace, n, per);
  EMO_LAUNCH_CHECK();
  wavenorm_dev_kernel<<<nb, WN_T, 0, st>>>(x, (float*)workspace, n, per, nb);
  EMO_LAUNCH_CHECK();
  wavenorm_apply_kernel<<<nb, WN_T, 0, st>>>(x, (const float*)workspace, y, n, nb, eps);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------ frame interpolation
// interpolate_latents (EMOAnimationPipeline.py:479-512) over x (B, C, F, HW) f32: output frame j = p * k + r is frame p (r == 0, a copy)
// or w0 * frame p + w1 * frame p+1 with the weights of util.py:125-138 at t = r / k.  A frame is ONE vector of N = B*C*HW values: plane
// pl = (b, c) contributes HW contiguous floats at (pl * F + f) * HW, so logical element n lives at plane n / HW, offset n % HW (64-bit).
// Pass 1: block (pair, slice [s*per, (s+1)*per) of the N elements) -> f32 partials (<v0, v1>, |v0|^2, |v1|^2) at part[(pair * ns + s) * 3].
// Pass 2: block (output frame, slice); for r != 0 thread 0 re-reduces the pair's ns partials in index order in f64, takes the threshold
// branch and derives the two weights.  No atomics, no counters: the same bits every run, nothing read back by the host.
static constexpr int IF_T = 256, IF_SLICE = 2048, IF_MAXS = 256;

static inline int if_slices(int64_t N) {
  int64_t s = (N + IF_SLICE - 1) / IF_SLICE;
  return (int)(s > IF_MAXS ? IF_MAXS : (s < 1 ? 1 : s));
}
static inline int64_t if_per(int64_t N, int ns) {    // a multiple of 4: a 16-byte chunk never straddles two slices
  const int64_t per = (N + ns - 1) / ns;
  return (per + 3) / 4 * 4;
}

template <bool VEC>
__global__ __launch_bounds__(IF_T) void interp_reduce_kernel(const float* __restrict__ x, float* __restrict__ part, int F, int64_t HW, int64_t N,
                                                             int64_t per) {
  const int pair = blockIdx.x, s = blockIdx.y, ns = gridDim.y;
  const int64_t n0 = s * per, n1 = n0 + per < N ? n0 + per : N;
  float d = 0.f, a = 0.f, b = 0.f;
  if constexpr (VEC) {      // HW % 4 == 0 (so N % 4 == 0) and x 16-byte aligned: every chunk lies inside one plane
    for (int64_t n = n0 + 4 * (int64_t)threadIdx.x; n < n1; n += 4 * IF_T) {
      const int64_t pl = n / HW, i = n - pl * HW;
      const float* q = x + (pl * F + pair) * HW + i;
      const float4 u = *(const float4*)q, v = *(const float4*)(q + HW);
      d = fmaf(u.x, v.x, d); d = fmaf(u.y, v.y, d); d = fmaf(u.z, v.z, d); d = fmaf(u.w, v.w, d);
      a = fmaf(u.x, u.x, a); a = fmaf(u.y, u.y, a); a = fmaf(u.z, u.z, a); a = fmaf(u.w, u.w, a);
      b = fmaf(v.x, v.x, b); b = fmaf(v.y, v.y, b); b = fmaf(v.z, v.z, b); b = fmaf(v.w, v.w, b);
    }
  } else {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += IF_T) {
      const int64_t pl = n / HW, i = n - pl * HW;
      const float* q = x + (pl * F + pair) * HW + i;
      const float u = q[0], v = q[HW];
      d = fmaf(u, v, d); a = fmaf(u, u, a); b = fmaf(v, v, b);
    }
  }
  d = wave_sum(d); a = wave_sum(a); b = wave_sum(b);
  __shared__ float sh[3][IF_T / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[0][wave] = d; sh[1][wave] = a; sh[2][wave] = b; }
  __syncthreads();
  if (threadIdx.x < 3) {
    float t = sh[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < IF_T / 64; w++) t += sh[threadIdx.x][w];
    part[((int64_t)pair * ns + s) * 3 + threadIdx.x] = t;
  }
}

template <bool VEC>
__global__ __launch_bounds__(IF_T) void interp_write_kernel(const float* __restrict__ x, const float* __restrict__ part, float* __restrict__ y, int F,
                                                            int Fo, int64_t HW, int64_t N, int64_t per, int ns, int k, int method, float thr) {
  const int j = blockIdx.x, s = blockIdx.y;
  const int pr = j / k, r = j - pr * k;
  __shared__ float wsh[2];
  if (r != 0) {             // block-uniform
    if (threadIdx.x == 0) {
      const double t = (double)r / (double)k;
      double w0 = 1.0 - t, w1 = t;
      if (method == 1) {
        const float* pp = part + (int64_t)pr * ns * 3;
        double dd = 0.0, aa = 0.0, bb = 0.0;
        for (int i = 0; i < ns; i++) { dd += (double)pp[3 * i]; aa += (double)pp[3 * i + 1]; bb += (double)pp[3 * i + 2]; }
        const double c = dd / (sqrt(aa) * sqrt(bb));     // 0 / 0 = NaN for a zero frame: compares false, acos(NaN) = NaN, as upstream
        if (!(fabs(c) > (double)thr)) {
          const double om = acos(c), so = sin(om);
          w0 = sin((1.0 - t) * om) / so;
          w1 = sin(t * om) / so;
        }
      }
      wsh[0] = (float)w0; wsh[1] = (float)w1;
    }
    __syncthreads();
  }
  const int64_t n0 = s * per, n1 = n0 + per < N ? n0 + per : N;
  if (r == 0) {             // bit-for-bit copy of input frame pr (the last output frame is the last input frame: pr + 1 is never read)
    if constexpr (VEC) {
      for (int64_t n = n0 + 4 * (int64_t)threadIdx.x; n < n1; n += 4 * IF_T) {
        const int64_t pl = n / HW, i = n - pl * HW;
        *(uint4*)(y + (pl * Fo + j) * HW + i) = *(const uint4*)(x + (pl * F + pr) * HW + i);
      }
    } else {
      const uint32_t* xs = (const uint32_t*)x;
      uint32_t* yd = (uint32_t*)y;
      for (int64_t n = n0 + threadIdx.x; n < n1; n += IF_T) {
        const int64_t pl = n / HW, i = n - pl * HW;
        yd[(pl * Fo + j) * HW + i] = xs[(pl * F + pr) * HW + i];
      }
    }
    return;
  }
  const float w0 = wsh[0], w1 = wsh[1];
  if constexpr (VEC) {
    for (int64_t n = n0 + 4 * (int64_t)threadIdx.x; n < n1; n += 4 * IF_T) {
      const int64_t pl = n / HW, i = n - pl * HW;
      const float* q = x + (pl * F + pr) * HW + i;
      const float4 u = *(const float4*)q, v = *(const float4*)(q + HW);
      float4 o;
      o.x = fmaf(w0, u.x, w1 * v.x); o.y = fmaf(w0, u.y, w1 * v.y); o.z = fmaf(w0, u.z, w1 * v.z); o.w = fmaf(w0, u.w, w1 * v.w);
      *(float4*)(y + (pl * Fo + j) * HW + i) = o;
    }
  } else {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += IF_T) {
      const int64_t pl = n / HW, i = n - pl * HW;
      const float* q = x + (pl * F + pr) * HW + i;
      y[(pl * Fo + j) * HW + i] = fmaf(w0, q[0], w1 * q[HW]);
    }
  }
}

extern "C" size_t emo_interp_frames_workspace_bytes(int B, int C, int F, int64_t HW) {
  if (B < 1 || C < 1 || F < 2 || HW < 1) return 0;
  return (size_t)(F - 1) * if_slices((int64_t)B * C * HW) * 3 * sizeof(float);
}
extern "C" int emo_interp_frames(const float* x, float* y, int B, int C, int F, int64_t HW, int k, int method, float dot_threshold, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  EMO_CHECK(x && y && workspace, EMO_ERR_NULL, "emo_interp_frames: null pointer");
  EMO_CHECK(B > 0 && C > 0 && F >= 2 && HW > 0 && k >= 2, EMO_ERR_BAD_SHAPE, "emo_interp_frames: B=%d C=%d F=%d HW=%lld k=%d (F >= 2, k >= 2)", B, C, F,
            (long long)HW, k);
  EMO_CHECK(method == 0 || method == 1, EMO_ERR_BAD_SHAPE, "emo_interp_frames: method %d (0 linear | 1 slerp)", method);
  const int64_t Fo64 = (int64_t)(F - 1) * k + 1;
  EMO_CHECK(HW < ((int64_t)1 << 40) && (int64_t)B * C < ((int64_t)1 << 20) && Fo64 <= 0x7fffffff &&
            (double)B * C * (double)HW * (double)Fo64 < 1.0e18, EMO_ERR_BAD_SHAPE, "emo_interp_frames: index range");
  const int Fo = (int)Fo64;
  const int64_t N = (int64_t)B * C * HW;
  const uintptr_t xa = (uintptr_t)x, xe = xa + (uintptr_t)N * F * sizeof(float), ya = (uintptr_t)y, ye = ya + (uintptr_t)N * Fo * sizeof(float);
  EMO_CHECK(ya >= xe || xa >= ye, EMO_ERR_BAD_SHAPE, "emo_interp_frames: the output overlaps the input");
  EMO_CHECK(workspace_bytes >= emo_interp_frames_workspace_bytes(B, C, F, HW), EMO_ERR_BAD_SHAPE,
            "emo_interp_frames: workspace of %llu bytes, emo_interp_frames_workspace_bytes(%d, %d, %d, %lld) = %llu",
            (unsigned long long)workspace_bytes, B, C, F, (long long)HW, (unsigned long long)emo_interp_frames_workspace_bytes(B, C, F, HW));
  const int ns = if_slices(N);
  const int64_t per = if_per(N, ns);
  const bool vec = HW % 4 == 0 && xa % 16 == 0 && ya % 16 == 0;
  hipStream_t st = as_stream(stream);
  const dim3 g1((unsigned)(F - 1), (unsigned)ns), g2((unsigned)Fo, (unsigned)ns);
  if (method == 1) {      // the linear weights need no scalars
    if (vec) interp_reduce_kernel<true><<<g1, IF_T, 0, st>>>(x, (float*)workspace, F, HW, N, per);
    else interp_reduce_kernel<false><<<g1, IF_T, 0, st>>>(x, (float*)workspace, F, HW, N, per);
    EMO_LAUNCH_CHECK();
  }
  if (vec) interp_write_kernel<true><<<g2, IF_T, 0, st>>>(x, (const float*)workspace, y, F, Fo, HW, N, per, ns, k, method, dot_threshold);
  else interp_write_kernel<false><<<g2, IF_T, 0, st>>>(x, (const float*)workspace, y, F, Fo, HW, N, per, ns, k, method, dot_threshold);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------ 8-bit output frames
// rows ((b f) h w, ld >= C) -> dense uint8 (B, F, HW, C): t = clamp(fma(x, mul, add), lo, hi), byte = trunc(t * 255).  One lane packs 16
// consecutive output bytes (they span 16 / C rows) in registers and stores them as one 16-byte vector, as dwords when y is only 4-byte
// aligned, and bytewise in the ragged tail (total need not be a multiple of 16).  Columns >= C of the rows are never addressed.
template <typename T>
__global__ __launch_bounds__(256) void rows_to_frames_u8_kernel(const T* __restrict__ x, int64_t ld, uint8_t* __restrict__ y, int64_t total, int C,
                                                                float mul, float add, float lo, float hi, int align) {
  const int64_t nvec = (total + 15) / 16;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o0 = v * 16, left = total - o0;
    int64_t row = o0 / C;
    int col = (int)(o0 - row * C);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 16; e++) {
      if (e < left) {
        const float t = fminf(fmaxf(fmaf(TT<T>::ld(x + row * ld + col), mul, add), lo), hi);
        w[e >> 2] |= (uint32_t)(uint8_t)(t * 255.0f) << (8 * (e & 3));
      }
      if (++col == C) { col = 0; row++; }
    }
    if (align == 16 && left >= 16) {
      *(uint4*)(y + o0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (align >= 4 && left >= 4 * q + 4) {
          *(uint32_t*)(y + o0 + 4 * q) = w[q];
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (4 * q + e < left) y[o0 + 4 * q + e] = (uint8_t)(w[q] >> (8 * e));
        }
      }
    }
  }
}

extern "C" int emo_rows_to_frames_u8(const void* x, int64_t ld, uint8_t* y, int B, int C, int F, int HW, float mul, float add, float lo, float hi,
                                     int dtype, void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_rows_to_frames_u8: null pointer");
  EMO_CHECK(B > 0 && C > 0 && F > 0 && HW > 0 && ld >= C, EMO_ERR_BAD_SHAPE, "emo_rows_to_frames_u8: bad shape");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_rows_to_frames_u8: dtype %d", dtype);
  const int64_t total = (int64_t)B * F * HW * C;
  const int align = ((uintptr_t)y % 16 == 0) ? 16 : (((uintptr_t)y % 4 == 0) ? 4 : 1);
  EMO_DISPATCH(dtype, "emo_rows_to_frames_u8", (rows_to_frames_u8_kernel<T><<<fgrid((total + 15) / 16, 256), 256, 0, as_stream(stream)>>>(
                                                   (const T*)x, ld, y, total, C, mul, add, lo, hi, align)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
