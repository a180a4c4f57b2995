// vision.hip - the front of the CLIP vision encoder (transformers CLIPVisionModelWithProjection, the `image_encoder` of
// EMOAnimationPipeline.py:867,909-917):
//   emo_image_preprocess : CLIPImageProcessor in one launch - antialiased bicubic resize of uint8 RGB frames, centre crop (only the
//                          crop window is computed), clamp, rescale and per-channel normalisation, all in f32
//   emo_patch_rows       : pixel_values (B, 3, S, S) f32 -> the A rows of the patch-embedding GEMM (the stride-P conv of
//                          CLIPVisionEmbeddings is a GEMM over non-overlapping patches), K padded to a multiple of 8 with zeros
//   emo_vision_embed     : class token | patch embeddings, + position embedding, then pre_layrnorm - one read, one write
// All small and memory- or latency-bound; no MFMA.
#include "common.h"

static inline int vgrid(int64_t work, int block) {
  int64_t g = (work + block - 1) / block;
  if (g > 256 * 8) g = 256 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------------------------------------------------------- preprocess
// Separable resampling from host-built tap tables (per output row / column of the CROP WINDOW: first input index, tap count, weights
// that sum to 1).  A block produces IP_TX output columns of one output row for the three channels: pass 1 filters the input columns
// it needs vertically into LDS (contiguous byte reads along the interleaved RGB row), pass 2 filters those horizontally.  Every index
// taken from a table is clamped to the image / the LDS span, so a bad table cannot read or write out of bounds.
static constexpr int IP_TX = 64;
struct IpScalars { float rescale, mean[3], sd[3]; };

__global__ __launch_bounds__(256) void image_preprocess_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int H, int W, int S,
                                                               const int32_t* __restrict__ ytap, const float* __restrict__ yw, int ky,
                                                               const int32_t* __restrict__ xtap, const float* __restrict__ xw, int kx,
                                                               int span_max, IpScalars sc) {
  extern __shared__ float col[];   // [span][3]: the vertically filtered input columns of this tile
  const int oy = blockIdx.y, n = blockIdx.z;
  const int ox0 = blockIdx.x * IP_TX, nx = S - ox0 < IP_TX ? S - ox0 : IP_TX, oxl = ox0 + nx - 1;
  int x0 = xtap[2 * ox0], x1 = xtap[2 * oxl] + xtap[2 * oxl + 1];
  x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);
  x1 = x1 > W ? W : x1;
  int span = x1 - x0;
  span = span < 0 ? 0 : (span > span_max ? span_max : span);
  int y0 = ytap[2 * oy], yn = ytap[2 * oy + 1];
  y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
  yn = yn > ky ? ky : yn;
  yn = yn > H - y0 ? H - y0 : yn;
  const int64_t row = (int64_t)W * 3;
  const uint8_t* base = img + ((int64_t)n * H + y0) * row + (int64_t)x0 * 3;
  const float* wy = yw + (int64_t)oy * ky;
  for (int i = threadIdx.x; i < span * 3; i += blockDim.x) {
    float acc = 0.f;
    for (int j = 0; j < yn; j++) acc = fmaf(wy[j], (float)base[j * row + i], acc);
    col[i] = acc;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nx * 3; t += blockDim.x) {
    const int c = t / nx, ox = ox0 + t % nx;
    int xm = xtap[2 * ox] - x0, xn = xtap[2 * ox + 1];
    xm = xm < 0 ? 0 : xm;
    xn = xn > kx ? kx : xn;
    xn = xn > span - xm ? span - xm : xn;
    const float* wx = xw + (int64_t)ox * kx;
    float acc = 0.f;
    for (int j = 0; j < xn; j++) acc = fmaf(wx[j], col[(xm + j) * 3 + c], acc);
    {
      // rescale, subtract and divide each round to f32 as the processor's three steps do: contracting the first two into one fma would
      // skip the rounding of the rescaled pixel
#pragma clang fp contract(off)
      const float v = fminf(fmaxf(acc, 0.f), 255.f) * sc.rescale;
      out[(((int64_t)n * 3 + c) * S + oy) * S + ox] = (v - sc.mean[c]) / sc.sd[c];
    }
  }
}

extern "C" int emo_image_preprocess(const uint8_t* img, float* out, int n, int H, int W, int S, const int32_t* ytap, const float* yw, int ky,
                                    const int32_t* xtap, const float* xw, int kx, int span_max, float rescale, const float* mean,
                                    const float* stddev, void* stream) {
  EMO_CHECK(img && out && ytap && yw && xtap && xw && mean && stddev, EMO_ERR_NULL, "emo_image_preprocess: null pointer");
  EMO_CHECK(n > 0 && n <= 65535 && H > 0 && W > 0 && S > 0 && S <= 65535 && ky > 0 && kx > 0 && span_max > 0 && span_max <= W, EMO_ERR_BAD_SHAPE,
            "emo_image_preprocess: n=%d H=%d W=%d S=%d ky=%d kx=%d span=%d", n, H, W, S, ky, kx, span_max);
  EMO_CHECK((int64_t)W * 3 * H <= 0x7fffffff, EMO_ERR_BAD_SHAPE, "emo_image_preprocess: frame of %d x %d too large", H, W);
  const size_t lds = (size_t)span_max * 3 * sizeof(float);
  EMO_CHECK(lds <= 64 * 1024, EMO_ERR_UNSUPPORTED, "emo_image_preprocess: %d input columns per %d-column tile exceed 64 KB of LDS (shrink factor too large)",
            span_max, IP_TX);
  EMO_CHECK(stddev[0] != 0.f && stddev[1] != 0.f && stddev[2] != 0.f, EMO_ERR_BAD_SHAPE, "emo_image_preprocess: zero std");
  IpScalars sc;
  sc.rescale = rescale;
  for (int c = 0; c < 3; c++) { sc.mean[c] = mean[c]; sc.sd[c] = stddev[c]; }
  const dim3 grid((unsigned)((S + IP_TX - 1) / IP_TX), (unsigned)S, (unsigned)n);
  image_preprocess_kernel<<<grid, 256, lds, as_stream(stream)>>>(img, out, H, W, S, ytap, yw, ky, xtap, xw, kx, span_max, sc);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ---------------------------------------------------------------------------------------------------------------- patch rows
// out[(b * G * G + gy * G + gx) * ld + (c * P + py) * P + px] = pix[b][c][gy * P + py][gx * P + px]; columns [3 P P, ld) are zero
template <typename T>
__global__ __launch_bounds__(256) void patch_rows_kernel(const float* __restrict__ pix, T* __restrict__ out, int B, int S, int P, int ld) {
  const int G = S / P, K = 3 * P * P;
  const int64_t total = (int64_t)B * G * G * ld;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int col = (int)(i % ld);
    int64_t r = i / ld;
    float v = 0.f;
    if (col < K) {
      const int px = col % P, py = (col / P) % P, c = col / (P * P);
      const int gx = (int)(r % G); r /= G;
      const int gy = (int)(r % G);
      const int64_t b = r / G;
      v = pix[((b * 3 + c) * S + gy * P + py) * S + gx * P + px];
    }
    TT<T>::st(out + i, v);
  }
}

extern "C" int emo_patch_rows(const float* pix, void* out, int B, int S, int P, int ld, int dtype, void* stream) {
  EMO_CHECK(pix && out, EMO_ERR_NULL, "emo_patch_rows: null pointer");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_patch_rows: dtype %d", dtype);
  EMO_CHECK(B > 0 && S > 0 && P > 0 && S % P == 0 && S <= 32768 && ld >= 3 * P * P, EMO_ERR_BAD_SHAPE, "emo_patch_rows: B=%d S=%d P=%d ld=%d", B, S, P, ld);
  const int64_t total = (int64_t)B * (S / P) * (S / P) * ld;
  EMO_DISPATCH(dtype, "emo_patch_rows", (patch_rows_kernel<T><<<vgrid(total, 256), 256, 0, as_stream(stream)>>>(pix, (T*)out, B, S, P, ld)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ---------------------------------------------------------------------------------------------------------------- vision embed
// One wavefront per token row: the row (class embedding or a patch embedding, + its position embedding; f32 sums) is held in
// registers, lane-strided 16-byte vectors; mean, then the centred sum of squares (two passes, like layernorm_kernel in norm.hip),
// rstd = rsqrt(var + eps); rounded once on the way out.
static constexpr int VE_MAXV = 5;

template <typename T>
__global__ __launch_bounds__(256) void vision_embed_kernel(const T* __restrict__ patch, int64_t ldp, const T* __restrict__ cls, const T* __restrict__ pos,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ y,
                                                           int64_t ldy, int B, int Np, int C, float eps) {
  constexpr int V = TT<T>::VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int CV = C / V, L = Np + 1;
  const float invC = 1.0f / (float)C;
  const int64_t M = (int64_t)B * L;
  for (int64_t m = (int64_t)blockIdx.x * 4 + wave; m < M; m += (int64_t)gridDim.x * 4) {
    const int t = (int)(m % L);
    const int64_t b = m / L;
    const T* src = t == 0 ? cls : patch + (b * Np + (t - 1)) * ldp;
    const T* pr = pos + (int64_t)t * C;
    float f[VE_MAXV][V];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VE_MAXV; j++) {
      const int cv = lane + 64 * j;
      if (cv < CV) {
        float p[V];
        unpack16<T>(*(const uint4*)(src + cv * V), f[j]);
        unpack16<T>(*(const uint4*)(pr + cv * V), p);
#pragma unroll
        for (int e = 0; e < V; e++) { f[j][e] += p[e]; s += f[j][e]; }
      }
    }
    const float mean = wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VE_MAXV; j++) {
      if (lane + 64 * j < CV) {
#pragma unroll
        for (int e = 0; e < V; e++) { const float d = f[j][e] - mean; q += d * d; }
      }
    }
    const float rstd = rsqrtf(wave_sum(q) * invC + eps);
#pragma unroll
    for (int j = 0; j < VE_MAXV; j++) {
      const int cv = lane + 64 * j;
      if (cv < CV) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; e++) o[e] = (f[j][e] - mean) * rstd * gamma[cv * V + e] + beta[cv * V + e];
        *(uint4*)(y + m * ldy + cv * V) = pack16<T>(o);
      }
    }
  }
}

extern "C" int emo_vision_embed(const void* patch, int64_t ldp, const void* cls, const void* pos, const float* gamma, const float* beta, void* y,
                                int64_t ldy, int B, int Np, int C, float eps, int dtype, void* stream) {
  EMO_CHECK(patch && cls && pos && gamma && beta && y, EMO_ERR_NULL, "emo_vision_embed: null pointer");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_vision_embed: dtype %d", dtype);
  const int V = emo_dtype_vec(dtype);
  EMO_CHECK(B > 0 && Np > 0 && C > 0 && C % V == 0 && ldp >= C && ldy >= C && ldp % V == 0 && ldy % V == 0, EMO_ERR_BAD_SHAPE,
            "emo_vision_embed: B=%d Np=%d C=%d ldp=%lld ldy=%lld", B, Np, C, (long long)ldp, (long long)ldy);
  EMO_CHECK(C / V <= 64 * VE_MAXV, EMO_ERR_UNSUPPORTED, "emo_vision_embed: C=%d too wide", C);
  EMO_CHECK(((uintptr_t)patch % 16) == 0 && ((uintptr_t)cls % 16) == 0 && ((uintptr_t)pos % 16) == 0 && ((uintptr_t)y % 16) == 0, EMO_ERR_BAD_SHAPE,
            "emo_vision_embed: 16-byte alignment");
  const int64_t M = (int64_t)B * (Np + 1);
  EMO_DISPATCH(dtype, "emo_vision_embed", (vision_embed_kernel<T><<<vgrid(M, 4), 256, 0, as_stream(stream)>>>(
                                               (const T*)patch, ldp, (const T*)cls, (const T*)pos, gamma, beta, (T*)y, ldy, B, Np, C, eps)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
