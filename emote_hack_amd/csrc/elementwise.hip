// elementwise.hip - layout conversion, channel concat, residual add, dtype convert, SiLU, timestep
// sinusoid, and the fused sampler step.  All HBM-bound: 16-byte vector accesses, grid-stride.
#include <stdarg.h>
#include "common.h"

thread_local char emo_err_buf[256] = {0};
int emo_fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(emo_err_buf, sizeof(emo_err_buf), fmt, ap); va_end(ap);
  return code;
}
extern "C" int emo_version(void) { return 200; }   // round 2: emo_attention_params.seg1_row, LayerNorm-folded GEMM
extern "C" const char* emo_last_error_string(void) { return emo_err_buf; }

static inline int grid_for(int64_t work, int block) {
  int64_t g = (work + block - 1) / block;
  if (g > 256 * 8) g = 256 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------- (B,C,F,H,W) f32 <-> rows
// Tile transpose through LDS: a block moves a [32 channels x 64 pixels] tile so both sides are coalesced.
template <typename T>
__global__ __launch_bounds__(256) void ncfhw_to_rows_kernel(const float* __restrict__ x, T* __restrict__ y, int B, int C,
                                                            int F, int HW, int Cpad, int ldo) {
  __shared__ float tile[32][65];
  const int ptiles = (HW + 63) / 64, ctiles = (Cpad + 31) / 32;
  const int64_t ntiles = (int64_t)B * F * ptiles * ctiles;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int ct = t % ctiles; int64_t r = t / ctiles;
    int pt = r % ptiles; r /= ptiles;
    int f = r % F; int b = r / F;
    for (int i = threadIdx.x; i < 32 * 64; i += 256) {
      int c = i / 64, p = i % 64;
      int cc = ct * 32 + c, pp = pt * 64 + p;
      float v = 0.f;
      if (cc < C && pp < HW) v = x[(((int64_t)b * C + cc) * F + f) * HW + pp];
      tile[c][p] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * 64; i += 256) {
      int p = i / 32, c = i % 32;
      int cc = ct * 32 + c, pp = pt * 64 + p;
      if (cc < Cpad && pp < HW) TT<T>::st(&y[((int64_t)(b * F + f) * HW + pp) * ldo + cc], tile[c][p]);
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(256) void rows_to_ncfhw_kernel(const T* __restrict__ x, float* __restrict__ y, int B, int C,
                                                            int F, int HW, int ldi) {
  __shared__ float tile[32][65];
  const int ptiles = (HW + 63) / 64, ctiles = (C + 31) / 32;
  const int64_t ntiles = (int64_t)B * F * ptiles * ctiles;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int ct = t % ctiles; int64_t r = t / ctiles;
    int pt = r % ptiles; r /= ptiles;
    int f = r % F; int b = r / F;
    for (int i = threadIdx.x; i < 32 * 64; i += 256) {
      int p = i / 32, c = i % 32;
      int cc = ct * 32 + c, pp = pt * 64 + p;
      float v = 0.f;
      if (cc < C && pp < HW) v = TT<T>::ld(&x[((int64_t)(b * F + f) * HW + pp) * ldi + cc]);
      tile[c][p] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * 64; i += 256) {
      int c = i / 64, p = i % 64;
      int cc = ct * 32 + c, pp = pt * 64 + p;
      if (cc < C && pp < HW) y[(((int64_t)b * C + cc) * F + f) * HW + pp] = tile[c][p];
    }
    __syncthreads();
  }
}

extern "C" int emo_ncfhw_to_rows(const float* x, void* y, int B, int C, int F, int H, int W, int Cpad, int ldo,
                                 int dtype, void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_ncfhw_to_rows: null pointer");
  EMO_CHECK(B > 0 && C > 0 && F > 0 && H > 0 && W > 0 && Cpad >= C && ldo >= Cpad, EMO_ERR_BAD_SHAPE,
            "emo_ncfhw_to_rows: bad shape B=%d C=%d F=%d H=%d W=%d Cpad=%d ldo=%d", B, C, F, H, W, Cpad, ldo);
  int HW = H * W;
  int64_t ntiles = (int64_t)B * F * ((HW + 63) / 64) * ((Cpad + 31) / 32);
  int grid = (int)(ntiles < 4096 ? ntiles : 4096);
  EMO_DISPATCH(dtype, "emo_ncfhw_to_rows", (ncfhw_to_rows_kernel<T><<<grid, 256, 0, as_stream(stream)>>>(x, (T*)y, B, C, F, HW, Cpad, ldo)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

extern "C" int emo_rows_to_ncfhw(const void* x, float* y, int B, int C, int F, int H, int W, int ldi, int dtype,
                                 void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_rows_to_ncfhw: null pointer");
  EMO_CHECK(B > 0 && C > 0 && F > 0 && H > 0 && W > 0 && ldi >= C, EMO_ERR_BAD_SHAPE, "emo_rows_to_ncfhw: bad shape");
  int HW = H * W;
  int64_t ntiles = (int64_t)B * F * ((HW + 63) / 64) * ((C + 31) / 32);
  int grid = (int)(ntiles < 4096 ? ntiles : 4096);
  EMO_DISPATCH(dtype, "emo_rows_to_ncfhw", (rows_to_ncfhw_kernel<T><<<grid, 256, 0, as_stream(stream)>>>((const T*)x, y, B, C, F, HW, ldi)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ---------------------------------------------------------------- copy columns / add (16-byte vectors)
template <typename T>
__global__ __launch_bounds__(256) void copy_cols_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, int coff,
                                                        int64_t M, int C) {
  constexpr int V = TT<T>::VEC;
  const int cv = C / V;
  const int64_t total = M * cv;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t m = i / cv; int c = (int)(i % cv) * V;
    *(uint4*)(y + m * ldy + coff + c) = *(const uint4*)(x + m * ldx + c);
  }
}
extern "C" int emo_copy_cols(const void* x, int ldx, void* y, int ldy, int coff, int64_t M, int C, int dtype, void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_copy_cols: null pointer");
  int V = emo_dtype_vec(dtype);
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_copy_cols: dtype %d", dtype);
  EMO_CHECK(M > 0 && C > 0 && C % V == 0 && coff % V == 0 && ldx % V == 0 && ldy % V == 0 && coff + C <= ldy && C <= ldx,
            EMO_ERR_BAD_SHAPE, "emo_copy_cols: C=%d coff=%d ldx=%d ldy=%d must be multiples of %d", C, coff, ldx, ldy, V);
  int grid = grid_for(M * (C / V), 256);
  EMO_DISPATCH(dtype, "emo_copy_cols", (copy_cols_kernel<T><<<grid, 256, 0, as_stream(stream)>>>((const T*)x, ldx, (T*)y, ldy, coff, M, C)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void add_kernel(const T* __restrict__ a, int lda, const T* __restrict__ b, int ldb, float alpha,
                                                  T* __restrict__ y, int ldy, int64_t M, int C) {
  constexpr int V = TT<T>::VEC;
  const int cv = C / V;
  const int64_t total = M * cv;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t m = i / cv; int c = (int)(i % cv) * V;
    float fa[V], fb[V];
    unpack16<T>(*(const uint4*)(a + m * lda + c), fa);
    unpack16<T>(*(const uint4*)(b + m * ldb + c), fb);
#pragma unroll
    for (int j = 0; j < V; j++) fa[j] += alpha * fb[j];
    *(uint4*)(y + m * ldy + c) = pack16<T>(fa);
  }
}
extern "C" int emo_add(const void* a, int lda, const void* b, int ldb, float alpha, void* y, int ldy, int64_t M, int C,
                       int dtype, void* stream) {
  EMO_CHECK(a && b && y, EMO_ERR_NULL, "emo_add: null pointer");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_add: dtype %d", dtype);
  int V = emo_dtype_vec(dtype);
  EMO_CHECK(M > 0 && C > 0 && C % V == 0 && lda % V == 0 && ldb % V == 0 && ldy % V == 0, EMO_ERR_BAD_SHAPE, "emo_add: bad shape");
  int grid = grid_for(M * (C / V), 256);
  EMO_DISPATCH(dtype, "emo_add", (add_kernel<T><<<grid, 256, 0, as_stream(stream)>>>((const T*)a, lda, (const T*)b, ldb, alpha, (T*)y, ldy, M, C)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// y[m, :] = x[m, :] + f[m % P, :]: a (P, C) map added to every period of P rows (the face-region features behind conv_in, one period
// per frame).  y may BE x (no __restrict__ on the two): every element is read, added in f32 and written by the same thread.
template <typename T>
__global__ __launch_bounds__(256) void add_periodic_kernel(const T* x, int64_t ldx, const T* __restrict__ f, int64_t ldf, T* y, int64_t ldy,
                                                           int64_t M, int C, int64_t P) {
  constexpr int V = TT<T>::VEC;
  const int cv = C / V;
  const int64_t total = M * cv;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / cv; const int c = (int)(i % cv) * V;
    float fx[V], ff[V];
    unpack16<T>(*(const uint4*)(x + m * ldx + c), fx);
    unpack16<T>(*(const uint4*)(f + (m % P) * ldf + c), ff);
#pragma unroll
    for (int j = 0; j < V; j++) fx[j] += ff[j];
    *(uint4*)(y + m * ldy + c) = pack16<T>(fx);
  }
}
extern "C" int emo_add_periodic(const void* x, int64_t ldx, const void* f, int64_t ldf, void* y, int64_t ldy, int64_t M, int C, int64_t P,
                                int dtype, void* stream) {
  EMO_CHECK(x && f && y, EMO_ERR_NULL, "emo_add_periodic: null pointer");
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_add_periodic: dtype %d", dtype);
  const int V = emo_dtype_vec(dtype);
  EMO_CHECK(M > 0 && C > 0 && P > 0 && C % V == 0 && ldx % V == 0 && ldf % V == 0 && ldy % V == 0 && ldx >= C && ldf >= C && ldy >= C,
            EMO_ERR_BAD_SHAPE, "emo_add_periodic: M=%lld C=%d P=%lld ldx=%lld ldf=%lld ldy=%lld (widths multiples of %d)", (long long)M, C,
            (long long)P, (long long)ldx, (long long)ldf, (long long)ldy, V);
  EMO_CHECK(M % P == 0, EMO_ERR_BAD_SHAPE, "emo_add_periodic: M=%lld is not a whole number of periods of P=%lld rows", (long long)M, (long long)P);
  EMO_CHECK(((uintptr_t)x % 16) == 0 && ((uintptr_t)f % 16) == 0 && ((uintptr_t)y % 16) == 0, EMO_ERR_BAD_SHAPE,
            "emo_add_periodic: operands must be 16-byte aligned");
  const int grid = grid_for(M * (C / V), 256);
  EMO_DISPATCH(dtype, "emo_add_periodic",
               (add_periodic_kernel<T><<<grid, 256, 0, as_stream(stream)>>>((const T*)x, ldx, (const T*)f, ldf, (T*)y, ldy, M, C, P)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// (Hp, Wp) f32 map -> (Hp / 8 * Wp / 8, 8) rows: channel 0 = the mean of the cell's 8 x 8 pixels (of x > thr ? 1 : 0 with use_thr),
// channels 1..7 = 0.  One thread per cell: 64 loads summed in row-major order, one multiply by 1/64 (exact), one 8-channel store.
template <typename T>
__global__ __launch_bounds__(256) void mask_pool_kernel(const float* __restrict__ x, T* __restrict__ y, int Hc, int Wc, int Wp, int use_thr,
                                                        float thr) {
  const int n = Hc * Wc;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int cy = i / Wc, cx = i % Wc;
    const float* p = x + (int64_t)cy * 8 * Wp + cx * 8;
    float s = 0.f;
    for (int r = 0; r < 8; r++) {
      const float4 a = *(const float4*)(p + (int64_t)r * Wp), b = *(const float4*)(p + (int64_t)r * Wp + 4);
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 8; j++) s += use_thr ? (v[j] > thr ? 1.0f : 0.0f) : v[j];
    }
    T* o = y + (int64_t)i * 8;
    TT<T>::st(o, s * 0.015625f);
#pragma unroll
    for (int j = 1; j < 8; j++) TT<T>::st(o + j, 0.0f);
  }
}
extern "C" int emo_mask_pool(const float* x, void* y, int Hp, int Wp, int use_thr, float thr, int dtype, void* stream) {
  EMO_CHECK(emo_dtype_ok(dtype), EMO_ERR_BAD_DTYPE, "emo_mask_pool: dtype %d", dtype);
  EMO_CHECK(Hp > 0 && Wp > 0 && Hp % 8 == 0 && Wp % 8 == 0, EMO_ERR_BAD_SHAPE, "emo_mask_pool: Hp=%d Wp=%d must be multiples of 8", Hp, Wp);
  EMO_CHECK((int64_t)Hp * Wp < ((int64_t)1 << 31), EMO_ERR_BAD_SHAPE, "emo_mask_pool: %d x %d pixels (at most 2^31 - 1)", Hp, Wp);
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_mask_pool: null pointer");
  EMO_CHECK(((uintptr_t)x % 16) == 0, EMO_ERR_BAD_SHAPE, "emo_mask_pool: the map must be 16-byte aligned");
  const int Hc = Hp / 8, Wc = Wp / 8;
  const int grid = grid_for((int64_t)Hc * Wc, 256);
  EMO_DISPATCH(dtype, "emo_mask_pool", (mask_pool_kernel<T><<<grid, 256, 0, as_stream(stream)>>>(x, (T*)y, Hc, Wc, Wp, use_thr, thr)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ---------------------------------------------------------------- convert / silu (scalar tails allowed)
__device__ __forceinline__ float round_through_half(float f) { return (float)(_Float16)f; }  // IEEE half, RNE

template <typename S, typename D>
__global__ __launch_bounds__(256) void convert_kernel(const S* __restrict__ s, D* __restrict__ d, int64_t n, int fp16_round) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = TT<S>::ld(s + i);
    if (fp16_round) v = round_through_half(v);
    TT<D>::st(d + i, v);
  }
}
extern "C" int emo_convert(const void* src, int sdt, void* dst, int ddt, int64_t n, int fp16_round, void* stream) {
  EMO_CHECK(src && dst, EMO_ERR_NULL, "emo_convert: null pointer");
  EMO_CHECK(n > 0, EMO_ERR_BAD_SHAPE, "emo_convert: n=%lld", (long long)n);
  int grid = grid_for(n, 256);
  hipStream_t st = as_stream(stream);
  EMO_CHECK(emo_dtype_ok(sdt) && emo_dtype_ok(ddt), EMO_ERR_BAD_DTYPE, "emo_convert: dtypes %d -> %d", sdt, ddt);
  EMO_DISPATCH(sdt, "emo_convert", {
    using S = T;
    const S* sp = (const S*)src;
    if (ddt == EMO_F32) convert_kernel<S, float><<<grid, 256, 0, st>>>(sp, (float*)dst, n, fp16_round);
    else if (ddt == EMO_BF16) convert_kernel<S, bf16_t><<<grid, 256, 0, st>>>(sp, (bf16_t*)dst, n, fp16_round);
    else convert_kernel<S, f16_t><<<grid, 256, 0, st>>>(sp, (f16_t*)dst, n, fp16_round);
  });
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void silu_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = TT<T>::ld(x + i);
    TT<T>::st(y + i, v == -INFINITY ? -0.f : silu_f(v));   // (the limit at -inf, where x * sigmoid(x) is -inf * 0)
  }
}
extern "C" int emo_silu(const void* x, void* y, int64_t n, int dtype, void* stream) {
  EMO_CHECK(x && y, EMO_ERR_NULL, "emo_silu: null pointer");
  EMO_CHECK(n > 0, EMO_ERR_BAD_SHAPE, "emo_silu: n");
  int grid = grid_for(n, 256);
  EMO_DISPATCH(dtype, "emo_silu", (silu_kernel<T><<<grid, 256, 0, as_stream(stream)>>>((const T*)x, (T*)y, n)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ---------------------------------------------------------------- timestep sinusoid
// embeddings.py:46-63: emb = t.float() * exp(exponent); [sin | cos], flipped to [cos | sin] when
// flip_sin_to_cos.  `freqs` = exp(-ln(max_period) * arange(half) / (half - shift)) is a constant f32
// table built once on the host exactly as the reference builds it, so the angle t*freq is the same
// f32 product (an on-device expf would move the k=0 angle of t=981 by ~1e-4 rad).
// TS = int64_t (the integer tables) or float (the fractional timesteps of the sigma-space samplers): for an integral value both
// round to the same f32, so the two entries give the same bits.
template <typename T, typename TS>
__global__ void timestep_kernel(const TS* __restrict__ ts, const float* __restrict__ freqs, T* __restrict__ out, int B,
                                int dim, int flip) {
  const int half = dim / 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * dim; i += gridDim.x * blockDim.x) {
    int b = i / dim, j = i % dim;
    float v = 0.f;
    if (j < 2 * half) {
      int k = j % half;
      bool second = j >= half;
      float ang = (float)ts[b] * freqs[k];
      bool want_cos = flip ? !second : second;
      v = want_cos ? cosf(ang) : sinf(ang);
    }
    TT<T>::st(out + i, v);
  }
}
extern "C" int emo_timestep_embedding(const int64_t* ts, const float* freqs, void* out, int B, int dim, int flip, int dtype,
                                      void* stream) {
  EMO_CHECK(ts && out && freqs, EMO_ERR_NULL, "emo_timestep_embedding: null pointer");
  EMO_CHECK(B > 0 && dim > 1, EMO_ERR_BAD_SHAPE, "emo_timestep_embedding: B=%d dim=%d", B, dim);
  int grid = grid_for((int64_t)B * dim, 256);
  EMO_DISPATCH(dtype, "emo_timestep_embedding", (timestep_kernel<T, int64_t><<<grid, 256, 0, as_stream(stream)>>>(ts, freqs, (T*)out, B, dim, flip)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
extern "C" int emo_timestep_embedding_f32(const float* ts, const float* freqs, void* out, int B, int dim, int flip, int dtype,
                                          void* stream) {
  EMO_CHECK(ts && out && freqs, EMO_ERR_NULL, "emo_timestep_embedding_f32: null pointer");
  EMO_CHECK(B > 0 && dim > 1, EMO_ERR_BAD_SHAPE, "emo_timestep_embedding_f32: B=%d dim=%d", B, dim);
  int grid = grid_for((int64_t)B * dim, 256);
  EMO_DISPATCH(dtype, "emo_timestep_embedding_f32", (timestep_kernel<T, float><<<grid, 256, 0, as_stream(stream)>>>(ts, freqs, (T*)out, B, dim, flip)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ---------------------------------------------------------------- sampler: CFG + window average + linear multistep step
// Every scheduler of the loop (DDIM, DDPM, DPM-Solver++ 2M, Euler, Euler-ancestral, LMS) as one linear form over the f32 latents,
// see include/emo_hip.h.  One element: read x and the ring entries before writing anything of element i, so x' may overwrite x in
// place.  z is a pure function of (seed, step, i): every rank draws the same bits without communication.
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x = (x ^ (x >> 16)) * 0x7FEB352Du;
  x = (x ^ (x >> 15)) * 0x846CA68Bu;
  x = x ^ (x >> 16);
  return x;
}

// npu / npc: noise_pred of element i in the uncond / cond plane (npc unused without guidance); x0: its latent; cnt: the counter
// of its frame.
__device__ __forceinline__ float sched_elem(float npu, float npc, float x0, float cnt, float* __restrict__ hist,
                                            float* __restrict__ eps_out, int i, int n, const emo_sched_step_params& p,
                                            uint32_t key) {
  const float inv = 1.0f / cnt;
  float eps = npu * inv;
  // CFG with c*inv - uc in one rounding, written out so that the bits do not depend on the compiler: left to it, u*inv and c*inv
  // were paired into one packed multiply, which rounds c*inv first (tests/golden/sched_ddim_ddpm.safetensors pins the bits)
  if (p.guidance_scale > 1.0f) eps = fmaf(p.guidance_scale, fmaf(npc, inv, -eps), eps);
  const float d = p.a * x0 + p.b * eps;
  float x = p.c_x * x0 + p.c[0] * d;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (p.slot[k] >= 0) x += p.c[k] * hist[(size_t)p.slot[k] * n + i];
  if (p.slot[0] >= 0) hist[(size_t)p.slot[0] * n + i] = d;
  if (p.c_noise != 0.f) {
    const float c_n = p.c_noise;
    uint32_t h1 = mix32(((uint32_t)i * 2u + 0u) ^ key), h2 = mix32(((uint32_t)i * 2u + 1u) ^ key);
    float u1 = ((float)h1 + 1.0f) * 2.3283064365386963e-10f;  // (0,1]
    float u2 = (float)h2 * 2.3283064365386963e-10f;
    x += c_n * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
  }
  if (eps_out) eps_out[i] = eps;
  return x;
}

// x_in = s * x: the model input of the first step that runs (emo_sched_step with scale_only)
template <bool VEC>
__global__ __launch_bounds__(256) void sched_scale_kernel(const float* __restrict__ lat, float* __restrict__ lat_in, int n, float s) {
  const int stride = gridDim.x * blockDim.x;
  if (VEC) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / 4; g += stride) {
      float4 v = reinterpret_cast<const float4*>(lat)[g];
      v.x *= s; v.y *= s; v.z *= s; v.w *= s;
      reinterpret_cast<float4*>(lat_in)[g] = v;
    }
  } else {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) lat_in[i] = s * lat[i];
  }
}

// VEC: n % 4 == 0 and every base 16-byte aligned -> float4 accesses of the eps planes, x, x' and x_in (the ring entries stay per
// element; the frame of each lane is its own when HW is not a multiple of 4); otherwise one element per iteration.
template <bool VEC>
__global__ __launch_bounds__(256) void sched_step_kernel(const float* __restrict__ np, const float* __restrict__ counter,
                                                         float* __restrict__ lat, float* __restrict__ hist, float* __restrict__ lat_in,
                                                         float* __restrict__ eps_out, int C, int F, int HW, emo_sched_step_params p) {
  const int n = C * F * HW;   // < 2^31 (checked by the entry)
  const int stride = gridDim.x * blockDim.x;
  const uint32_t key = mix32(p.seed ^ mix32(p.step + 0x9E3779B9u));
  if (VEC) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n / 4; g += stride) {
      const int i = g * 4;
      const float4 u = reinterpret_cast<const float4*>(np)[g];
      const float4 c = p.guidance_scale > 1.0f ? reinterpret_cast<const float4*>(np + n)[g] : u;
      const float4 x = reinterpret_cast<const float4*>(lat)[g];
      // frame of each lane: one division for the group, then step the pixel (HW may be < 4 or not a multiple of 4)
      const int q = (int)((unsigned)i / (unsigned)HW);
      int px = i - q * HW, f = (int)((unsigned)q % (unsigned)F);
      float cnt[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cnt[j] = counter[f];
        if (++px == HW) { px = 0; f = (f + 1 == F) ? 0 : f + 1; }
      }
      float4 o;
      o.x = sched_elem(u.x, c.x, x.x, cnt[0], hist, eps_out, i + 0, n, p, key);
      o.y = sched_elem(u.y, c.y, x.y, cnt[1], hist, eps_out, i + 1, n, p, key);
      o.z = sched_elem(u.z, c.z, x.z, cnt[2], hist, eps_out, i + 2, n, p, key);
      o.w = sched_elem(u.w, c.w, x.w, cnt[3], hist, eps_out, i + 3, n, p, key);
      reinterpret_cast<float4*>(lat)[g] = o;
      if (lat_in) reinterpret_cast<float4*>(lat_in)[g] = make_float4(p.s_next * o.x, p.s_next * o.y, p.s_next * o.z, p.s_next * o.w);
    }
  } else {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const float x = sched_elem(np[i], p.guidance_scale > 1.0f ? np[n + i] : 0.f, lat[i], counter[((unsigned)i / (unsigned)HW) % (unsigned)F],
                                 hist, eps_out, i, n, p, key);
      lat[i] = x;
      if (lat_in) lat_in[i] = p.s_next * x;
    }
  }
}
static inline bool aligned16(const void* q) { return q == nullptr || ((uintptr_t)q & 15u) == 0; }
extern "C" int emo_sched_step(const float* np, const float* counter, float* lat, float* hist, float* lat_in, float* eps_out, int C, int F,
                              int HW, const emo_sched_step_params* p, void* stream) {
  EMO_CHECK(p && lat, EMO_ERR_NULL, "emo_sched_step: null pointer");
  EMO_CHECK(C > 0 && F > 0 && HW > 0, EMO_ERR_BAD_SHAPE, "emo_sched_step: bad shape");
  const int64_t n = (int64_t)C * F * HW;
  EMO_CHECK(n < ((int64_t)1 << 31), EMO_ERR_BAD_SHAPE, "emo_sched_step: %lld elements (at most 2^31 - 1)", (long long)n);
  if (p->scale_only) {
    EMO_CHECK(lat_in != nullptr, EMO_ERR_NULL, "emo_sched_step: scale_only needs lat_in");
  } else {
    EMO_CHECK(np && counter, EMO_ERR_NULL, "emo_sched_step: null pointer");
    for (int k = 0; k < 4; ++k) {
      EMO_CHECK(p->slot[k] >= -1 && p->slot[k] < EMO_SCHED_RING, EMO_ERR_BAD_SHAPE, "emo_sched_step: slot[%d]=%d", k, p->slot[k]);
      EMO_CHECK(p->slot[k] < 0 || hist != nullptr, EMO_ERR_NULL, "emo_sched_step: slot[%d] set without a history ring", k);
    }
    for (int k = 1; k < 4; ++k)   // the entry written this step is never one read this step
      EMO_CHECK(p->slot[k] < 0 || p->slot[k] != p->slot[0], EMO_ERR_BAD_SHAPE, "emo_sched_step: slot[%d] == slot[0]", k);
  }
  const bool vec = (n % 4 == 0) && aligned16(np) && aligned16(lat) && aligned16(lat_in);
  const int grid = grid_for(vec ? n / 4 : n, 256);
  hipStream_t st = as_stream(stream);
  if (p->scale_only) {
    if (vec) sched_scale_kernel<true><<<grid, 256, 0, st>>>(lat, lat_in, (int)n, p->s_next);
    else sched_scale_kernel<false><<<grid, 256, 0, st>>>(lat, lat_in, (int)n, p->s_next);
  } else if (vec) {
    sched_step_kernel<true><<<grid, 256, 0, st>>>(np, counter, lat, hist, lat_in, eps_out, C, F, HW, *p);
  } else {
    sched_step_kernel<false><<<grid, 256, 0, st>>>(np, counter, lat, hist, lat_in, eps_out, C, F, HW, *p);
  }
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void accumulate_window_kernel(const T* __restrict__ pred, int ld, float* __restrict__ np,
                                                                float* __restrict__ counter, const int32_t* __restrict__ frames,
                                                                int nf, int C, int F, int HW, int add_counter) {
  const int64_t n = (int64_t)nf * HW * C;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(i % C); int64_t r = i / C;
    int p = (int)(r % HW); int j = (int)(r / HW);
    int f = frames[j];
    if (f < 0) continue;   // position dropped by the host: an earlier duplicate of a frame inside one window
    np[((int64_t)c * F + f) * HW + p] += TT<T>::ld(pred + r * ld + c);
  }
  if (add_counter && blockIdx.x == 0 && threadIdx.x < nf && frames[threadIdx.x] >= 0) counter[frames[threadIdx.x]] += 1.0f;
}
extern "C" int emo_accumulate_window(const void* pred, int ld, float* np, float* counter, const int32_t* frames, int nf, int C,
                                     int F, int HW, int add_counter, int dtype, void* stream) {
  EMO_CHECK(pred && np && counter && frames, EMO_ERR_NULL, "emo_accumulate_window: null pointer");
  EMO_CHECK(nf > 0 && nf <= 256 && C > 0 && ld >= C, EMO_ERR_BAD_SHAPE, "emo_accumulate_window: bad shape");
  int grid = grid_for((int64_t)nf * HW * C, 256);
  EMO_DISPATCH(dtype, "emo_accumulate_window", (accumulate_window_kernel<T><<<grid, 256, 0, as_stream(stream)>>>((const T*)pred, ld, np, counter, frames, nf, C, F, HW, add_counter)));
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
