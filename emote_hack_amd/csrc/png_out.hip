// png_out.hip - the device half of the PNG / APNG writer, the lossless file beside the Motion-JPEG AVI and the GIF (`save_images_grid`,
// magicanimate/utils/util.py:35-41; emote_hack_amd/video_io.py is the host half: the Huffman tables, the block header, the checksum's
// combination and the chunks).  What every entry computes is stated in include/emo_hip.h; how:
//   emo_png_filter        : ONE wavefront per scanline.  Adaptive: a first pass sums min(v, 256 - v) of all five filter types at once (lane l
//                           the bytes l, l + 64, ..), a butterfly adds the lanes, the lowest type keeps a tie; the second pass writes the
//                           chosen type's bytes and sums the row's Adler-32 pair.  Rows read raw rows only, so they are independent
//   emo_png_lz_count      : ONE wavefront per strip, the strip's bytes and the 4096-entry hash table in LDS (8 KiB + 1.25 KiB + the strip:
//                           11 KiB for one row of 512 RGB pixels, 21 KiB for eight).  The walk is wave-uniform - every lane reads the same
//                           three bytes (an LDS broadcast) and probes the same slot - and the 64 lanes compare 64 bytes of the match
//                           prefix per step: a ballot, its trailing ones.  Tokens collect in a register per lane and leave 64 at a time;
//                           the symbol counts collect in LDS and are added to the frame's histogram once per strip
//   emo_png_deflate_bits  : one workgroup per strip, one lane per token: the code lengths and extra bits under the frame's table, summed
//   emo_png_deflate_emit  : one workgroup per strip, 256 tokens per step: a scan of their sizes gives each its bit position, and its
//                           codes are OR-ed least-significant-bit first into the zeroed stream (32-bit atomicOr: strips and frames share
//                           words)
// Byte work; no MFMA.
#include "common.h"

#define PNG_ADLER 65521u
#define PNG_HASH_SLOTS 4096
#define PNG_EMPTY 0xFFFF
#define PNG_MAX_STRIP 65535
#define PNG_MAX_MATCH 258
#define PNG_MAX_DIST 32768
#define PNG_SYMBOLS 320            // 0 .. 285 literal / length, 288 .. 317 distance
#define PNG_DIST0 288
#define PNG_EOB 256
#define PNG_LDS_FIXED (PNG_HASH_SLOTS * 2 + PNG_SYMBOLS * 4)

struct png_shape {
  int n, H, W, C;
  int64_t row;                       // bytes of a filtered scanline: 1 + W * C
  int strip_rows, per_frame;         // per_frame: strips of a frame, the last may be short
  int64_t n_strips, cap;             // cap: tokens of the scratch buffer per strip = bytes of a full strip
};

static int png_frame_args(const char* who, int n, int H, int W, int C, png_shape* s) {
  EMO_CHECK(C == 1 || C == 3 || C == 4, EMO_ERR_BAD_SHAPE, "%s: C=%d (1: grey, 3: RGB, 4: RGBA; 8 bits each)", who, C);
  EMO_CHECK(n > 0 && H > 0 && W > 0, EMO_ERR_BAD_SHAPE, "%s: n=%d H=%d W=%d (at least 1 each)", who, n, H, W);
  const int64_t row = 1 + (int64_t)W * C;
  EMO_CHECK(row <= 0x7FFFFFFFLL && (int64_t)H <= 0x7FFFFFFFLL / row, EMO_ERR_BAD_SHAPE,
            "%s: H=%d rows of %lld filtered bytes; a frame's filtered bytes are counted in 31 bits", who, H, (long long)row);
  s->n = n; s->H = H; s->W = W; s->C = C; s->row = row;
  return EMO_OK;
}

static int png_strip_args(const char* who, int n, int H, int W, int C, int strip_rows, png_shape* s) {
  const int rc = png_frame_args(who, n, H, W, C, s);
  if (rc != EMO_OK) return rc;
  EMO_CHECK(strip_rows >= 1, EMO_ERR_BAD_SHAPE, "%s: strip_rows=%d", who, strip_rows);
  if (strip_rows > H) strip_rows = H;
  EMO_CHECK((int64_t)strip_rows * s->row <= PNG_MAX_STRIP, EMO_ERR_BAD_SHAPE, "%s: a strip of %d rows of %lld bytes; at most 65535 bytes per strip "
            "(the hash table holds 16-bit offsets)", who, strip_rows, (long long)s->row);
  s->strip_rows = strip_rows;
  s->per_frame = (H + strip_rows - 1) / strip_rows;
  s->n_strips = (int64_t)s->per_frame * n;
  s->cap = (int64_t)strip_rows * s->row;
  return EMO_OK;
}

extern "C" int64_t emo_png_tokens_per_strip(int H, int W, int C, int strip_rows) {
  if (H < 1 || W < 1 || strip_rows < 1 || !(C == 1 || C == 3 || C == 4)) return 0;
  return (int64_t)(strip_rows < H ? strip_rows : H) * (1 + (int64_t)W * C);
}

// ------------------------------------------------------------------------------------------------------------------------ filter
__device__ __forceinline__ int png_paeth(int a, int b, int c) {               // PNG 9.4: a on ties, then b
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint32_t png_filtered(int t, int x, int a, int b, int c) {
  const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
  return (uint32_t)(x - pred) & 255u;
}

__device__ __forceinline__ uint64_t png_wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}

// four wavefronts per workgroup, each a scanline of its own
__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ filt, uint32_t* __restrict__ adler,
                                                         int64_t rows, int H, int64_t L, int C, int filter) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {       // wave-uniform
    const uint8_t* src = frames + r * L;
    const bool top = r % H == 0;                                                 // the row above a frame's first row is zeros
    const uint8_t* up = top ? src : src - L;                                     // never read through when top
    int t = filter;
    if (filter == 5) {
      uint64_t cost[5] = {0, 0, 0, 0, 0};
      for (int64_t j = lane; j < L; j += 64) {
        const int x = src[j], a = j >= C ? src[j - C] : 0, b = top ? 0 : up[j], c = (top || j < C) ? 0 : up[j - C];
#pragma unroll
        for (int k = 0; k < 5; k++) {
          const uint32_t v = png_filtered(k, x, a, b, c);
          cost[k] += v < 128 ? v : 256 - v;                                      // min(v, 256 - v)
        }
      }
      uint64_t best = 0;
#pragma unroll
      for (int k = 0; k < 5; k++) {
        const uint64_t ck = png_wave_sum(cost[k]);
        if (k == 0 || ck < best) { best = ck; t = k; }                           // strictly below: the lowest type keeps a tie
      }
    }
    uint8_t* dst = filt + r * (L + 1);
    uint64_t s1 = 0, s2 = 0;
    for (int64_t j = lane; j < L; j += 64) {
      const int x = src[j], a = j >= C ? src[j - C] : 0, b = top ? 0 : up[j], c = (top || j < C) ? 0 : up[j - C];
      const uint32_t v = png_filtered(t, x, a, b, c);
      dst[1 + j] = (uint8_t)v;
      s1 += v;
      s2 += (uint64_t)((uint64_t)(L - j) % PNG_ADLER) * v;                       // byte 1 + j of L + 1 is added to s2 L - j times
    }
    s1 = png_wave_sum(s1);
    s2 = png_wave_sum(s2);
    if (lane == 0) {
      dst[0] = (uint8_t)t;
      const uint64_t N = (uint64_t)(L + 1) % PNG_ADLER;
      adler[2 * r] = (uint32_t)((1 + t + s1) % PNG_ADLER);
      adler[2 * r + 1] = (uint32_t)((N + N * t + s2) % PNG_ADLER);
    }
  }
}

extern "C" int emo_png_filter(const uint8_t* frames, uint8_t* filtered, uint32_t* adler, int n, int H, int W, int C, int filter, void* stream) {
  EMO_CHECK(frames && filtered && adler, EMO_ERR_NULL, "emo_png_filter: null pointer");
  png_shape s;
  const int rc = png_frame_args("emo_png_filter", n, H, W, C, &s);
  if (rc != EMO_OK) return rc;
  EMO_CHECK(filter >= 0 && filter <= 5, EMO_ERR_BAD_SHAPE, "emo_png_filter: filter=%d (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth, 5 adaptive)", filter);
  EMO_CHECK((uintptr_t)adler % 4 == 0, EMO_ERR_BAD_SHAPE, "emo_png_filter: adler must be 4-byte aligned");
  const int64_t rows = (int64_t)n * H, g = (rows + 3) / 4;
  png_filter_kernel<<<(int)(g < 8192 ? g : 8192), 256, 0, as_stream(stream)>>>(frames, filtered, adler, rows, H, s.row - 1, C, filter);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ tokens
// RFC 1951 3.2.5.  length 3 .. 258 -> symbol 257 .. 285, the number of extra bits and their value
__device__ __forceinline__ void png_length_symbol(uint32_t len, int& sym, int& nx, uint32_t& x) {
  const uint32_t l = len - 3;
  if (l >= 255) { sym = 285; nx = 0; x = 0; return; }
  if (l < 8) { sym = 257 + (int)l; nx = 0; x = 0; return; }
  nx = 29 - __clz(l);                                                            // floor(log2 l) - 2
  sym = 261 + 4 * nx + (int)((l >> nx) & 3);
  x = l & ((1u << nx) - 1);
}
// distance 1 .. 32768 -> symbol 0 .. 29
__device__ __forceinline__ void png_distance_symbol(uint32_t dist, int& sym, int& nx, uint32_t& x) {
  const uint32_t d = (dist - 1) & 32767u;
  if (d < 4) { sym = (int)d; nx = 0; x = 0; return; }
  nx = 30 - __clz(d);                                                            // floor(log2 d) - 1
  sym = 2 * nx + 2 + (int)((d >> nx) & 1);
  x = d & ((1u << nx) - 1);
}

// one wavefront per strip
__global__ __launch_bounds__(64) void png_lz_count_kernel(const uint8_t* __restrict__ filt, uint32_t* __restrict__ tokens,
                                                          int32_t* __restrict__ n_tokens, uint32_t* __restrict__ hist, png_shape g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char png_lds[];
  uint16_t* table = (uint16_t*)png_lds;                                          // strip offsets of token starts, PNG_EMPTY: none
  uint32_t* count = (uint32_t*)(png_lds + PNG_HASH_SLOTS * 2);
  uint8_t* data = png_lds + PNG_LDS_FIXED;
  const int lane = threadIdx.x;
  for (int64_t s = blockIdx.x; s < g.n_strips; s += gridDim.x) {                 // block-uniform
    const int64_t frame = s / g.per_frame;
    const int k = (int)(s - frame * g.per_frame), row0 = k * g.strip_rows;
    const int P = (int)(min(g.strip_rows, g.H - row0) * g.row);                 // bytes of this strip, 2 .. 65535
    const uint8_t* src = filt + (frame * g.H + row0) * g.row;
    uint32_t* out = tokens + s * g.cap;
    __syncthreads();                                                             // the previous strip's reads are done
    for (int j = lane; j < PNG_HASH_SLOTS / 2; j += 64) ((uint32_t*)table)[j] = 0xFFFFFFFFu;
    for (int j = lane; j < PNG_SYMBOLS; j += 64) count[j] = 0;
    for (int j = lane; j < P; j += 64) data[j] = src[j];
    __syncthreads();
    int pos = 0, nt = 0;                                                         // the same in every lane
    uint32_t mine = 0;                                                           // token nt of the current 64 is kept by lane nt & 63
    while (pos < P) {
      uint32_t tok = data[pos];
      if (pos + 3 <= P) {
        const uint32_t h = (((uint32_t)data[pos] | (uint32_t)data[pos + 1] << 8 | (uint32_t)data[pos + 2] << 16) * 0x9E3779B1u) >> 20;
        const int cand = table[h];
        table[h] = (uint16_t)pos;                                                // one value from all lanes
        if (cand != PNG_EMPTY && pos - cand <= PNG_MAX_DIST) {
          const int maxlen = min(PNG_MAX_MATCH, P - pos);
          int l = 0;
          for (;;) {                                                             // 64 bytes of the prefix per step
            const int i = l + lane;
            const bool same = i < maxlen && data[cand + i] == data[pos + i];
            const unsigned long long differ = ~__ballot(same);
            const int run = differ ? __builtin_ctzll(differ) : 64;
            l += run;
            if (run < 64) break;
          }
          if (l >= 3) tok = (uint32_t)l << 16 | (uint32_t)(pos - cand);
        }
      }
      const uint32_t len = tok >> 16;
      if (lane == 0) {
        if (len == 0) {
          count[tok]++;
        } else {
          int sym, nx; uint32_t x;
          png_length_symbol(len, sym, nx, x);
          count[sym]++;
          png_distance_symbol(tok & 0xFFFFu, sym, nx, x);
          count[PNG_DIST0 + sym]++;
        }
      }
      if (lane == (nt & 63)) mine = tok;
      nt++;
      if ((nt & 63) == 0) out[nt - 64 + lane] = mine;
      pos += len ? (int)len : 1;
    }
    if (lane < (nt & 63)) out[(nt & ~63) + lane] = mine;
    if (lane == 0) {
      n_tokens[s] = nt;
      if (k == g.per_frame - 1) count[PNG_EOB]++;                                // the frame's one end-of-block
    }
    __syncthreads();
    for (int j = lane; j < PNG_SYMBOLS; j += 64)
      if (count[j]) atomicAdd(hist + frame * PNG_SYMBOLS + j, count[j]);
  }
}

extern "C" int emo_png_lz_count(const uint8_t* filtered, uint32_t* tokens, int32_t* n_tokens, uint32_t* hist, int n, int H, int W, int C,
                                int strip_rows, void* stream) {
  EMO_CHECK(filtered && tokens && n_tokens && hist, EMO_ERR_NULL, "emo_png_lz_count: null pointer");
  png_shape g;
  const int rc = png_strip_args("emo_png_lz_count", n, H, W, C, strip_rows, &g);
  if (rc != EMO_OK) return rc;
  EMO_CHECK((uintptr_t)tokens % 4 == 0 && (uintptr_t)hist % 4 == 0, EMO_ERR_BAD_SHAPE, "emo_png_lz_count: tokens and hist must be 4-byte aligned");
  const size_t lds = PNG_LDS_FIXED + (size_t)((g.cap + 15) / 16 * 16);
  if (lds > 64 * 1024) {      // a strip above 54.75 KiB: opt in to the CU's 160 KiB
    static bool once = false;   // idempotent attribute, benign race
    if (!once) {
      const hipError_t e = hipFuncSetAttribute((const void*)png_lz_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               PNG_LDS_FIXED + 65536);
      if (e != hipSuccess) return emo_fail(EMO_ERR_HIP, "emo_png_lz_count: hipFuncSetAttribute: %s", hipGetErrorString(e));
      once = true;
    }
  }
  png_lz_count_kernel<<<(int)(g.n_strips < 16384 ? g.n_strips : 16384), 64, lds, as_stream(stream)>>>(filtered, tokens, n_tokens, hist, g);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ deflate
// a token under the frame's table (per symbol: code length << 16 | the code, bit-reversed) -> the literal / length code with the
// length's extra bits above it (v0, n0 bits) and the distance code with its extra bits (v1, n1 bits; n1 = 0 for a literal)
__device__ __forceinline__ void png_token_code(const uint32_t* tab, uint32_t tok, uint32_t& v0, int& n0, uint32_t& v1, int& n1) {
  const uint32_t len = tok >> 16;
  if (len == 0) {
    const uint32_t e = tab[tok & 255u];
    v0 = e & 0xFFFFu; n0 = (int)(e >> 16) & 15; v1 = 0; n1 = 0;
    return;
  }
  int sym, nx; uint32_t x;
  png_length_symbol(len < 3 ? 3 : len, sym, nx, x);
  uint32_t e = tab[sym];
  int cl = (int)(e >> 16) & 15;
  v0 = (e & 0xFFFFu) | x << cl; n0 = cl + nx;
  png_distance_symbol(tok & 0xFFFFu, sym, nx, x);
  e = tab[PNG_DIST0 + sym];
  cl = (int)(e >> 16) & 15;
  v1 = (e & 0xFFFFu) | x << cl; n1 = cl + nx;
}

__device__ __forceinline__ int png_wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void png_deflate_bits_kernel(const uint32_t* __restrict__ tokens, const int32_t* __restrict__ n_tokens,
                                                               const uint32_t* __restrict__ codes, int32_t* __restrict__ bits, png_shape g) {
  __shared__ uint32_t tab[PNG_SYMBOLS];
  __shared__ int part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t s = blockIdx.x; s < g.n_strips; s += gridDim.x) {                 // block-uniform
    const int64_t frame = s / g.per_frame;
    __syncthreads();                                                             // the previous strip's reads are done
    for (int j = threadIdx.x; j < PNG_SYMBOLS; j += 256) tab[j] = codes[frame * PNG_SYMBOLS + j];
    __syncthreads();
    int nt = n_tokens[s];
    if (nt < 0 || nt > g.cap) nt = 0;                                            // not what emo_png_lz_count leaves: nothing is read past cap
    int sum = 0;
    for (int e = threadIdx.x; e < nt; e += 256) {
      uint32_t v0, v1; int n0, n1;
      png_token_code(tab, tokens[s * g.cap + e], v0, n0, v1, n1);
      sum += n0 + n1;
    }
    sum = png_wave_sum_i32(sum);
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) bits[s] = part[0] + part[1] + part[2] + part[3];
  }
}

static int png_table_args(const char* who, const void* tokens, const void* codes) {
  EMO_CHECK((uintptr_t)tokens % 4 == 0 && (uintptr_t)codes % 4 == 0, EMO_ERR_BAD_SHAPE, "%s: tokens and codes must be 4-byte aligned", who);
  return EMO_OK;
}

extern "C" int emo_png_deflate_bits(const uint32_t* tokens, const int32_t* n_tokens, const uint32_t* codes, int32_t* bits, int n, int H, int W,
                                    int C, int strip_rows, void* stream) {
  EMO_CHECK(tokens && n_tokens && codes && bits, EMO_ERR_NULL, "emo_png_deflate_bits: null pointer");
  png_shape g;
  int rc = png_strip_args("emo_png_deflate_bits", n, H, W, C, strip_rows, &g);
  if (rc == EMO_OK) rc = png_table_args("emo_png_deflate_bits", tokens, codes);
  if (rc != EMO_OK) return rc;
  png_deflate_bits_kernel<<<(int)(g.n_strips < 16384 ? g.n_strips : 16384), 256, 0, as_stream(stream)>>>(tokens, n_tokens, codes, bits, g);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// at most 28 bits, least significant bit first, at bit `pos` of the stream; words at or past n_words are never touched
__device__ __forceinline__ void png_put_bits(uint32_t* __restrict__ words, int64_t n_words, int64_t pos, uint32_t value) {
  const int64_t w = pos >> 5;
  const uint64_t x = (uint64_t)value << (int)(pos & 31);
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (lo && w >= 0 && w < n_words) atomicOr(words + w, lo);
  if (hi && w + 1 >= 0 && w + 1 < n_words) atomicOr(words + w + 1, hi);
}

__global__ __launch_bounds__(256) void png_deflate_emit_kernel(const uint32_t* __restrict__ tokens, const int32_t* __restrict__ n_tokens,
                                                               const uint32_t* __restrict__ codes, const int64_t* __restrict__ bit_offsets,
                                                               uint32_t* __restrict__ words, int64_t n_words, png_shape g) {
  __shared__ uint32_t tab[PNG_SYMBOLS];
  __shared__ int part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t s = blockIdx.x; s < g.n_strips; s += gridDim.x) {                 // block-uniform
    const int64_t frame = s / g.per_frame;
    __syncthreads();
    for (int j = threadIdx.x; j < PNG_SYMBOLS; j += 256) tab[j] = codes[frame * PNG_SYMBOLS + j];
    __syncthreads();
    int nt = n_tokens[s];
    if (nt < 0 || nt > g.cap) nt = 0;
    int64_t base = bit_offsets[s];
    for (int e0 = 0; e0 < nt; e0 += 256) {                                       // block-uniform
      const int e = e0 + (int)threadIdx.x;
      uint32_t v0 = 0, v1 = 0; int n0 = 0, n1 = 0;
      if (e < nt) png_token_code(tab, tokens[s * g.cap + e], v0, n0, v1, n1);
      int end = n0 + n1;                                                         // -> the bits up to and with this token, inside the wavefront
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(end, o, 64);
        if (lane >= o) end += y;
      }
      if (lane == 63) part[wave] = end;
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const int p = part[w];
        if (w < wave) before += p;
        total += p;
      }
      if (e < nt) {
        const int64_t at = base + before + end - n0 - n1;
        png_put_bits(words, n_words, at, v0);
        if (n1) png_put_bits(words, n_words, at + n0, v1);
      }
      base += total;
      __syncthreads();                                                           // the next step writes what was just read
    }
  }
}

extern "C" int emo_png_deflate_emit(const uint32_t* tokens, const int32_t* n_tokens, const uint32_t* codes, const int64_t* bit_offsets,
                                    uint8_t* out, int64_t out_bytes, int n, int H, int W, int C, int strip_rows, void* stream) {
  EMO_CHECK(tokens && n_tokens && codes && bit_offsets && out, EMO_ERR_NULL, "emo_png_deflate_emit: null pointer");
  png_shape g;
  int rc = png_strip_args("emo_png_deflate_emit", n, H, W, C, strip_rows, &g);
  if (rc == EMO_OK) rc = png_table_args("emo_png_deflate_emit", tokens, codes);
  if (rc != EMO_OK) return rc;
  EMO_CHECK(out_bytes > 0 && out_bytes % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)bit_offsets % 8 == 0, EMO_ERR_BAD_SHAPE,
            "emo_png_deflate_emit: the stream buffer is written as 32-bit words: out 4-byte aligned, out_bytes (%lld) a multiple of 4", (long long)out_bytes);
  png_deflate_emit_kernel<<<(int)(g.n_strips < 16384 ? g.n_strips : 16384), 256, 0, as_stream(stream)>>>(tokens, n_tokens, codes, bit_offsets,
                                                                                                       (uint32_t*)out, out_bytes / 4, g);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
