// gif_out.hip - the device half of the GIF89a writer, the other container `save_videos_grid`'s imageio.mimsave is used for
// (magicanimate/utils/util.py:21-33; emote_hack_amd/video_io.py is the host half: median cut, the container, the 255-byte sub-blocks):
//   emo_gif_histogram  : per table 32768 bins (r >> 3, g >> 3, b >> 3) x {count, sum R, sum G, sum B}, 64-bit integer atomics only.  A
//                        lane folds runs of equal bins in its 8 consecutive pixels before it adds, and a wavefront whose 512 pixels end
//                        in ONE bin (a flat background) adds once: four atomics per 512 pixels instead of 2048
//   emo_gif_map        : the nearest of the first n_colors palette entries per pixel (squared Euclidean distance on the 8-bit integers,
//                        the lowest index on a tie; exact search), the palette staged in LDS and read by broadcast; optionally an 8x8
//                        ordered (Bayer) dither in front of the search
//   emo_gif_lzw_count  : variable-width LZW (GIF89a Appendix F) of every strip of rows, each from an empty dictionary: ONE wavefront per
//                        strip, the dictionary an open-addressed table of up to 8192 words in LDS (32 KiB: five strips per CU), lane 0
//                        walks, all 64 lanes stage the pixels and clear the table (sized to the strip, so a reset costs less than the
//                        walk).  The codes are left in a scratch buffer: the walk happens once
//   emo_gif_lzw_emit   : one lane per code.  A code's width and its bit position inside its strip follow from its INDEX alone (the
//                        decoder's table grows by one entry per code), so the second pass is a gather with a closed-form offset,
//                        OR-ed least-significant-bit first into the zeroed stream (32-bit atomicOr: strips and frames share words)
// Byte work and one serial walk per strip; no MFMA.
#include "common.h"

#define GIF_BINS 32768
#define GIF_CLEAR 256
#define GIF_EOI 257
#define GIF_FIRST_FREE 258
// a segment = what lies between two Clear codes: code j of it (j = 0 the first) is read by a decoder that has added max(0, j - 1)
// entries, so its next free code is 258 (j = 0) or 257 + j, and the width is 9 up to 511, 10 up to 1023, 11 up to 2047, else 12.
// The encoder adds entry 258 + j behind code j while that is below 4096: j = 0 .. 3837.  Code 3838 finds the table full; a Clear goes
// behind it as entry 3839 (12 bits) and the next segment starts.  So every full segment is 3840 entries of GIF_SEG_BITS bits.
#define GIF_SEG_DATA 3839
#define GIF_SEG_ENTRIES 3840
#define GIF_SEG_BITS 43267          // gif_bits_in_segment(3840)
#define GIF_TABLE_SLOTS 8192
#define GIF_EMPTY 0xFFFFFFFFu       // key << 12 | code is never this: the key of prefix 4095 never gets an entry (the table is full by then)
#define GIF_CHUNK 1024
#define GIF_MAX_STRIP_PIXELS (1 << 26)

__host__ __device__ __forceinline__ int gif_width_at(int j) { return 9 + (j >= 255) + (j >= 767) + (j >= 1791); }
__host__ __device__ __forceinline__ int gif_bits_in_segment(int j) {       // bits of codes 0 .. j - 1 of a segment
  return 9 * j + (j > 255 ? j - 255 : 0) + (j > 767 ? j - 767 : 0) + (j > 1791 ? j - 1791 : 0);
}
__host__ __device__ __forceinline__ int64_t gif_bits_before(int e) {       // bits of entries 0 .. e - 1 of a strip (mid-strip Clears count)
  return (int64_t)(e / GIF_SEG_ENTRIES) * GIF_SEG_BITS + gif_bits_in_segment(e % GIF_SEG_ENTRIES);
}
static inline int64_t gif_codes_per_strip(int64_t strip_pixels) { return strip_pixels + strip_pixels / GIF_SEG_DATA + 2; }

// ------------------------------------------------------------------------------------------------------------------------ histogram
// A workgroup owns a span of consecutive pixels; one wavefront takes 512 of them at a time, lane l the pixels 8 l .. 8 l + 7.  What the
// span adds to a bin is collected in LDS first: 2048 slots, each claimed by the first (table, bin) that hashes to it (atomicCAS on its
// tag); a (table, bin) that finds its slot taken by another goes to global memory at once.  At the span's end every claimed slot is
// added to global memory once.  Integer adds commute, so which pixels went through LDS does not show in the result.
#define GIF_HIST_SLOTS 2048
#define GIF_HIST_SPAN_MAX (1 << 22)      // pixels per span: the 32-bit sums in LDS hold 255 * 2^22
#define GIF_HIST_REL_MAX 0xFFFF          // a tag is (table - the span's first table) << 15 | bin; tables further on bypass LDS

__device__ __forceinline__ void gif_hist_add(unsigned long long* __restrict__ hist, int64_t key, uint32_t c, uint32_t r, uint32_t g, uint32_t b) {
  unsigned long long* p = hist + key * 4;      // key = table * 32768 + bin
  atomicAdd(p, (unsigned long long)c);
  atomicAdd(p + 1, (unsigned long long)r);
  atomicAdd(p + 2, (unsigned long long)g);
  atomicAdd(p + 3, (unsigned long long)b);
}

__device__ __forceinline__ void gif_hist_collect(uint32_t* tags, uint32_t (*acc)[4], unsigned long long* __restrict__ hist, int64_t table0,
                                                 int64_t key, uint32_t c, uint32_t r, uint32_t g, uint32_t b) {
  const int64_t rel = key / GIF_BINS - table0;
  if (rel < GIF_HIST_REL_MAX) {
    const uint32_t tag = ((uint32_t)rel << 15) | (uint32_t)(key % GIF_BINS);    // never 0xFFFFFFFF
    const uint32_t slot = (tag * 0x9E3779B1u) >> 21;
    const uint32_t old = atomicCAS(tags + slot, 0xFFFFFFFFu, tag);
    if (old == 0xFFFFFFFFu || old == tag) {
      atomicAdd(&acc[slot][0], c); atomicAdd(&acc[slot][1], r); atomicAdd(&acc[slot][2], g); atomicAdd(&acc[slot][3], b);
      return;
    }
  }
  gif_hist_add(hist, key, c, r, g, b);
}

__device__ __forceinline__ uint32_t gif_wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void gif_histogram_kernel(const uint8_t* __restrict__ frames, unsigned long long* __restrict__ hist,
                                                            int64_t px_per_frame, int64_t total_px, int per_frame, int64_t span) {
  __shared__ uint32_t tags[GIF_HIST_SLOTS];
  __shared__ uint32_t acc[GIF_HIST_SLOTS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t start = (int64_t)blockIdx.x * span; start < total_px; start += (int64_t)gridDim.x * span) {                  // block-uniform
    const int64_t end = start + span < total_px ? start + span : total_px;
    const int64_t table0 = per_frame ? start / px_per_frame : 0;
    for (int j = threadIdx.x; j < GIF_HIST_SLOTS; j += 256) {
      tags[j] = 0xFFFFFFFFu;
      acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0;
    }
    __syncthreads();
    for (int64_t chunk = start + wave * 512; chunk < end; chunk += 2048) {                                                    // wave-uniform
      const int64_t p0 = chunk + lane * 8;
      int64_t frame = per_frame ? p0 / px_per_frame : 0;
      int64_t boundary = per_frame ? (frame + 1) * px_per_frame : total_px;     // the first pixel of the next table
      int64_t cur = -1;
      uint32_t c = 0, r = 0, g = 0, b = 0;
      for (int i = 0; i < 8; i++) {                                              // runs of one bin inside the lane's pixels are folded
        const int64_t p = p0 + i;
        if (p >= end) break;
        if (p >= boundary) { frame++; boundary += px_per_frame; }
        const uint8_t* px = frames + p * 3;
        const uint32_t pr = px[0], pg = px[1], pb = px[2];
        const int64_t key = frame * GIF_BINS + (int64_t)(((pr >> 3) << 10) | ((pg >> 3) << 5) | (pb >> 3));
        if (key != cur) {
          if (c) gif_hist_collect(tags, acc, hist, table0, cur, c, r, g, b);
          cur = key; c = r = g = b = 0;
        }
        c++; r += pr; g += pg; b += pb;
      }
      // what every lane still holds: its last run.  Lane 0 always holds one (chunk < end).  A wavefront whose lanes all end in ONE
      // bin - a flat background - adds once
      const int64_t k0 = __shfl(cur, 0, 64);
      if (__all(c == 0 || cur == k0)) {
        c = gif_wave_sum_u32(c); r = gif_wave_sum_u32(r); g = gif_wave_sum_u32(g); b = gif_wave_sum_u32(b);    // <= 512 * 255 each
        if (lane == 0) gif_hist_collect(tags, acc, hist, table0, k0, c, r, g, b);
      } else if (c) {
        gif_hist_collect(tags, acc, hist, table0, cur, c, r, g, b);
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < GIF_HIST_SLOTS; j += 256) {
      const uint32_t tag = tags[j];
      if (tag != 0xFFFFFFFFu) gif_hist_add(hist, (table0 + (tag >> 15)) * GIF_BINS + (tag & 32767u), acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    }
    __syncthreads();                                                             // the next span clears what was just read
  }
}

extern "C" int emo_gif_histogram(const uint8_t* frames, uint64_t* hist, int n, int H, int W, int per_frame, void* stream) {
  EMO_CHECK(frames && hist, EMO_ERR_NULL, "emo_gif_histogram: null pointer");
  EMO_CHECK(n > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535, EMO_ERR_BAD_SHAPE,
            "emo_gif_histogram: n=%d H=%d W=%d (1 .. 65535: the logical screen descriptor holds 16 bits)", n, H, W);
  const int64_t px = (int64_t)H * W, total = px * n;
  EMO_CHECK(total <= (int64_t)1 << 55, EMO_ERR_BAD_SHAPE, "emo_gif_histogram: %lld pixels; the 64-bit sums are exact up to 2^55 pixels of 255",
            (long long)total);
  EMO_CHECK((uintptr_t)hist % 8 == 0, EMO_ERR_BAD_SHAPE, "emo_gif_histogram: hist must be 8-byte aligned");
  // four workgroups of 40 KiB of LDS per CU, 256 CUs: up to 1024 spans at once, each a whole number of 2048-pixel rounds
  int64_t span = ((total + 1023) / 1024 + 2047) / 2048 * 2048;
  if (span > GIF_HIST_SPAN_MAX) span = GIF_HIST_SPAN_MAX;
  const int64_t g = (total + span - 1) / span;
  gif_histogram_kernel<<<(int)(g < 4096 ? g : 4096), 256, 0, as_stream(stream)>>>(frames, (unsigned long long*)hist, px, total, per_frame != 0, span);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ palette mapping
// B8[y][x] of the recursion B1 = [[0]], B2k = [[4B, 4B + 2], [4B + 3, 4B + 1]]: the quadrant a bit pair picks at each level adds
// q = (3 * ybit) ^ (2 * xbit) = 0, 2, 3, 1, times 16 at the finest level (bit 0), 4 at the next, 1 at the coarsest (bit 2)
__device__ __forceinline__ int gif_bayer8(int y, int x) {
  const int q0 = (3 * (y & 1)) ^ (2 * (x & 1)), q1 = (3 * ((y >> 1) & 1)) ^ (2 * ((x >> 1) & 1)), q2 = (3 * ((y >> 2) & 1)) ^ (2 * ((x >> 2) & 1));
  return 16 * q0 + 4 * q1 + q2;
}

__global__ __launch_bounds__(256) void gif_map_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ palettes,
                                                      uint8_t* __restrict__ indices, int n, int64_t px_per_frame, int W, int n_colors,
                                                      int per_frame, int strength) {
  __shared__ uint32_t pal[256];       // r | g << 8 | b << 16
  for (int f = blockIdx.y; f < n; f += gridDim.y) {                              // block-uniform
    if (f == (int)blockIdx.y || per_frame) {
      __syncthreads();                                                           // the previous frame's reads are done
      const uint8_t* src = palettes + (per_frame ? (int64_t)f * 768 : 0);
      if ((int)threadIdx.x < n_colors) pal[threadIdx.x] = src[threadIdx.x * 3] | (src[threadIdx.x * 3 + 1] << 8) | (src[threadIdx.x * 3 + 2] << 16);
      __syncthreads();
    }
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < px_per_frame; p += (int64_t)gridDim.x * 256) {
      const uint8_t* px = frames + ((int64_t)f * px_per_frame + p) * 3;
      int r = px[0], g = px[1], b = px[2];
      if (strength) {
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        const int d = ((2 * gif_bayer8(y & 7, x & 7) - 63) * strength) >> 7;    // an arithmetic shift: floor
        r = min(max(r + d, 0), 255); g = min(max(g + d, 0), 255); b = min(max(b + d, 0), 255);
      }
      int best = 0x7FFFFFFF, bi = 0;
      for (int k = 0; k < n_colors; k++) {
        const uint32_t e = pal[k];                                               // one address for the whole wavefront: a broadcast
        const int dr = r - (int)(e & 255), dg = g - (int)((e >> 8) & 255), db = b - (int)(e >> 16);
        const int d = dr * dr + dg * dg + db * db;
        if (d < best) { best = d; bi = k; }                                      // strictly below: the lowest index keeps a tie
      }
      indices[(int64_t)f * px_per_frame + p] = (uint8_t)bi;
    }
  }
}

extern "C" int emo_gif_map(const uint8_t* frames, const uint8_t* palettes, uint8_t* indices, int n, int H, int W, int n_colors,
                           int per_frame, int dither_strength, void* stream) {
  EMO_CHECK(frames && palettes && indices, EMO_ERR_NULL, "emo_gif_map: null pointer");
  EMO_CHECK(n > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535, EMO_ERR_BAD_SHAPE, "emo_gif_map: n=%d H=%d W=%d (1 .. 65535)", n, H, W);
  EMO_CHECK(n_colors >= 1 && n_colors <= 256, EMO_ERR_BAD_SHAPE, "emo_gif_map: n_colors=%d (1 .. 256)", n_colors);
  EMO_CHECK(dither_strength >= 0 && dither_strength <= 128, EMO_ERR_BAD_SHAPE, "emo_gif_map: dither_strength=%d (0: none, 1 .. 128)", dither_strength);
  const int64_t px = (int64_t)H * W, g = (px + 255) / 256;
  dim3 grid((unsigned)(g < 1024 ? g : 1024), (unsigned)(n < 1024 ? n : 1024));
  gif_map_kernel<<<grid, 256, 0, as_stream(stream)>>>(frames, palettes, indices, n, px, W, n_colors, per_frame != 0, dither_strength);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ LZW
struct gif_strips {
  int H, W, strip_rows, per_frame;   // per_frame: strips of a frame, the last may be short
  int64_t n_strips, cap;             // cap: entries of the scratch buffer per strip
};

static int gif_strip_args(const char* who, int n, int H, int W, int strip_rows, gif_strips* s) {
  EMO_CHECK(n > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535, EMO_ERR_BAD_SHAPE, "%s: n=%d H=%d W=%d (1 .. 65535)", who, n, H, W);
  EMO_CHECK(strip_rows >= 1, EMO_ERR_BAD_SHAPE, "%s: strip_rows=%d", who, strip_rows);
  if (strip_rows > H) strip_rows = H;
  EMO_CHECK((int64_t)strip_rows * W <= GIF_MAX_STRIP_PIXELS, EMO_ERR_BAD_SHAPE, "%s: a strip of %d rows of %d pixels; at most 2^26 pixels per strip "
            "(its bits are counted in 32)", who, strip_rows, W);
  s->H = H; s->W = W; s->strip_rows = strip_rows;
  s->per_frame = (H + strip_rows - 1) / strip_rows;
  s->n_strips = (int64_t)s->per_frame * n;
  s->cap = gif_codes_per_strip((int64_t)strip_rows * W);
  return EMO_OK;
}

extern "C" int64_t emo_gif_lzw_codes_per_strip(int H, int W, int strip_rows) {
  if (H < 1 || W < 1 || strip_rows < 1) return 0;
  return gif_codes_per_strip((int64_t)(strip_rows < H ? strip_rows : H) * W);
}

// one wavefront per strip
__global__ __launch_bounds__(64) void gif_lzw_count_kernel(const uint8_t* __restrict__ indices, uint16_t* __restrict__ codes,
                                                           int32_t* __restrict__ n_codes, int32_t* __restrict__ bits, gif_strips g) {
  __shared__ uint32_t table[GIF_TABLE_SLOTS];       // key << 12 | code, key = prefix << 8 | byte
  __shared__ uint8_t chunk[GIF_CHUNK];
  const int lane = threadIdx.x;
  for (int64_t s = blockIdx.x; s < g.n_strips; s += gridDim.x) {                 // block-uniform
    const int64_t frame = s / g.per_frame;
    const int k = (int)(s - frame * g.per_frame), row0 = k * g.strip_rows;
    const int P = min(g.strip_rows, g.H - row0) * g.W;                          // pixels of this strip, >= 1
    const uint8_t* src = indices + (frame * g.H + row0) * (int64_t)g.W;
    uint16_t* out = codes + s * g.cap;
    int lg = 6;                                                                  // slots >= 2 * the entries the strip can make
    while (lg < 13 && (1 << lg) < 2 * min(P, GIF_SEG_DATA)) lg++;
    const int slots = 1 << lg;
    int w = -1, seg = 0, e = 0;                                                  // lane 0's: the open string, codes of this segment, entries
    int pos = 0, full = 0;
    bool clear = true;
    while (pos < P) {                                                            // wave-uniform: pos and clear come from lane 0
      __syncthreads();
      if (clear)
        for (int j = lane; j < slots; j += 64) table[j] = GIF_EMPTY;
      const int m = min(GIF_CHUNK, P - pos);
      for (int j = lane; j < m; j += 64) chunk[j] = src[pos + j];
      __syncthreads();
      int i = 0;
      full = 0;
      if (lane == 0) {
        if (clear && e > 0) { out[e++] = GIF_CLEAR; seg = 0; }                    // the table was full: entry 3839 of the segment
        for (; i < m; i++) {
          const int c = chunk[i];
          if (w < 0) { w = c; continue; }
          const uint32_t key = ((uint32_t)w << 8) | (uint32_t)c;
          uint32_t h = (key * 0x9E3779B1u) >> (32 - lg), v;
          for (;;) {                                                             // ends: the table is never more than half full
            v = table[h];
            if (v == GIF_EMPTY || (v >> 12) == key) break;
            h = (h + 1) & (uint32_t)(slots - 1);
          }
          if (v != GIF_EMPTY) { w = (int)(v & 0xFFFu); continue; }
          out[e++] = (uint16_t)w;                                                // code `seg` of the segment
          w = c;
          if (seg < GIF_SEG_DATA - 1) {
            table[h] = (key << 12) | (uint32_t)(GIF_FIRST_FREE + seg);
            seg++;
          } else {                                                               // code 3838: no entry is left for it
            seg++;
            full = 1;
            i++;
            break;
          }
        }
      }
      pos += __shfl(i, 0, 64);
      clear = __shfl(full, 0, 64) != 0;
    }
    if (lane == 0) {
      if (clear && e > 0) out[e++] = GIF_CLEAR;                                  // the table filled at the strip's last pixel: the open
      //                                                                            string still follows, and no code may be entry 3839
      out[e++] = (uint16_t)w;                                                    // the open string: P >= 1, so there is one
      n_codes[s] = e;
      bits[s] = (k == 0 ? 9 : 0) + (int32_t)gif_bits_before(e) + gif_width_at(e % GIF_SEG_ENTRIES);      // [Clear] codes Clear | EOI
    }
  }
}

extern "C" int emo_gif_lzw_count(const uint8_t* indices, uint16_t* codes, int32_t* n_codes, int32_t* bits, int n, int H, int W,
                                 int strip_rows, void* stream) {
  EMO_CHECK(indices && codes && n_codes && bits, EMO_ERR_NULL, "emo_gif_lzw_count: null pointer");
  gif_strips g;
  const int rc = gif_strip_args("emo_gif_lzw_count", n, H, W, strip_rows, &g);
  if (rc != EMO_OK) return rc;
  EMO_CHECK((uintptr_t)codes % 2 == 0, EMO_ERR_BAD_SHAPE, "emo_gif_lzw_count: codes must be 2-byte aligned");
  gif_lzw_count_kernel<<<(int)(g.n_strips < 8192 ? g.n_strips : 8192), 64, 0, as_stream(stream)>>>(indices, codes, n_codes, bits, g);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// `nbits` (9 .. 12) bits of `code`, least significant bit first, at bit `pos` of the stream; words at or past n_words are never touched
__device__ __forceinline__ void gif_put_bits(uint32_t* __restrict__ words, int64_t n_words, int64_t pos, uint32_t code) {
  const int64_t w = pos >> 5;
  const uint64_t x = (uint64_t)code << (int)(pos & 31);
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (lo && w >= 0 && w < n_words) atomicOr(words + w, lo);
  if (hi && w + 1 >= 0 && w + 1 < n_words) atomicOr(words + w + 1, hi);
}

__global__ __launch_bounds__(256) void gif_lzw_emit_kernel(const uint16_t* __restrict__ codes, const int32_t* __restrict__ n_codes,
                                                           const int64_t* __restrict__ bit_offsets, uint32_t* __restrict__ words,
                                                           int64_t n_words, gif_strips g) {
  for (int64_t s = blockIdx.y; s < g.n_strips; s += gridDim.y) {
    const int k = (int)(s % g.per_frame), ne = n_codes[s];
    if (ne < 1 || ne > g.cap - 1) continue;                                      // not what emo_gif_lzw_count leaves: nothing is read past cap
    int64_t base = bit_offsets[s];
    if (k == 0) {
      if (blockIdx.x == 0 && threadIdx.x == 0) gif_put_bits(words, n_words, base, GIF_CLEAR);
      base += 9;
    }
    const uint32_t last = k == g.per_frame - 1 ? GIF_EOI : GIF_CLEAR;
    for (int e = blockIdx.x * 256 + threadIdx.x; e <= ne; e += gridDim.x * 256)
      gif_put_bits(words, n_words, base + gif_bits_before(e), e < ne ? (uint32_t)codes[s * g.cap + e] : last);
  }
}

extern "C" int emo_gif_lzw_emit(const uint16_t* codes, const int32_t* n_codes, const int64_t* bit_offsets, uint8_t* out, int64_t out_bytes,
                                int n, int H, int W, int strip_rows, void* stream) {
  EMO_CHECK(codes && n_codes && bit_offsets && out, EMO_ERR_NULL, "emo_gif_lzw_emit: null pointer");
  gif_strips g;
  const int rc = gif_strip_args("emo_gif_lzw_emit", n, H, W, strip_rows, &g);
  if (rc != EMO_OK) return rc;
  EMO_CHECK(out_bytes > 0 && out_bytes % 4 == 0 && (uintptr_t)out % 4 == 0, EMO_ERR_BAD_SHAPE,
            "emo_gif_lzw_emit: the stream buffer is written as 32-bit words: out 4-byte aligned, out_bytes (%lld) a multiple of 4", (long long)out_bytes);
  const int64_t gx = (g.cap + 255) / 256;
  dim3 grid((unsigned)(gx < 64 ? gx : 64), (unsigned)(g.n_strips < 16384 ? g.n_strips : 16384));
  gif_lzw_emit_kernel<<<grid, 256, 0, as_stream(stream)>>>(codes, n_codes, bit_offsets, (uint32_t*)out, out_bytes / 4, g);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
