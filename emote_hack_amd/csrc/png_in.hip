// png_in.hip - the device half of the PNG / APNG reader (emote_hack_amd/video_io.py is the host half: the chunks and their CRCs, the zlib
// header, the combination of the rows' checksums).  What both entries compute is stated in include/emo_hip.h; how:
//   emo_png_inflate  : ONE wavefront per frame.  The walk is wave-uniform - the bit buffer, the table look-ups and every decision are the
//                      same in all lanes - and the lanes share the work that has a width: a match is copied 64 bytes per step out of the
//                      32 KiB window, a ring in LDS (lane i reads ring[pos - dist + i % dist], so an overlapping match is no special
//                      case), a stored block is a 64-lane copy, and the decoding tables of a block are built by ballots: per code length
//                      the lanes that hold a symbol of it rank themselves, which sorts the symbols canonically and fills a 9-bit
//                      look-up; longer codes walk the counts per length as puff does, from registers.  Produced bytes go to the ring; the ring leaves
//                      for `filtered` 64 bytes at a time, so no byte is read back from global memory; the stream enters through a 1 KiB window
//                      in LDS that the lanes fill one chunk ahead.  37 KiB of LDS: four frames a CU
//   emo_png_unfilter : ONE wavefront per frame, bands of 64 rows one after the other, lane k on row k of the band and, at step t, on
//                      pixel t - k: a (its previous pixel) and c (its previous b) stay in registers, b comes from lane k - 1 by a
//                      lane shift; lane 0 reads the row above from a copy of the previous band's last row in LDS (zeros in a frame's
//                      first band), which lane 63 refreshes 63 steps behind.  The rows pass through an LDS tile of 64 rows x 2 chunks
//                      of 64 pixels, reconstructed in place, so the global loads and stores run along the rows
// Byte work; no MFMA.
#include "jpeg_bits.h"                 // jd_stage_dword: masked dwords of a byte buffer; jd_wave_sync: a wave's own barrier

#define PI_RING 32768                  // RFC 1951: distances reach 32768 bytes back
#define PI_LUT_BITS 9
#define PI_CL_BITS 7                   // the code-length code's codes have at most 7 bits: its look-up is complete
#define PI_DIST0 288                   // lens[0 .. 287]: literal / length, lens[288 .. 319]: distance
#define PI_SYMS 320
#define PI_WINDOW 256                  // dwords of the stream held in LDS: four chunks of 64, of which two or three are live

__constant__ uint8_t pi_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};      // RFC 1951 3.2.7

static int png_in_args(const char* who, int n, int H, int W, int C, int64_t* row) {
  EMO_CHECK(C >= 1 && C <= 4, EMO_ERR_BAD_SHAPE, "%s: C=%d (1: grey, 2: grey + alpha, 3: RGB, 4: RGBA; 8 bits each)", who, C);
  EMO_CHECK(n > 0 && H > 0 && W > 0, EMO_ERR_BAD_SHAPE, "%s: n=%d H=%d W=%d (at least 1 each)", who, n, H, W);
  *row = 1 + (int64_t)W * C;
  EMO_CHECK(*row <= 0x7FFFFFFFLL && (int64_t)H <= 0x7FFFFFFFLL / *row, EMO_ERR_BAD_SHAPE,
            "%s: H=%d rows of %lld filtered bytes; a frame's filtered bytes are counted in 31 bits", who, H, (long long)*row);
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ inflate
// the bit reader, least significant bit first (RFC 1951 3.1.1): `hold` has `have` unread bits from bit 0 up, `next` is the dword behind
// them, read one refill ahead.  The dwords come from a window of the frame in LDS, which the 64 lanes fill 256 bytes at a time with
// vector loads issued one chunk ahead of their use (`pending`): a wave-uniform load would be a scalar one, and the wait for it would
// fall on every LDS access of the walk.  Bytes at or behind the frame's last read as 0; used() tells the caller when it has gone past
struct pi_reader {
  const uint8_t* scan;
  uint32_t* win;                       // PI_WINDOW dwords of LDS: dword w of the frame at w % PI_WINDOW
  int64_t first, hi, wi, filled;       // the frame's bytes first .. hi of scan; wi: dwords taken into hold; chunks below `filled` are in win
  uint64_t hold;
  uint32_t next, pending;              // pending: this lane's dword of chunk `filled`, on its way
  int have, lane;
  __device__ __forceinline__ uint32_t load(int64_t chunk) const { return jd_stage_dword(scan, first + 4 * (chunk * 64 + lane), 0, hi); }
  __device__ __forceinline__ void advance() {                                    // chunk `filled` enters the window, the one behind it sets out
    win[(filled * 64 + lane) & (PI_WINDOW - 1)] = pending;
    filled++;
    pending = load(filled);
    jd_wave_sync();
  }
  __device__ __forceinline__ void open(int64_t byte) {                           // at a byte of the frame
    const int sh = (int)(byte & 3) * 8;
    wi = byte >> 2;
    filled = wi >> 6;
    jd_wave_sync();                                                              // reads of the window before this are done
    pending = load(filled);
    advance();
    hold = (uint64_t)(win[wi & (PI_WINDOW - 1)] >> sh);
    have = 32 - sh;
    wi++;
    if ((wi >> 6) >= filled) advance();
    next = win[wi & (PI_WINDOW - 1)];
  }
  __device__ __forceinline__ void refill() {                                     // afterwards have >= 33
    if (have <= 32) {
      hold |= (uint64_t)next << have;
      have += 32;
      wi++;
      if ((wi >> 6) >= filled) advance();
      next = win[wi & (PI_WINDOW - 1)];
    }
  }
  __device__ __forceinline__ uint32_t peek(int k) const { return (uint32_t)hold & ((1u << k) - 1u); }         // k <= 16
  __device__ __forceinline__ void skip(int k) { hold >>= k; have -= k; }
  __device__ __forceinline__ uint32_t take(int k) { const uint32_t v = peek(k); skip(k); return v; }
  __device__ __forceinline__ int64_t used() const { return wi * 32 - have; }                                   // bits since the frame's first
};

// what the walk of the codes longer than the look-up needs, wave-uniform and in registers: how many symbols have a code of at most
// `bits` bits (they come first in `sorted`), the first code of bits + 1 bits, and the number of codes of every greater length
struct pi_long {
  int index, first, cnt[8];
};

// Code lengths lens[0 .. nsym - 1] (nsym <= 320) -> the symbols sorted by (length, symbol) in `sorted`, the look-up of the next `bits`
// stream bits: symbol << 4 | length, 0 where no code of at most `bits` bits begins, and `lg` for the longer codes.  Per length the
// lanes holding a symbol of it rank themselves by a ballot; the canonical code of a symbol (RFC 1951 3.2.2) is the first code of its
// length plus its rank.  -> what is left of the code space (negative: over-subscribed, positive: incomplete)
__device__ __forceinline__ int pi_build(const uint8_t* lens, int nsym, uint16_t* sorted, uint16_t* lut, int bits, int lane, int& longest,
                                        pi_long& lg) {
  for (int j = lane; j < (1 << bits); j += 64) lut[j] = 0;
  int mine[5];
#pragma unroll
  for (int c = 0; c < 5; c++) mine[c] = c * 64 + lane < nsym ? lens[c * 64 + lane] : 0;
  jd_wave_sync();
  int base = 0, left = 1, code = 0;
  longest = 0;
#pragma unroll
  for (int l = 1; l <= 15; l++) {
    const int start = base;
#pragma unroll
    for (int c = 0; c < 5; c++) {
      if (c * 64 >= nsym) break;                                                 // wave-uniform
      const bool has = mine[c] == l;
      const unsigned long long mask = __ballot(has);
      if (has) {
        const int at = base + __popcll(mask & ((1ull << lane) - 1ull));           // < nsym: every symbol is counted once
        const int sym = c * 64 + lane;
        sorted[at] = (uint16_t)sym;
        if (l <= bits) {
          const uint32_t rev = (__brev((uint32_t)(code + at - start)) >> (32 - l)) & ((1u << l) - 1u);
          for (uint32_t j = rev; j < (1u << bits); j += 1u << l) lut[j] = (uint16_t)(sym << 4 | l);
        }
      }
      base += __popcll(mask);
    }
    const int cnt = base - start;
    if (cnt) longest = l;
    left = left < 0 ? -1 : left * 2 - cnt;
    code = (code + cnt) << 1;
    if (l == bits) { lg.index = base; lg.first = code; }
    if (l > bits) lg.cnt[l - bits - 1] = cnt;
  }
  jd_wave_sync();
  return left;
}

// the next symbol, or -1 when the next 15 bits begin no code; the caller has refilled.  Behind the look-up the count / offset walk of
// a canonical code (as puff walks it), entered at bits + 1 bits: no shorter code begins here, and the walk's state there is lg's
__device__ __forceinline__ int pi_symbol(pi_reader& r, const uint16_t* lut, int bits, const uint16_t* sorted, int nsym, const pi_long& lg) {
  const uint32_t e = lut[r.peek(bits)];
  if (e & 15u) {
    r.skip((int)(e & 15u));
    return (int)(e >> 4);
  }
  uint32_t b = r.peek(15) >> bits;
  int code = (int)(__brev(r.peek(bits)) >> (32 - bits)), first = lg.first, index = lg.index;
#pragma unroll
  for (int k = 0; k < 15 - bits; k++) {
    code = code << 1 | (int)(b & 1u);
    b >>= 1;
    const int cnt = lg.cnt[k];
    if (code - cnt < first) {
      r.skip(bits + 1 + k);
      return sorted[max(0, min(index + (code - first), nsym - 1))];
    }
    index += cnt;
    first = (first + cnt) << 1;
  }
  return -1;
}

struct pi_tables {
  uint16_t lit_lut[1 << PI_LUT_BITS], dist_lut[1 << PI_LUT_BITS], cl_lut[1 << PI_CL_BITS];
  uint16_t lit_sorted[PI_DIST0], dist_sorted[32], cl_sorted[32];
  uint8_t lens[PI_SYMS], cl_lens[32];
};

// both alphabets' tables from lens; zlib's rule: over-subscribed is bad, incomplete is bad unless the set is one code of one bit or
// (distances) empty
__device__ __forceinline__ bool pi_build_both(pi_tables& t, int lane, pi_long& lit, pi_long& dist) {
  int longest;
  int left = pi_build(t.lens, PI_DIST0, t.lit_sorted, t.lit_lut, PI_LUT_BITS, lane, longest, lit);
  if (left < 0 || (left > 0 && longest > 1)) return false;
  left = pi_build(t.lens + PI_DIST0, 32, t.dist_sorted, t.dist_lut, PI_LUT_BITS, lane, longest, dist);
  return !(left < 0 || (left > 0 && longest > 1));
}

// the header of a dynamic block (RFC 1951 3.2.7) -> the status
__device__ __forceinline__ int pi_dynamic(pi_reader& r, int64_t total, pi_tables& t, int lane, pi_long& lit, pi_long& dist) {
  r.refill();
  const int hlit = (int)r.take(5) + 257, hdist = (int)r.take(5) + 1, hclen = (int)r.take(4) + 4;
  if (r.used() > total) return EMO_PNG_PAST_END;
  if (hlit > 286 || hdist > 30) return EMO_PNG_BAD_LENGTHS;
  if (lane < 32) t.cl_lens[lane] = 0;
  for (int j = lane; j < PI_SYMS; j += 64) t.lens[j] = 0;
  jd_wave_sync();
  for (int i = 0; i < hclen; i++) {
    r.refill();
    const uint32_t v = r.take(3);
    if (lane == 0) t.cl_lens[pi_cl_order[i]] = (uint8_t)v;
  }
  if (r.used() > total) return EMO_PNG_PAST_END;
  jd_wave_sync();
  int longest;
  pi_long cl;
  if (pi_build(t.cl_lens, 19, t.cl_sorted, t.cl_lut, PI_CL_BITS, lane, longest, cl) != 0) return EMO_PNG_BAD_LENGTHS;
  const int want = hlit + hdist;
  int n = 0, prev = 0;
  while (n < want) {                                                             // every turn takes at least one bit
    r.refill();
    const int s = pi_symbol(r, t.cl_lut, PI_CL_BITS, t.cl_sorted, 32, cl);
    if (s < 0) return total - r.used() < 15 ? EMO_PNG_PAST_END : EMO_PNG_BAD_LENGTHS;
    int v = 0, rep = 1;
    if (s < 16) { v = s; prev = s; }
    else if (s == 16) {
      if (n == 0) return r.used() > total ? EMO_PNG_PAST_END : EMO_PNG_BAD_LENGTHS;
      v = prev; rep = 3 + (int)r.take(2);
    }
    else if (s == 17) { prev = 0; rep = 3 + (int)r.take(3); }
    else { prev = 0; rep = 11 + (int)r.take(7); }
    if (r.used() > total) return EMO_PNG_PAST_END;
    if (n + rep > want) return EMO_PNG_BAD_LENGTHS;
    for (int k = lane; k < rep; k += 64) {                                       // a run may cross from the literal / length lengths into the distances'
      const int at = n + k;
      t.lens[at < hlit ? at : PI_DIST0 + at - hlit] = (uint8_t)v;
    }
    n += rep;
  }
  jd_wave_sync();
  if (t.lens[256] == 0) return EMO_PNG_BAD_LENGTHS;                              // no end-of-block code
  return pi_build_both(t, lane, lit, dist) ? EMO_PNG_OK : EMO_PNG_BAD_LENGTHS;
}

// ring -> filtered, 64 bytes per step; `all`: the rest too
__device__ __forceinline__ void pi_flush(const uint8_t* ring, uint8_t* __restrict__ out, int64_t& flushed, int64_t pos, int64_t cap, int lane,
                                         bool all) {
  jd_wave_sync();
  while (pos - flushed >= 64 || (all && flushed < pos)) {
    const int64_t i = flushed + lane;
    if (i < pos && i < cap) out[i] = ring[i & (PI_RING - 1)];
    flushed = flushed + 64 < pos ? flushed + 64 : pos;
  }
}

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ scan, int64_t scan_bytes, const int64_t* __restrict__ offsets,
                                                         uint8_t* __restrict__ filtered, int32_t* __restrict__ produced,
                                                         int32_t* __restrict__ status, int n, int64_t cap) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[PI_RING];
  __shared__ pi_tables t;
  __shared__ uint32_t window[PI_WINDOW];
  const int lane = threadIdx.x;
  for (int f = blockIdx.x; f < n; f += gridDim.x) {                              // wave-uniform, as everything below
    int64_t lo = offsets[f], hi = offsets[f + 1];
    if (lo < 0 || hi < lo || hi > scan_bytes) lo = hi = 0;                       // offsets that run backwards or leave the buffer: an empty frame
    const int64_t total = (hi - lo) * 8;
    uint8_t* out = filtered + (int64_t)f * cap;
    pi_reader r;
    r.scan = scan; r.win = window; r.first = lo; r.hi = hi; r.lane = lane;
    r.open(0);
    int64_t pos = 0, flushed = 0;
    int st = EMO_PNG_OK;
    bool fixed_ready = false;
    pi_long lit_long = {}, dist_long = {};
    jd_wave_sync();                                                              // the frame before is done with the LDS
    for (;;) {                                                                   // blocks: every turn takes at least three bits
      r.refill();
      const int last = (int)r.take(1), type = (int)r.take(2);
      if (r.used() > total) { st = EMO_PNG_PAST_END; break; }
      if (type == 3) { st = EMO_PNG_BAD_BLOCK; break; }
      if (type == 0) {                                                           // stored (3.2.4), from the next byte on
        r.skip((int)((-r.used()) & 7));
        r.refill();
        const int64_t len = r.take(16);
        r.refill();
        const int64_t nlen = r.take(16);
        if (r.used() > total) { st = EMO_PNG_PAST_END; break; }
        if ((len ^ nlen) != 0xFFFF) { st = EMO_PNG_BAD_STORED; break; }
        const int64_t from = r.used() >> 3;
        if (from + len > hi - lo) { st = EMO_PNG_PAST_END; break; }
        if (pos + len > cap) { st = EMO_PNG_OVERFLOW; break; }
        pi_flush(ring, out, flushed, pos, cap, lane, true);
        for (int64_t k = lane; k < len; k += 64) {                               // lo + from + k < hi, pos + k < cap
          const uint8_t b = scan[lo + from + k];
          ring[(pos + k) & (PI_RING - 1)] = b;
          out[pos + k] = b;
        }
        pos += len;
        flushed = pos;
        r.open(from + len);
      } else {
        if (type == 1) {                                                         // fixed codes (3.2.6): built once, kept until a dynamic block
          if (!fixed_ready) {
            for (int j = lane; j < PI_SYMS; j += 64) t.lens[j] = j < 144 ? 8 : j < 256 ? 9 : j < 280 ? 7 : j < PI_DIST0 ? 8 : 5;
            jd_wave_sync();
            pi_build_both(t, lane, lit_long, dist_long);
            fixed_ready = true;
          }
        } else {
          fixed_ready = false;
          st = pi_dynamic(r, total, t, lane, lit_long, dist_long);
          if (st != EMO_PNG_OK) break;
        }
        for (;;) {                                                               // symbols: every turn takes at least one bit
          r.refill();
          const int sym = pi_symbol(r, t.lit_lut, PI_LUT_BITS, t.lit_sorted, PI_DIST0, lit_long);
          if (r.used() > total || (sym < 0 && total - r.used() < 15)) { st = EMO_PNG_PAST_END; break; }
          if (sym < 0 || sym > 285) { st = EMO_PNG_BAD_SYMBOL; break; }
          if (sym == 256) break;
          if (sym < 256) {
            if (pos >= cap) { st = EMO_PNG_OVERFLOW; break; }
            if (lane == 0) ring[pos & (PI_RING - 1)] = (uint8_t)sym;
            pos++;
          } else {
            int len;                                                             // 3.2.5
            if (sym < 265) len = sym - 254;
            else if (sym == 285) len = 258;
            else {
              const int nx = (sym - 261) >> 2;
              len = 3 + ((4 + ((sym - 261) & 3)) << nx) + (int)r.take(nx);
            }
            r.refill();
            const int ds = pi_symbol(r, t.dist_lut, PI_LUT_BITS, t.dist_sorted, 32, dist_long);
            if (r.used() > total || (ds < 0 && total - r.used() < 15)) { st = EMO_PNG_PAST_END; break; }
            if (ds < 0 || ds > 29) { st = EMO_PNG_BAD_SYMBOL; break; }
            int dist = ds + 1;
            if (ds >= 4) {
              const int nx = (ds >> 1) - 1;
              dist = 1 + ((2 + (ds & 1)) << nx) + (int)r.take(nx);
            }
            if (r.used() > total) { st = EMO_PNG_PAST_END; break; }
            if (dist > pos) { st = EMO_PNG_BAD_DISTANCE; break; }
            if (pos + len > cap) { st = EMO_PNG_OVERFLOW; break; }
            jd_wave_sync();
            for (int b = 0; b < len; b += 64) {                                  // every source byte lies in front of pos: steps do not feed each other
              const int i = b + lane;
              if (i < len) {
                const int o = dist >= len ? i : i % dist;
                const uint8_t v = ring[(pos - dist + o) & (PI_RING - 1)];
                ring[(pos + i) & (PI_RING - 1)] = v;
              }
            }
            pos += len;
          }
          if (pos - flushed >= 64) pi_flush(ring, out, flushed, pos, cap, lane, false);
        }
        if (st != EMO_PNG_OK) break;
      }
      if (last) break;
    }
    pi_flush(ring, out, flushed, pos, cap, lane, true);
    if (st == EMO_PNG_OK && pos < cap) st = EMO_PNG_SHORT;
    if (lane == 0) {
      produced[f] = (int32_t)pos;
      status[f] = st;
    }
  }
}

extern "C" int emo_png_inflate(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, uint8_t* filtered, int32_t* produced,
                               int32_t* status, int n, int H, int W, int C, void* stream) {
  EMO_CHECK(streams && offsets && filtered && produced && status, EMO_ERR_NULL, "emo_png_inflate: null pointer");
  int64_t row;
  const int rc = png_in_args("emo_png_inflate", n, H, W, C, &row);
  if (rc != EMO_OK) return rc;
  EMO_CHECK(stream_bytes > 0 && stream_bytes % 4 == 0 && (uintptr_t)streams % 4 == 0, EMO_ERR_BAD_SHAPE,
            "emo_png_inflate: the streams are read as 32-bit words: 4-byte aligned, stream_bytes (%lld) a positive multiple of 4", (long long)stream_bytes);
  EMO_CHECK((uintptr_t)offsets % 8 == 0 && (uintptr_t)produced % 4 == 0 && (uintptr_t)status % 4 == 0, EMO_ERR_BAD_SHAPE,
            "emo_png_inflate: offsets must be 8-byte aligned, produced and status 4-byte aligned");
  png_inflate_kernel<<<n < 16384 ? n : 16384, 64, 0, as_stream(stream)>>>(streams, stream_bytes, offsets, filtered, produced, status, n,
                                                                           (int64_t)H * row);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ unfilter
#define PU_CHUNK 64                    // pixels of a chunk; the tile holds two
#define PU_MAX_ROW 98304               // bytes of a raw row the copy of the row above may take in LDS
#define PU_ADLER 65521u

__device__ __forceinline__ int pu_paeth(int a, int b, int c) {                   // PNG 9.4: a on ties, then b
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

static inline int pu_tile_stride(int C) { return 2 * PU_CHUNK * C + C + 4; }     // lane k at pixel t - k lands 4 k bytes on: one bank per lane

template <int C>
__global__ __launch_bounds__(64) void png_unfilter_kernel(const uint8_t* __restrict__ filt, uint8_t* __restrict__ frames, uint32_t* __restrict__ adler,
                                                          int32_t* __restrict__ status, int n, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pu_lds[];
  constexpr int stride = 2 * PU_CHUNK * C + C + 4;
  uint8_t* tile = pu_lds;                                                        // [64][stride]: row k, pixel p at (p & 127) * C
  uint8_t* above = pu_lds + 64 * stride;                                         // [W * C]: the raw row above the band
  const int lane = threadIdx.x;
  const int64_t L = (int64_t)W * C, R = L + 1;
  const int chunks = (W + PU_CHUNK - 1) / PU_CHUNK, phases = (W + 63 + PU_CHUNK - 1) / PU_CHUNK;
  for (int f = blockIdx.x; f < n; f += gridDim.x) {                              // wave-uniform
    const uint8_t* src = filt + (int64_t)f * H * R;
    uint8_t* dst = frames + (int64_t)f * H * L;
    jd_wave_sync();
    for (int64_t j = lane; j < L; j += 64) above[j] = 0;                         // PNG 9.2: the row above the first is zeros
    int st = EMO_PNG_OK;
    for (int row0 = 0; row0 < H; row0 += 64) {
      const int rows = min(64, H - row0);
      const bool active = lane < rows;
      const int type = active ? src[(int64_t)(row0 + lane) * R] : 0;
      if (__ballot(active && type > 4)) { st = EMO_PNG_BAD_FILTER; break; }
      uint32_t s1 = 1 + type, s2 = s1;                                           // Adler-32 of the row's filtered bytes from (1, 0)
      int a[C], cc[C], mine[C];                                                  // the lane's previous pixel, its previous b, what it last produced
#pragma unroll
      for (int c = 0; c < C; c++) a[c] = cc[c] = mine[c] = 0;
      for (int q = 0; q <= chunks + 1; q++) {
        jd_wave_sync();
        if (q >= 2 && q - 2 < chunks) {                                          // chunk q - 2 is whole: every lane is past it
          const int px0 = (q - 2) * PU_CHUNK, nb = min(PU_CHUNK, W - px0) * C, slot = (q & 1) * PU_CHUNK * C;
          for (int r = 0; r < rows; r++)
            for (int j = lane; j < nb; j += 64) dst[(int64_t)(row0 + r) * L + (int64_t)px0 * C + j] = tile[r * stride + slot + j];
        }
        if (q < chunks) {                                                        // chunk q takes the place of chunk q - 2
          const int px0 = q * PU_CHUNK, nb = min(PU_CHUNK, W - px0) * C, slot = (q & 1) * PU_CHUNK * C;
          for (int r = 0; r < rows; r++)
            for (int j = lane; j < nb; j += 64) tile[r * stride + slot + j] = src[(int64_t)(row0 + r) * R + 1 + (int64_t)px0 * C + j];
        }
        jd_wave_sync();
        if (q >= phases) continue;
        for (int s = 0; s < PU_CHUNK; s++) {
          const int p = q * PU_CHUNK + s - lane;                                 // the lane's pixel at this step
          const bool work = active && p >= 0 && p < W;
          int up[C];
#pragma unroll
          for (int c = 0; c < C; c++) up[c] = __shfl_up(mine[c], 1, 64);         // lane k - 1 made pixel p one step ago
          if (work) {
            uint8_t* at = tile + lane * stride + (p & (2 * PU_CHUNK - 1)) * C;
#pragma unroll
            for (int c = 0; c < C; c++) {
              const int x = at[c];
              const int b = lane == 0 ? above[(int64_t)p * C + c] : up[c];
              const int pa = p > 0 ? a[c] : 0, pc = p > 0 ? cc[c] : 0;
              const int pred = type == 0 ? 0 : type == 1 ? pa : type == 2 ? b : type == 3 ? ((pa + b) >> 1) : pu_paeth(pa, b, pc);
              const int v = (x + pred) & 255;
              at[c] = (uint8_t)v;
              if (lane == 63) above[(int64_t)p * C + c] = (uint8_t)v;           // lane 0 of the next band reads it; lane 0 of this one is 63 pixels on
              s1 += (uint32_t)x; if (s1 >= PU_ADLER) s1 -= PU_ADLER;
              s2 += s1; if (s2 >= PU_ADLER) s2 -= PU_ADLER;
              a[c] = v; cc[c] = b; mine[c] = v;
            }
          }
        }
      }
      if (active) {
        adler[2 * ((int64_t)f * H + row0 + lane)] = s1;
        adler[2 * ((int64_t)f * H + row0 + lane) + 1] = s2;
      }
    }
    if (lane == 0) status[f] = st;
  }
}

extern "C" int emo_png_unfilter(const uint8_t* filtered, uint8_t* frames, uint32_t* adler, int32_t* status, int n, int H, int W, int C,
                                void* stream) {
  EMO_CHECK(filtered && frames && adler && status, EMO_ERR_NULL, "emo_png_unfilter: null pointer");
  int64_t row;
  const int rc = png_in_args("emo_png_unfilter", n, H, W, C, &row);
  if (rc != EMO_OK) return rc;
  EMO_CHECK(row - 1 <= PU_MAX_ROW, EMO_ERR_BAD_SHAPE, "emo_png_unfilter: a row of %d pixels of %d bytes; at most %d bytes per row (the row above a band "
            "of 64 is kept in LDS)", W, C, PU_MAX_ROW);
  EMO_CHECK((uintptr_t)adler % 4 == 0 && (uintptr_t)status % 4 == 0, EMO_ERR_BAD_SHAPE, "emo_png_unfilter: adler and status must be 4-byte aligned");
  const size_t lds = (size_t)64 * pu_tile_stride(C) + (size_t)((row - 1 + 15) / 16 * 16);
  const void* kernel = C == 1 ? (const void*)png_unfilter_kernel<1> : C == 2 ? (const void*)png_unfilter_kernel<2>
                     : C == 3 ? (const void*)png_unfilter_kernel<3> : (const void*)png_unfilter_kernel<4>;
  if (lds > 64 * 1024) {        // a row above 31 KiB: opt in to the CU's 160 KiB (idempotent attribute, benign race)
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * pu_tile_stride(4) + PU_MAX_ROW);
    if (e != hipSuccess) return emo_fail(EMO_ERR_HIP, "emo_png_unfilter: hipFuncSetAttribute: %s", hipGetErrorString(e));
  }
  const int grid = n < 16384 ? n : 16384;
  hipStream_t s = as_stream(stream);
  if (C == 1) png_unfilter_kernel<1><<<grid, 64, lds, s>>>(filtered, frames, adler, status, n, H, W);
  else if (C == 2) png_unfilter_kernel<2><<<grid, 64, lds, s>>>(filtered, frames, adler, status, n, H, W);
  else if (C == 3) png_unfilter_kernel<3><<<grid, 64, lds, s>>>(filtered, frames, adler, status, n, H, W);
  else png_unfilter_kernel<4><<<grid, 64, lds, s>>>(filtered, frames, adler, status, n, H, W);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
