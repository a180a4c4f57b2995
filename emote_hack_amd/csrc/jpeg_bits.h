// jpeg_bits.h - the bit-level half of Huffman decoding (ITU-T T.81 F.2.2) that the baseline kernels (video_in.hip) and the progressive
// one (video_in_progressive.hip) share: a window of the stream staged in LDS, the walking lane's bit reader on it, DECODE behind an
// 8-bit look-up, EXTEND, and the barrier of a wave that synchronises with itself only - and, for the host, which layouts are built.
// Every device function is __forceinline__: a kernel holds the same code as if it were written out there.
#pragma once
#include "common.h"

// blocks per MCU of a layout (components, luminance factors hs x vs; chrominance 1 x 1); 0 for one that is not built
static inline int jpeg_bpm(int ncomp, int hs, int vs) {
  if (ncomp == 1) return (hs == 1 && vs == 1) ? 1 : 0;
  if (ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return hs * vs + 2;
  return 0;
}
#define JPEG_LAYOUTS_BUILT "%s: %d component(s) with luminance at %dx%d: 4:2:0, 4:2:2, 4:4:4 and grey are built"   // who, ncomp, hs, vs

#define JD_TABLE_INTS EMO_JPEG_DECODE_TABLE_INTS  // per table: MINCODE[16] MAXCODE[16] VALPTR[16] 16 unused HUFFVAL[256]
#define JD_STAGE_BYTES 4096                        // the window of the stream held in LDS
#define JD_STAGE_SLACK 16                          // the reader runs at most 8 bytes ahead of the bits it has handed out

// the bit reader of the walking lane: `acc` holds `cnt` unread bits at its top, `rp` is the next dword of the window
struct jd_reader {
  const uint32_t* win;
  uint64_t acc;
  int cnt, rp;
  __device__ __forceinline__ void refill() {      // afterwards cnt >= 32
    if (cnt < 32) {
      const uint32_t w = win[min(rp, (JD_STAGE_BYTES + JD_STAGE_SLACK) / 4 - 1)];
      acc |= (uint64_t)__builtin_bswap32(w) << (32 - cnt);
      cnt += 32;
      rp++;
    }
  }
  __device__ __forceinline__ uint32_t peek(int k) const { return k ? (uint32_t)(acc >> (64 - k)) : 0u; }   // k <= 32
  __device__ __forceinline__ void skip(int k) { acc <<= k; cnt -= k; }
  __device__ __forceinline__ int64_t used() const { return (int64_t)rp * 32 - cnt; }                         // bits since the window's start
  __device__ __forceinline__ int bits(int k) {    // RECEIVE (figure F.17), k <= 16
    refill();
    const int v = (int)peek(k);
    skip(k);
    return v;
  }
  // at bit `bit` of a freshly staged window, whose first byte holds it: bit < 8
  __device__ __forceinline__ void open(const uint32_t* window, int bit) {
    win = window; acc = 0; cnt = 0; rp = 0;
    refill();
    skip(bit);
  }
};

// DECODE of T.81 figure F.16 behind an 8-bit look-up: the symbol, or -1 when no code of the table matches the next 16 bits (with fewer
// than 16 bits left in the frame or segment that is a code cut short, not an undefined one: the caller tells them apart)
__device__ __forceinline__ int jd_symbol(jd_reader& r, const uint16_t* lut, const int32_t* tab) {
  r.refill();
  const uint32_t e = lut[r.peek(8)];
  if (e) {
    r.skip((int)(e >> 8));
    return (int)(e & 255u);
  }
  const uint32_t bits16 = r.peek(16);
  for (int l = 9; l <= 16; l++) {
    const int code = (int)(bits16 >> (16 - l));
    const int maxcode = tab[16 + l - 1];
    if (code <= maxcode) {
      r.skip(l);
      return tab[64 + ((tab[32 + l - 1] + code - tab[l - 1]) & 255)];
    }
  }
  return -1;
}

// RECEIVE + EXTEND (figures F.17, F.12): the s-bit magnitude, s <= 11
__device__ __forceinline__ int jd_extend(jd_reader& r, int s) {
  const int v = r.bits(s);
  return (s && v < (1 << (s - 1))) ? v - (1 << s) + 1 : v;
}

// dword i of a window that starts at byte `first` of the buffer: bytes first + 4 i .. + 3, those at or behind `hi` as 0.  Aligned dword
// loads of the buffer (scan_bytes is a multiple of 4), shifted into place
__device__ __forceinline__ uint32_t jd_stage_dword(const uint8_t* __restrict__ scan, int64_t first, int i, int64_t hi) {
  const int64_t g = first + 4 * (int64_t)i;                    // the first byte wanted
  if (g >= hi) return 0u;
  const int64_t a = g & ~(int64_t)3;
  const int sh = (int)(g & 3) * 8;
  const uint32_t w0 = *(const uint32_t*)(scan + a);            // a < hi <= scan_bytes, a % 4 == 0: inside the buffer
  const uint32_t w1 = (sh && a + 4 < hi) ? *(const uint32_t*)(scan + a + 4) : 0u;
  uint32_t v = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
  const int64_t left = hi - g;                                 // >= 1
  if (left < 4) v &= (1u << (8 * (int)left)) - 1u;
  return v;
}

// What a wave wrote to its part of LDS is read by other lanes of the SAME wave only: a wave's LDS accesses complete in order, so the
// fences stop the compiler from moving them and the barrier is the wave's own.  No workgroup barrier: the waves of a workgroup walk
// segments of different lengths.
__device__ __forceinline__ void jd_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
