// gif_in.hip - the device half of the GIF reader (emote_hack_amd/video_io.py is the host half: the blocks of the container, the colour
// tables, the graphic control extensions, the sticky disposal).  What both entries compute is stated in include/emo_hip.h; how:
//   emo_gif_lzw_decode : ONE wavefront per frame.  The walk is wave-uniform - the bit buffer, the code, the table look-up and every
//                        decision are the same in all lanes.  A dictionary entry is never a chain of prefixes here: the entry a
//                        decoder adds is "the previous string plus the first byte of the current one", and those are len(prev) + 1
//                        CONSECUTIVE bytes of the frame's own output, beginning where the previous string was emitted.  So an entry
//                        is (start in the frame's output, length), 4096 x 6 bytes of LDS, set BEFORE the current code is looked up:
//                        the KwKwK code (the code equal to the next free one) then finds its own entry, whose source overlaps its
//                        destination by len(prev) bytes, and lane i reads source byte i % len(prev) - every source byte lies in
//                        front of the write position, so the 64-byte steps of one string never feed each other.  The source is
//                        the frame's earlier output in GLOBAL memory (LZW has no window: an entry may point at the frame's first
//                        byte), written by other lanes of this wave: a workgroup-scope release / acquire pair stands between a
//                        string's loads and the stores they may depend on - only when the source reaches behind `fenced`, the
//                        position up to which the stores are known to have landed.  Literals (codes below Clear) read nothing.
//                        The stream is held in two registers per lane (two chunks of 64 dwords, the second loaded one chunk
//                        ahead) and enters the wave-uniform bit buffer by a lane read: no LDS, no scalar load in the walk
//   emo_gif_compose    : one thread per 4 neighbouring pixels of the canvas (row-major), looping over the frames in file order with
//                        the pixels' current and saved (disposal 3) colours in registers; only the frames asked for are stored,
//                        as three whole dwords per thread where the frame's bytes allow it
// Byte work; no MFMA.
#include "jpeg_bits.h"                 // jd_stage_dword: masked dwords of a byte buffer; jd_wave_sync: a wave's own barrier

#define GI_TABLE 4096                  // GIF89a Appendix F: codes have at most 12 bits

// ------------------------------------------------------------------------------------------------------------------------ LZW
// the bit reader, least significant bit first: `hold` has `have` unread bits from bit 0 up.  Lane l keeps dword 64 c + l of the frame in
// `cur` for the chunk c being read and in `nxt` for the chunk behind it; bytes at or behind the frame's last read as 0, and used()
// tells the caller when it has gone past them
struct gi_reader {
  const uint8_t* scan;
  int64_t first, hi, wi;               // the frame's bytes first .. hi of scan; wi: dwords taken into hold
  uint64_t hold;
  uint32_t cur, nxt;
  int have, lane;
  __device__ __forceinline__ uint32_t load(int64_t chunk) const {
    const int64_t at = first + 4 * (chunk * 64 + lane);
    return at < hi ? jd_stage_dword(scan, at, 0, hi) : 0u;
  }
  __device__ __forceinline__ void open() {
    wi = 0; hold = 0; have = 0;
    cur = load(0);
    nxt = load(1);
  }
  __device__ __forceinline__ void refill() {                                     // afterwards have >= 33
    if (have <= 32) {
      const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(wi & 63));
      hold |= (uint64_t)w << have;
      have += 32;
      wi++;
      if ((wi & 63) == 0) { cur = nxt; nxt = load((wi >> 6) + 1); }
    }
  }
  __device__ __forceinline__ uint32_t take(int k) {                              // k <= 12
    const uint32_t v = (uint32_t)hold & ((1u << k) - 1u);
    hold >>= k; have -= k;
    return v;
  }
  __device__ __forceinline__ int64_t used() const { return wi * 32 - have; }     // bits since the frame's first
};

// the stores of this wave to `out` so far are visible to its loads behind this
__device__ __forceinline__ void gi_publish() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(64) void gif_lzw_kernel(const uint8_t* __restrict__ scan, int64_t scan_bytes, const int64_t* __restrict__ offsets,
                                                     const int32_t* __restrict__ code_size, const int64_t* __restrict__ out_offsets,
                                                     uint8_t* indices, int32_t* __restrict__ produced, int32_t* __restrict__ status, int n) {
  __shared__ uint32_t t_start[GI_TABLE];                                         // entry -> where its string begins in the frame's output
  __shared__ uint16_t t_len[GI_TABLE];                                           //          and its length
  const int lane = threadIdx.x;
  for (int f = blockIdx.x; f < n; f += gridDim.x) {                              // wave-uniform, as everything below
    int64_t lo = offsets[f], hi = offsets[f + 1];
    if (lo < 0 || hi < lo || hi > scan_bytes) lo = hi = 0;                       // offsets that run backwards or leave the buffer: an empty frame
    int64_t olo = out_offsets[f], ohi = out_offsets[f + 1];
    if (olo < 0 || ohi < olo || ohi - olo > 0x7FFFFFFFLL) ohi = olo = 0;         // no room: nothing is written
    const int cs = code_size[f];
    const int64_t total = (hi - lo) * 8;
    const int cap = (int)(ohi - olo);
    uint8_t* out = indices + olo;
    const int clear = 1 << (cs & 15), eoi = clear + 1;
    gi_reader r;
    r.scan = scan; r.first = lo; r.hi = hi; r.lane = lane;
    r.open();
    int pos = 0, fenced = 0, st = EMO_GIF_OK;
    int width = cs + 1, next = clear + 2;
    int pstart = 0, plen = 0;                                                    // the previous string; plen 0: none (the start, behind a Clear)
    if (cs < 2 || cs > 8) st = EMO_GIF_BAD_CODE;
    jd_wave_sync();                                                              // the frame before is done with the table
    while (st == EMO_GIF_OK && pos < cap) {                                      // codes: every turn takes at least 3 bits
      r.refill();
      const int code = (int)r.take(width);
      if (r.used() > total) { st = EMO_GIF_PAST_END; break; }
      if (code == clear) { width = cs + 1; next = clear + 2; plen = 0; continue; }
      if (code == eoi) { st = EMO_GIF_SHORT; break; }
      int s, l;
      if (plen == 0) {                                                           // the first code of a table: a literal
        if (code > clear) { st = EMO_GIF_BAD_CODE; break; }
        s = pos; l = 1;
      } else {
        if (code > next || (code == next && next >= GI_TABLE)) { st = EMO_GIF_BAD_CODE; break; }
        if (next < GI_TABLE) {                                                   // the previous string plus this one's first byte
          if (lane == 0) { t_start[next & (GI_TABLE - 1)] = (uint32_t)pstart; t_len[next & (GI_TABLE - 1)] = (uint16_t)(plen + 1); }
          jd_wave_sync();
        }
        if (code < clear) { s = pos; l = 1; }
        else {                                                                   // the same in every lane: kept in scalar registers
          s = __builtin_amdgcn_readfirstlane((int)t_start[code & (GI_TABLE - 1)]);
          l = __builtin_amdgcn_readfirstlane((int)t_len[code & (GI_TABLE - 1)]);
        }
        if (next < GI_TABLE) {
          next++;
          if (next == (1 << width) && width < 12) width++;
        }
      }
      if (code < clear) {
        if (lane == 0) out[pos] = (uint8_t)code;                                 // pos < cap
      } else {
        l = min(l, cap - pos);                                                   // decoding stops at the frame's last index
        const int dist = pos - s;                                                // >= 1: an entry begins in front of the write position
        if (dist < 1 || s < 0) { st = EMO_GIF_BAD_CODE; break; }                 // (cannot happen: entries are made from positions below pos)
        if (s + min(l, dist) > fenced) { gi_publish(); fenced = pos; }
        for (int b = 0; b < l; b += 64) {                                        // every source byte lies in front of pos: steps do not feed each other
          const int i = b + lane;
          if (i < l) {
            const int o = l > dist ? i % dist : i;
            out[pos + i] = out[min(s + o, cap - 1)];                             // pos + i < cap
          }
        }
      }
      pstart = pos; plen = l;
      pos += l;
    }
    if (lane == 0) {
      produced[f] = pos;
      status[f] = st;
    }
  }
}

extern "C" int emo_gif_lzw_decode(const uint8_t* streams, int64_t stream_bytes, const int64_t* offsets, const int32_t* code_size,
                                  const int64_t* out_offsets, uint8_t* indices, int32_t* produced, int32_t* status, int n, void* stream) {
  EMO_CHECK(streams && offsets && code_size && out_offsets && indices && produced && status, EMO_ERR_NULL, "emo_gif_lzw_decode: null pointer");
  EMO_CHECK(n >= 1, EMO_ERR_BAD_SHAPE, "emo_gif_lzw_decode: n=%d (at least 1 frame)", n);
  EMO_CHECK(stream_bytes > 0 && stream_bytes % 4 == 0 && (uintptr_t)streams % 4 == 0, EMO_ERR_BAD_SHAPE,
            "emo_gif_lzw_decode: the streams are read as 32-bit words: 4-byte aligned, stream_bytes (%lld) a positive multiple of 4", (long long)stream_bytes);
  EMO_CHECK((uintptr_t)offsets % 8 == 0 && (uintptr_t)out_offsets % 8 == 0 && (uintptr_t)code_size % 4 == 0 && (uintptr_t)produced % 4 == 0 &&
            (uintptr_t)status % 4 == 0, EMO_ERR_BAD_SHAPE,
            "emo_gif_lzw_decode: offsets and out_offsets must be 8-byte aligned, code_size, produced and status 4-byte aligned");
  gif_lzw_kernel<<<n < 16384 ? n : 16384, 64, 0, as_stream(stream)>>>(streams, stream_bytes, offsets, code_size, out_offsets, indices, produced,
                                                                       status, n);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------------------ compose
#define GC_PIXELS 4                    // pixels of a thread: 12 bytes, three dwords of a returned frame

// the row of a frame's stream that canvas row y of its h rows reads (GIF89a Appendix E: passes of every 8th row from 0, every 8th from
// 4, every 4th from 2, every 2nd from 1)
__device__ __forceinline__ int gc_stream_row(int y, int h) {
  const int a = (h + 7) >> 3, b = (max(h - 4, 0) + 7) >> 3, c = (max(h - 2, 0) + 3) >> 2;
  if ((y & 7) == 0) return y >> 3;
  if ((y & 7) == 4) return a + ((y - 4) >> 3);
  if ((y & 3) == 2) return a + b + ((y - 2) >> 2);
  return a + b + c + ((y - 1) >> 1);
}

__device__ __forceinline__ uint32_t gc_colour(const uint8_t* __restrict__ tables, int row, int index) {
  const uint8_t* e = tables + ((int64_t)row * 256 + (index & 255)) * 3;
  return (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16;
}

__global__ __launch_bounds__(256) void gif_compose_kernel(const uint8_t* __restrict__ indices, const int64_t* __restrict__ out_offsets,
                                                          const int32_t* __restrict__ frames, const uint8_t* __restrict__ tables,
                                                          uint8_t* __restrict__ rgb, int32_t* __restrict__ status, int n, int n_tables, int n_out,
                                                          int H, int W) {
  const int64_t pixels = (int64_t)H * W, p0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * GC_PIXELS;
  const bool dwords = (pixels * 3) % 4 == 0 && p0 + GC_PIXELS <= pixels;         // every frame of rgb then begins on a dword, and so do this thread's 12 bytes
  int x[GC_PIXELS], y[GC_PIXELS];
  uint32_t cur[GC_PIXELS], saved[GC_PIXELS];
#pragma unroll
  for (int j = 0; j < GC_PIXELS; j++) {
    const int64_t p = min(p0 + j, pixels - 1);
    y[j] = (int)(p / W); x[j] = (int)(p % W);
    cur[j] = saved[j] = 0;
  }
  int pl = 0, pt = 0, pw = 0, ph = 0, pdisp = 0;                                 // the rectangle and the pending action of the frame before
  uint32_t pfill = 0;
  for (int k = 0; k < n; k++) {                                                  // block-uniform: the descriptors are the same for every thread
    const int32_t* d = frames + (int64_t)k * EMO_GIF_FRAME_INTS;
    const int left = d[0], top = d[1], w = d[2], h = d[3], transparent = d[4], disposal = d[5], fill = d[6], interlace = d[7], row = d[8],
              entries = d[9], slot = d[10];
    const int64_t first = out_offsets[k];
    if (left < 0 || top < 0 || w < 1 || h < 1 || (int64_t)left + w > W || (int64_t)top + h > H || row < 0 || row >= n_tables || slot >= n_out ||
        entries < 1 || entries > 256 || out_offsets[k + 1] - first != (int64_t)w * h || first < 0) {
      if (p0 == 0) atomicOr(&status[k], EMO_GIF_BAD_FRAME);                     // a descriptor that does not fit: the frame is left out
      continue;
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < GC_PIXELS; j++) {
      if (k == 0) cur[j] = gc_colour(tables, row, transparent >= 0 ? transparent : 0);
      if (pdisp >= 2 && x[j] >= pl && x[j] < pl + pw && y[j] >= pt && y[j] < pt + ph) cur[j] = pdisp == 2 ? pfill : saved[j];
      const bool inside = x[j] >= left && x[j] < left + w && y[j] >= top && y[j] < top + h;
      if (inside) {
        saved[j] = cur[j];
        const int sy = interlace ? gc_stream_row(y[j] - top, h) : y[j] - top;
        const int index = indices[first + (int64_t)sy * w + (x[j] - left)];
        if (k == 0 || index != transparent) {
          bad = bad || index >= entries;
          cur[j] = gc_colour(tables, row, index);
        }
      }
    }
    pl = left; pt = top; pw = w; ph = h; pdisp = disposal; pfill = gc_colour(tables, row, fill);
    const unsigned long long offending = __ballot(bad && p0 < pixels);           // every lane is here: the loop is uniform
    if (offending && (int)(threadIdx.x & 63) == __ffsll((long long)offending) - 1) atomicOr(&status[k], EMO_GIF_BAD_INDEX);      // one atomic per wave
    if (slot >= 0 && p0 < pixels) {
      uint8_t* o = rgb + ((int64_t)slot * pixels + p0) * 3;
      if (dwords) {
        uint32_t* o4 = (uint32_t*)o;
        o4[0] = cur[0] | cur[1] << 24;
        o4[1] = cur[1] >> 8 | cur[2] << 16;
        o4[2] = cur[2] >> 16 | cur[3] << 8;
      } else {
#pragma unroll
        for (int j = 0; j < GC_PIXELS; j++)
          if (p0 + j < pixels) {
            o[3 * j] = (uint8_t)cur[j]; o[3 * j + 1] = (uint8_t)(cur[j] >> 8); o[3 * j + 2] = (uint8_t)(cur[j] >> 16);
          }
      }
    }
  }
}

extern "C" int emo_gif_compose(const uint8_t* indices, const int64_t* out_offsets, const int32_t* frames, const uint8_t* tables, uint8_t* rgb,
                               int32_t* status, int n, int n_tables, int n_out, int H, int W, void* stream) {
  EMO_CHECK(indices && out_offsets && frames && tables && rgb && status, EMO_ERR_NULL, "emo_gif_compose: null pointer");
  EMO_CHECK(n >= 1 && n_tables >= 1 && n_out >= 1 && n_out <= n && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, EMO_ERR_BAD_SHAPE,
            "emo_gif_compose: n=%d n_tables=%d n_out=%d H=%d W=%d (at least 1 each, n_out <= n, a GIF screen is at most 65535 each way)", n,
            n_tables, n_out, H, W);
  EMO_CHECK((int64_t)H * W <= 0x7FFFFFFFLL / 3 / n_out, EMO_ERR_BAD_SHAPE,
            "emo_gif_compose: %d frames of %d x %d x 3 bytes; the returned frames are counted in 31 bits", n_out, H, W);
  EMO_CHECK((uintptr_t)out_offsets % 8 == 0 && (uintptr_t)frames % 4 == 0 && (uintptr_t)status % 4 == 0 && (uintptr_t)rgb % 4 == 0, EMO_ERR_BAD_SHAPE,
            "emo_gif_compose: out_offsets must be 8-byte aligned, frames, status and rgb 4-byte aligned");
  hipStream_t s = as_stream(stream);
  const hipError_t e = hipMemsetAsync(status, 0, (size_t)n * sizeof(int32_t), s);
  if (e != hipSuccess) return emo_fail(EMO_ERR_HIP, "emo_gif_compose: hipMemsetAsync: %s", hipGetErrorString(e));
  const int64_t threads = ((int64_t)H * W + GC_PIXELS - 1) / GC_PIXELS;
  gif_compose_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(indices, out_offsets, frames, tables, rgb, status, n, n_tables, n_out, H, W);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
