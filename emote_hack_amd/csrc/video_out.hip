// video_out.hip - baseline JPEG (ITU-T T.81) encoding of the packed 8-bit frames, the device half of the Motion-JPEG writer that stands
// in for `save_videos_grid`'s imageio.mimsave (magicanimate/utils/util.py:21-33; emote_hack_amd/video_io.py is the host half):
//   emo_jpeg_blocks     : RGB -> YCbCr, 4:2:0, 8x8 DCT-II (T.81 A.3.3), quantisation (A.3.4), zig-zag (A.3.6, figure A.6).  One workgroup
//                         owns a whole 16x16 MCU at a time: 256 lanes fetch its 256 pixels (edge pixels replicated), the 2x2 chroma mean and
//                         the six separable DCTs read one staged tile in LDS, and the 768 output bytes leave as coalesced dwords
//   emo_jpeg_count_bits : the exact Huffman-coded size of every block (T.81 F.1.2): one wavefront per block, one coefficient per lane;
//                         the zero runs come from a ballot of the non-zero lanes, not from a serial scan
//   emo_jpeg_emit_bits  : the same per-lane codes, placed by a wave prefix sum behind the block's bit offset and OR-ed MSB-first into the
//                         stream (32-bit atomicOr of byte-swapped words: neighbouring blocks share words, OR commutes, so the bytes are
//                         the same every run)
//   emo_jpeg_count_bits_ri, emo_jpeg_emit_bits_ri : the same two kernels with a restart interval (T.81 E.1.4): the DC predictor returns
//                         to 0 every Ri MCUs, which is all the device has to know of it - where an interval's bits start is the caller's
//                         business, as where a frame's start is (every interval on a byte)
// Byte gathers and bit packing, no MFMA; a 512x512 frame is 1024 MCUs.
#include "common.h"

// 0.5 * c(u) * cos((2x + 1) u pi / 16), c(0) = 1 / sqrt 2: the orthonormal DCT-II basis of A.3.3, rounded once to f32
__device__ const float JPEG_DCT[64] = {
  0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
  0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f,
  0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f,
  0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f,
  0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
  0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f,
  0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f,
  0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f,
};
// zig-zag position of the natural-order coefficient v * 8 + u (figure A.6)
__device__ const uint8_t JPEG_ZIGZAG_OF[64] = {
  0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
  10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63,
};

// ------------------------------------------------------------------------------------------------------------ colour, DCT, quantisation
// 256 lanes = the 16 x 16 pixels of one MCU.  LDS rows are padded by one float (a column walk of an 8- or 16-wide f32 tile would
// otherwise put every lane of a group on the same few banks).
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const uint8_t* __restrict__ img, int16_t* __restrict__ coefs, int64_t n_mcu_total,
                                                          int n_mcu, int mcu_cols, int H, int W, const uint16_t* __restrict__ quant) {
  __shared__ float chroma[2][16][17];   // full-resolution Cb, Cr of the MCU
  __shared__ float blk[6][8][9];        // the six 8x8 sample blocks: Y00 Y01 Y10 Y11 Cb Cr
  __shared__ float tmp[6][8][9];        // after the row pass
  __shared__ float basis[8][9];
  __shared__ float qf[2][64];
  __shared__ uint8_t zz[64];
  __shared__ __attribute__((aligned(4))) int16_t outz[384];
  const int t = threadIdx.x;
  if (t < 64) {
    basis[t >> 3][t & 7] = JPEG_DCT[t];
    zz[t] = JPEG_ZIGZAG_OF[t];
  }
  if (t < 128) qf[t >> 6][t & 63] = fmaxf((float)quant[t], 1.0f);
  const int py = t >> 4, px = t & 15;
  for (int64_t m = blockIdx.x; m < n_mcu_total; m += gridDim.x) {
    const int64_t frame = m / n_mcu;
    const int mi = (int)(m - frame * n_mcu), my = mi / mcu_cols, mx = mi - my * mcu_cols;
    const int y = min(my * 16 + py, H - 1), x = min(mx * 16 + px, W - 1);       // beyond the right / bottom edge: the edge pixel
    const uint8_t* p = img + ((frame * H + y) * (int64_t)W + x) * 3;
    const float r = (float)p[0], g = (float)p[1], b = (float)p[2];
    blk[(py >> 3) * 2 + (px >> 3)][py & 7][px & 7] = 0.299f * r + 0.587f * g + 0.114f * b - 128.0f;
    chroma[0][py][px] = -0.168736f * r - 0.331264f * g + 0.5f * b;
    chroma[1][py][px] = 0.5f * r - 0.418688f * g - 0.081312f * b;
    __syncthreads();
    if (t < 128) {
      const int c = t >> 6, cy = (t >> 3) & 7, cx = t & 7;
      blk[4 + c][cy][cx] = 0.25f * ((chroma[c][2 * cy][2 * cx] + chroma[c][2 * cy][2 * cx + 1]) +
                                    (chroma[c][2 * cy + 1][2 * cx] + chroma[c][2 * cy + 1][2 * cx + 1]));
    }
    __syncthreads();
    for (int it = t; it < 384; it += 256) {           // rows: tmp[b][y][u] = sum_x blk[b][y][x] * basis[u][x]
      const int bq = it >> 6, yy = (it >> 3) & 7, u = it & 7;
      float acc = 0.f;
#pragma unroll
      for (int xx = 0; xx < 8; xx++) acc = fmaf(blk[bq][yy][xx], basis[u][xx], acc);
      tmp[bq][yy][u] = acc;
    }
    __syncthreads();
    for (int it = t; it < 384; it += 256) {           // columns: c[v][u] = sum_y basis[v][y] * tmp[b][y][u], then rintf(c / q)
      const int bq = it >> 6, v = (it >> 3) & 7, u = it & 7;
      float acc = 0.f;
#pragma unroll
      for (int yy = 0; yy < 8; yy++) acc = fmaf(basis[v][yy], tmp[bq][yy][u], acc);
      outz[bq * 64 + zz[v * 8 + u]] = (int16_t)rintf(acc / qf[bq >= 4][v * 8 + u]);
    }
    __syncthreads();
    if (t < 192) ((uint32_t*)(coefs + m * 384))[t] = ((const uint32_t*)outz)[t];
    // the next MCU's first LDS writes (blk, chroma) are behind three barriers from the last reads of them; outz is rewritten only
    // after two more barriers
  }
}

extern "C" int emo_jpeg_blocks(const uint8_t* frames, int16_t* coefs, int n, int H, int W, const uint16_t* quant, void* stream) {
  EMO_CHECK(frames && coefs && quant, EMO_ERR_NULL, "emo_jpeg_blocks: null pointer");
  EMO_CHECK(n > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535, EMO_ERR_BAD_SHAPE, "emo_jpeg_blocks: n=%d H=%d W=%d (1 .. 65535: SOF0 holds 16 bits)",
            n, H, W);
  EMO_CHECK((uintptr_t)coefs % 4 == 0, EMO_ERR_BAD_SHAPE, "emo_jpeg_blocks: coefs must be 4-byte aligned");
  const int mcu_cols = (W + 15) / 16, mcu_rows = (H + 15) / 16;
  const int64_t n_mcu = (int64_t)mcu_cols * mcu_rows, total = n_mcu * n;
  EMO_CHECK(total * 6 < (int64_t)1 << 31, EMO_ERR_BAD_SHAPE, "emo_jpeg_blocks: %lld blocks", (long long)(total * 6));
  const int grid = (int)(total < 4096 ? total : 4096);
  jpeg_blocks_kernel<<<grid, 256, 0, as_stream(stream)>>>(frames, coefs, total, (int)n_mcu, mcu_cols, H, W, quant);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------ entropy coding
// What lane k of the wavefront contributes to its block's code (F.1.2; k = the zig-zag index).  huff: LDS copy of the four tables,
// entry = length << 16 | code, in the order DC luma, AC luma, DC chroma, AC chroma.  The block's code is, in lane order:
//   lane 0        the DC difference: the code of its size category, then `size` magnitude bits (F.1.2.1)
//   lane k >= 1   a non-zero AC coefficient after a run of r zeros: r >> 4 ZRL codes (symbol 0xF0), then the code of (r & 15) << 4 |
//                 size with the magnitude bits behind it (F.1.2.2); a zero coefficient: nothing, except
//   lane 63       a zero LAST coefficient: EOB (symbol 0x00) - every block whose last coefficient is zero ends in exactly one
// code (<= 26 bits: a 16-bit code and 10 or 11 magnitude bits) holds the symbol's code and the magnitude bits; n_zrl ZRL codes go before it.
struct jpeg_lane_code {
  uint32_t code, zrl;      // zrl: the table entry of symbol 0xF0
  int nbits, n_zrl;
  __device__ __forceinline__ int total() const { return nbits + n_zrl * (int)(zrl >> 16); }
};

// b_in_interval: the block's index inside its restart interval (a whole number of MCUs), which is its frame when there are no restarts
__device__ __forceinline__ jpeg_lane_code jpeg_code_of_lane(const int16_t* __restrict__ coefs, int64_t block, int b_in_interval,
                                                            const uint32_t* huff, int lane) {
  const int k6 = b_in_interval % 6;
  const uint32_t* dc_tab = huff + (k6 >= 4 ? 512 : 0);
  const uint32_t* ac_tab = dc_tab + 256;
  int v = coefs[block * 64 + lane];
  if (lane == 0) {
    // the predictor: the previous block of the same component in this interval, 0 at the interval's first MCU (F.1.1.5.1)
    const int back = k6 == 0 ? 3 : (k6 < 4 ? 1 : 6);            // Y00 follows the previous MCU's Y11
    if (b_in_interval >= back) v -= coefs[(block - back) * 64];
  }
  const uint64_t nz = __ballot(v != 0) & ~1ull;                  // the non-zero AC lanes
  const int a = v < 0 ? -v : v;
  const int size = 32 - __clz(a);                                // 0 for a == 0
  const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
  jpeg_lane_code c;
  c.zrl = ac_tab[0xF0];
  c.code = 0; c.nbits = 0; c.n_zrl = 0;
  uint32_t e = 0;
  int extra = 0;
  if (lane == 0) {
    e = dc_tab[size & 15]; extra = size;
  } else if (v != 0) {
    const uint64_t below = nz & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - __clzll((long long)below) : 0;
    const int run = lane - prev - 1;
    c.n_zrl = run >> 4;
    e = ac_tab[((run & 15) << 4) | (size & 15)]; extra = size;
  } else if (lane == 63) {
    e = ac_tab[0];
  }
  if (e >> 16) {
    c.code = ((e & 0xFFFFu) << extra) | mag;
    c.nbits = (int)(e >> 16) + extra;
  }
  return c;
}

__device__ __forceinline__ void jpeg_load_tables(uint32_t* sh, const uint32_t* __restrict__ huff) {
  for (int i = threadIdx.x; i < 1024; i += blockDim.x) sh[i] = huff[i];
  __syncthreads();
}

// one wavefront per block, four blocks per workgroup.  blocks_per_interval: restart interval * 6, blocks_per_frame without one
__global__ __launch_bounds__(256) void jpeg_count_bits_kernel(const int16_t* __restrict__ coefs, int32_t* __restrict__ counts, int64_t n_blocks,
                                                              int blocks_per_frame, int blocks_per_interval,
                                                              const uint32_t* __restrict__ huff) {
  __shared__ uint32_t sh[1024];
  jpeg_load_tables(sh, huff);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t blk = (int64_t)blockIdx.x * 4 + wave; blk < n_blocks; blk += (int64_t)gridDim.x * 4) {   // wave-uniform
    int bits = jpeg_code_of_lane(coefs, blk, (int)(blk % blocks_per_frame) % blocks_per_interval, sh, lane).total();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o, 64);
    if (lane == 0) counts[blk] = bits;
  }
}

// `nbits` (1 .. 32) bits of `code`, MSB first, at bit `pos` of the stream; words at or past n_words are never touched
__device__ __forceinline__ void jpeg_put_bits(uint32_t* __restrict__ words, int64_t n_words, int64_t pos, uint32_t code, int nbits) {
  const int64_t w = pos >> 5;
  const int sh = (int)(pos & 31);
  const uint64_t x = (uint64_t)code << (64 - nbits - sh);
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  if (hi && w >= 0 && w < n_words) atomicOr(words + w, __builtin_bswap32(hi));
  if (lo && w + 1 >= 0 && w + 1 < n_words) atomicOr(words + w + 1, __builtin_bswap32(lo));
}

__global__ __launch_bounds__(256) void jpeg_emit_bits_kernel(const int16_t* __restrict__ coefs, const int64_t* __restrict__ bit_offsets,
                                                             uint32_t* __restrict__ words, int64_t n_words, int64_t n_blocks,
                                                             int blocks_per_frame, int blocks_per_interval,
                                                             const uint32_t* __restrict__ huff) {
  __shared__ uint32_t sh[1024];
  jpeg_load_tables(sh, huff);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t blk = (int64_t)blockIdx.x * 4 + wave; blk < n_blocks; blk += (int64_t)gridDim.x * 4) {   // wave-uniform
    const jpeg_lane_code c = jpeg_code_of_lane(coefs, blk, (int)(blk % blocks_per_frame) % blocks_per_interval, sh, lane);
    const int mine = c.total();
    int incl = mine;                                  // inclusive prefix sum over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    int64_t pos = bit_offsets[blk] + (incl - mine);
    const int zl = (int)(c.zrl >> 16);
    for (int i = 0; i < c.n_zrl; i++) {               // at most 3
      jpeg_put_bits(words, n_words, pos, c.zrl & 0xFFFFu, zl);
      pos += zl;
    }
    if (c.nbits) jpeg_put_bits(words, n_words, pos, c.code, c.nbits);
  }
}

static int jpeg_entropy_args(const char* who, const void* coefs, const void* huff, int n, int n_mcu, int64_t* n_blocks) {
  EMO_CHECK(coefs && huff, EMO_ERR_NULL, "%s: null pointer", who);
  EMO_CHECK(n > 0 && n_mcu > 0 && (int64_t)n * n_mcu * 6 < (int64_t)1 << 31, EMO_ERR_BAD_SHAPE, "%s: n=%d n_mcu=%d", who, n, n_mcu);
  *n_blocks = (int64_t)n * n_mcu * 6;
  return EMO_OK;
}

static int jpeg_count_bits(const char* who, const int16_t* coefs, int32_t* counts, int n, int n_mcu, int restart_mcus, const uint32_t* huff,
                           void* stream) {
  int64_t n_blocks = 0;
  const int rc = jpeg_entropy_args(who, coefs, huff, n, n_mcu, &n_blocks);
  if (rc != EMO_OK) return rc;
  EMO_CHECK(counts, EMO_ERR_NULL, "%s: null pointer", who);
  EMO_CHECK(restart_mcus > 0, EMO_ERR_BAD_SHAPE, "%s: restart_mcus=%d", who, restart_mcus);
  const int64_t g = (n_blocks + 3) / 4;
  jpeg_count_bits_kernel<<<(int)(g < 4096 ? g : 4096), 256, 0, as_stream(stream)>>>(coefs, counts, n_blocks, n_mcu * 6,
                                                                                     (restart_mcus < n_mcu ? restart_mcus : n_mcu) * 6, huff);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

static int jpeg_emit_bits(const char* who, const int16_t* coefs, const int64_t* bit_offsets, uint8_t* out, int64_t out_bytes, int n, int n_mcu,
                          int restart_mcus, const uint32_t* huff, void* stream) {
  int64_t n_blocks = 0;
  const int rc = jpeg_entropy_args(who, coefs, huff, n, n_mcu, &n_blocks);
  if (rc != EMO_OK) return rc;
  EMO_CHECK(bit_offsets && out, EMO_ERR_NULL, "%s: null pointer", who);
  EMO_CHECK(restart_mcus > 0, EMO_ERR_BAD_SHAPE, "%s: restart_mcus=%d", who, restart_mcus);
  EMO_CHECK(out_bytes > 0 && out_bytes % 4 == 0 && (uintptr_t)out % 4 == 0, EMO_ERR_BAD_SHAPE,
            "%s: the stream buffer is written as 32-bit words: out 4-byte aligned, out_bytes (%lld) a multiple of 4", who, (long long)out_bytes);
  const int64_t g = (n_blocks + 3) / 4;
  jpeg_emit_bits_kernel<<<(int)(g < 4096 ? g : 4096), 256, 0, as_stream(stream)>>>(coefs, bit_offsets, (uint32_t*)out, out_bytes / 4, n_blocks,
                                                                                    n_mcu * 6, (restart_mcus < n_mcu ? restart_mcus : n_mcu) * 6,
                                                                                    huff);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// without a restart interval the one interval is the frame
extern "C" int emo_jpeg_count_bits(const int16_t* coefs, int32_t* counts, int n, int n_mcu, const uint32_t* huff, void* stream) {
  return jpeg_count_bits("emo_jpeg_count_bits", coefs, counts, n, n_mcu, n_mcu > 0 ? n_mcu : 1, huff, stream);
}

extern "C" int emo_jpeg_emit_bits(const int16_t* coefs, const int64_t* bit_offsets, uint8_t* out, int64_t out_bytes, int n, int n_mcu,
                                  const uint32_t* huff, void* stream) {
  return jpeg_emit_bits("emo_jpeg_emit_bits", coefs, bit_offsets, out, out_bytes, n, n_mcu, n_mcu > 0 ? n_mcu : 1, huff, stream);
}

extern "C" int emo_jpeg_count_bits_ri(const int16_t* coefs, int32_t* counts, int n, int n_mcu, int restart_mcus, const uint32_t* huff,
                                      void* stream) {
  return jpeg_count_bits("emo_jpeg_count_bits_ri", coefs, counts, n, n_mcu, restart_mcus, huff, stream);
}

extern "C" int emo_jpeg_emit_bits_ri(const int16_t* coefs, const int64_t* bit_offsets, uint8_t* out, int64_t out_bytes, int n, int n_mcu,
                                     int restart_mcus, const uint32_t* huff, void* stream) {
  return jpeg_emit_bits("emo_jpeg_emit_bits_ri", coefs, bit_offsets, out, out_bytes, n, n_mcu, restart_mcus, huff, stream);
}
