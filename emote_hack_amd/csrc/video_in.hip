// video_in.hip - baseline JPEG (ITU-T T.81) decoding of Motion-JPEG frames, the device half of the reader that stands in for
// `VideoReader(path).read()` (magicanimate/utils/videoreader.py; magicanimate/pipelines/animation.py:174-185) and the reverse of
// video_out.hip (emote_hack_amd/video_io.py is the host half: marker segments, byte unstuffing, the decoding tables):
//   emo_jpeg_decode_bits  : Huffman decoding (T.81 F.2.2) of one interleaved scan per frame.  A frame's stream is serial - where a
//                           code starts depends on every code before it - and frames are independent: ONE workgroup per frame.  Its 256
//                           lanes stage the stream through LDS a window at a time and flush the decoded coefficients as coalesced 16-byte
//                           stores; lane 0 walks the codes in between.  Every loop is counted, every read is masked to the frame's bytes,
//                           an error ends the frame.
//   emo_jpeg_decode_segments : the same walk, ONE WAVEFRONT per segment - a restart interval (T.81 B.2.4.4, E.1.4: the stream is byte-aligned
//                           and the DC predictions return to 0 every Ri MCUs, F.1.1.5.1) or a whole frame without restart markers - four
//                           segments per workgroup.  The tables and look-ups are shared in LDS; every wave has its own window and block
//                           buffer, its 64 lanes stage and flush, its lane 0 walks.  Segments differ in length: behind the set-up no
//                           workgroup barrier is met, a wave synchronises with itself only.
//   emo_jpeg_idct         : dequantisation and libjpeg's "islow" integer IDCT (jidctint.c); a wavefront takes eight whole blocks
//                           (1024 contiguous bytes), one column and then one row per lane
//   emo_jpeg_rgb          : libjpeg's "fancy" (triangle) chroma up-sampling on the real chroma plane and its 16-bit fixed-point
//                           YCbCr -> RGB (jdsample.c, jdcolor.c); every lane writes one whole dword of the packed frames
// Every entry takes the scan's layout as three small ints - the number of components NC and the luminance sampling factors HS x VS
// (T.81 A.1.1, A.2.3), chrominance always 1 x 1 - and picks the instance of its kernel, a template over them; an MCU holds
// BPM = HS * VS + 2 blocks, or 1 when NC is 1:
//   4:2:0  NC 3, 2 x 2, MCU 16 x 16, blocks Y00 Y01 Y10 Y11 Cb Cr   h2v2_fancy_upsample (jdsample.c), ycc_rgb_convert (jdcolor.c)
//   4:2:2  NC 3, 2 x 1, MCU 16 x 8,  blocks Y0 Y1 Cb Cr             h2v1_fancy_upsample (jdsample.c), ycc_rgb_convert
//   4:4:4  NC 3, 1 x 1, MCU 8 x 8,   blocks Y Cb Cr                 fullsize_upsample: chroma as it is, ycc_rgb_convert
//   grey   NC 1,        MCU 8 x 8,   one block (not interleaved, T.81 A.2.2)   gray_rgb_convert (jdcolor.c): the sample three times
// The bit reader, the symbol look-up and the staging window are in jpeg_bits.h, which video_in_progressive.hip shares.
// Integer arithmetic throughout: the bytes are those libjpeg's default decoder gives.
#include "jpeg_bits.h"

// the component of block k of an MCU of BPM blocks: the luminance blocks first, then Cb, then Cr
template <int BPM>
__device__ __forceinline__ int jd_component(int k) {
  return BPM == 1 ? 0 : (k < BPM - 2 ? 0 : k - (BPM - 3));
}

// natural (row-major) index of zig-zag position k (T.81 figure A.6)
__device__ const uint8_t JPEG_NATURAL_OF[64] = {
  0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};

// ------------------------------------------------------------------------------------------------------------ entropy decoding
#define JD_BLOCK_BYTES_MAX 216                     // a block is at most 27 + 63 * 26 = 1665 bits
#define JD_BLOCKS 48                               // blocks decoded between two flushes (6 KiB of coefficients)

// the four tables into LDS and figure F.16 on every 8-bit prefix of each; all 256 lanes of the workgroup, which meet two barriers here
__device__ __forceinline__ void jd_tables_to_lds(const int32_t* __restrict__ tables, int32_t* tab, uint16_t (*lut)[256], int t) {
  for (int i = t; i < 4 * JD_TABLE_INTS; i += 256) tab[i] = tables[i];
  __syncthreads();
  for (int i = t; i < 1024; i += 256) {
    const int32_t* tb = tab + (i >> 8) * JD_TABLE_INTS;
    const int p = i & 255;
    uint16_t e = 0;
    for (int l = 1; l <= 8; l++) {
      const int code = p >> (8 - l);
      if (code <= tb[16 + l - 1]) {
        e = (uint16_t)(l << 8 | (tb[64 + ((tb[32 + l - 1] + code - tb[l - 1]) & 255)] & 255));
        break;
      }
    }
    lut[i >> 8][p] = e;
  }
  __syncthreads();
}

// One block into out[64] (zeroed): the DC difference (F.2.2.1) added to `pred`, then at most 63 AC symbols, each of which moves k on by
// at least one (F.2.2.2).  dc_tab / dc_lut: the block's DC table, its AC table right behind.  win_bit0: the window's first bit, counted
// from the start of the frame or segment, which is total_bits long.  Returns EMO_JPEG_OK or what ended the block.
__device__ __forceinline__ int jd_block(jd_reader& r, const int32_t* dc_tab, const uint16_t* dc_lut, int& pred, int16_t* out,
                                        int64_t win_bit0, int64_t total_bits) {
  int s = jd_symbol(r, dc_lut, dc_tab);
  if (s < 0) return win_bit0 + r.used() + 16 > total_bits ? EMO_JPEG_PAST_END : EMO_JPEG_BAD_CODE;
  if (s > 11) return EMO_JPEG_BAD_CODE;
  const int diff = jd_extend(r, s);
  if (win_bit0 + r.used() > total_bits) return EMO_JPEG_PAST_END;
  pred = (int16_t)(pred + diff);
  out[0] = (int16_t)pred;
  int k = 1;
  for (int it = 0; it < 63 && k < 64; it++) {
    const int rs = jd_symbol(r, dc_lut + 256, dc_tab + JD_TABLE_INTS);
    if (rs < 0) return win_bit0 + r.used() + 16 > total_bits ? EMO_JPEG_PAST_END : EMO_JPEG_BAD_CODE;
    const int run = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (win_bit0 + r.used() > total_bits) return EMO_JPEG_PAST_END;
      if (rs == 0) break;                                      // EOB
      if (rs != 0xF0) return EMO_JPEG_BAD_CODE;                // EOBn belongs to progressive scans
      k += 16;                                                 // ZRL
      if (k > 64) return EMO_JPEG_BAD_RUN;
      continue;
    }
    if (s > 10) return EMO_JPEG_BAD_CODE;
    const int v = jd_extend(r, s);
    if (win_bit0 + r.used() > total_bits) return EMO_JPEG_PAST_END;
    k += run;
    if (k > 63) return EMO_JPEG_BAD_RUN;
    out[k++] = (int16_t)v;
  }
  return EMO_JPEG_OK;
}

template <int BPM>
__global__ __launch_bounds__(256) void jpeg_decode_bits_kernel(const uint8_t* __restrict__ scan, int64_t scan_bytes,
                                                               const int64_t* __restrict__ offsets, const int32_t* __restrict__ tables,
                                                               int16_t* __restrict__ coefs, int32_t* __restrict__ status, int n_mcu) {
  __shared__ int32_t tab[4 * JD_TABLE_INTS];
  __shared__ uint16_t lut[4][256];                           // length << 8 | symbol of the code that starts the 8 bits; 0: longer than 8
  __shared__ uint32_t win[(JD_STAGE_BYTES + JD_STAGE_SLACK) / 4];
  __shared__ __attribute__((aligned(16))) int16_t blk[JD_BLOCKS * 64];
  __shared__ int64_t sh_bitpos;                              // the walker's place in the frame, in bits
  __shared__ int sh_done, sh_status, sh_pred[3];
  const int t = threadIdx.x;
  const int frame = blockIdx.x;
  const int n_blocks = n_mcu * BPM;
  // the frame's own bytes: [lo, hi) inside the buffer; offsets that leave it or run backwards give an empty frame
  int64_t lo = offsets[frame], hi = offsets[frame + 1];
  lo = min(max(lo, (int64_t)0), scan_bytes);
  hi = min(max(hi, lo), scan_bytes);
  const int64_t frame_bits = (hi - lo) * 8;

  if (t == 0) {
    sh_bitpos = 0; sh_done = 0; sh_status = EMO_JPEG_OK;
    sh_pred[0] = sh_pred[1] = sh_pred[2] = 0;
  }
  jd_tables_to_lds(tables, tab, lut, t);
  uint4* blk4 = (uint4*)blk;
  for (int i = t; i < JD_BLOCKS * 8; i += 256) blk4[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();

  int done_blocks = 0;                                       // uniform over the workgroup
  // every round decodes at least one block or ends the frame, so n_blocks rounds are enough
  for (int round = 0; round < n_blocks && done_blocks < n_blocks; round++) {
    const int64_t bit0 = sh_bitpos;
    const int64_t byte0 = bit0 >> 3;                         // the window starts at this byte of the frame
    // stage the window: frame bytes byte0 .., bytes at or behind the frame's end as 0
    for (int i = t; i < (JD_STAGE_BYTES + JD_STAGE_SLACK) / 4; i += 256) win[i] = jd_stage_dword(scan, lo + byte0, i, hi);
    __syncthreads();
    if (t == 0) {
      jd_reader r;
      r.open(win, (int)(bit0 & 7));
      const bool holds_end = byte0 + JD_STAGE_BYTES >= hi - lo;
      int pred0 = sh_pred[0], pred1 = sh_pred[1], pred2 = sh_pred[2];
      int st = EMO_JPEG_OK, nb = 0;
      for (; nb < JD_BLOCKS && done_blocks + nb < n_blocks; nb++) {
        if (!holds_end && (r.used() >> 3) + JD_BLOCK_BYTES_MAX > JD_STAGE_BYTES) break;    // the next block may leave the window
        const int comp = jd_component<BPM>((done_blocks + nb) % BPM);
        const int32_t* dc_tab = tab + (comp ? 2 : 0) * JD_TABLE_INTS;
        const uint16_t* dc_lut = lut[comp ? 2 : 0];
        st = jd_block(r, dc_tab, dc_lut, comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2), blk + nb * 64, byte0 * 8, frame_bits);
        if (st != EMO_JPEG_OK) break;
      }
      if (st != EMO_JPEG_OK) {                               // the block the error is in is dropped with the rest of the frame
        for (int i = 0; i < 64; i++) blk[min(nb, JD_BLOCKS - 1) * 64 + i] = 0;
        sh_status = st;
      }
      sh_pred[0] = pred0; sh_pred[1] = pred1; sh_pred[2] = pred2;
      sh_bitpos = byte0 * 8 + r.used();
      sh_done = nb;
    }
    __syncthreads();
    const int nb = sh_done;
    const int st = sh_status;
    // flush: nb whole blocks, 128 contiguous bytes each, as 16-byte stores; then clear them for the next round
    uint4* dst = (uint4*)(coefs + ((int64_t)frame * n_blocks + done_blocks) * 64);
    for (int i = t; i < nb * 8; i += 256) {
      dst[i] = blk4[i];
      blk4[i] = make_uint4(0, 0, 0, 0);
    }
    done_blocks += nb;
    __syncthreads();
    if (st != EMO_JPEG_OK || nb == 0) break;
  }
  // a frame that ended early: its remaining coefficients are zeroed, so the outputs never hold stale memory
  uint4* rest = (uint4*)(coefs + ((int64_t)frame * n_blocks + done_blocks) * 64);
  for (int i = t; i < (n_blocks - done_blocks) * 8; i += 256) rest[i] = make_uint4(0, 0, 0, 0);
  if (t == 0) status[frame] = sh_status != EMO_JPEG_OK ? sh_status : (done_blocks < n_blocks ? EMO_JPEG_PAST_END : EMO_JPEG_OK);
}

extern "C" int emo_jpeg_decode_bits(const uint8_t* scan, int64_t scan_bytes, const int64_t* offsets, const int32_t* tables, int16_t* coefs,
                                    int32_t* status, int n, int n_mcu, int ncomp, int hs, int vs, void* stream) {
  const char* who = "emo_jpeg_decode_bits";
  const int bpm = jpeg_bpm(ncomp, hs, vs);
  EMO_CHECK(bpm, EMO_ERR_BAD_SHAPE, JPEG_LAYOUTS_BUILT, who, ncomp, hs, vs);
  EMO_CHECK(scan && offsets && tables && coefs && status, EMO_ERR_NULL, "%s: null pointer", who);
  EMO_CHECK(n > 0 && n_mcu > 0 && (int64_t)n * n_mcu * bpm < (int64_t)1 << 31 && (int64_t)n_mcu * bpm < (int64_t)1 << 24, EMO_ERR_BAD_SHAPE,
            "%s: n=%d n_mcu=%d", who, n, n_mcu);
  EMO_CHECK(scan_bytes > 0 && scan_bytes % 4 == 0 && (uintptr_t)scan % 4 == 0, EMO_ERR_BAD_SHAPE,
            "%s: the scan buffer is read as 32-bit words: scan 4-byte aligned, scan_bytes (%lld) a multiple of 4", who, (long long)scan_bytes);
  EMO_CHECK((uintptr_t)coefs % 16 == 0 && (uintptr_t)offsets % 8 == 0, EMO_ERR_BAD_SHAPE,
            "%s: coefs must be 16-byte aligned, offsets 8-byte aligned", who);
  switch (bpm) {
    case 1: jpeg_decode_bits_kernel<1><<<n, 256, 0, as_stream(stream)>>>(scan, scan_bytes, offsets, tables, coefs, status, n_mcu); break;
    case 3: jpeg_decode_bits_kernel<3><<<n, 256, 0, as_stream(stream)>>>(scan, scan_bytes, offsets, tables, coefs, status, n_mcu); break;
    case 4: jpeg_decode_bits_kernel<4><<<n, 256, 0, as_stream(stream)>>>(scan, scan_bytes, offsets, tables, coefs, status, n_mcu); break;
    default: jpeg_decode_bits_kernel<6><<<n, 256, 0, as_stream(stream)>>>(scan, scan_bytes, offsets, tables, coefs, status, n_mcu); break;
  }
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------ segments in parallel
#define JS_WAVES 4                                 // segments (wavefronts) per workgroup
static_assert(64 * JS_WAVES == 256, "jd_tables_to_lds strides by 256 lanes");

template <int BPM>
__global__ __launch_bounds__(64 * JS_WAVES) void jpeg_decode_segments_kernel(const uint8_t* __restrict__ scan, int64_t scan_bytes,
                                                                              const int64_t* __restrict__ seg_offsets,
                                                                              const int32_t* __restrict__ seg_first_block,
                                                                              const int32_t* __restrict__ seg_blocks,
                                                                              const int32_t* __restrict__ tables, int16_t* __restrict__ coefs,
                                                                              int64_t coef_blocks, int32_t* __restrict__ status, int n_seg) {
  __shared__ int32_t tab[4 * JD_TABLE_INTS];
  __shared__ uint16_t lut[4][256];
  __shared__ uint32_t wins[JS_WAVES][(JD_STAGE_BYTES + JD_STAGE_SLACK) / 4];
  __shared__ __attribute__((aligned(16))) int16_t blks[JS_WAVES][JD_BLOCKS * 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t* win = wins[wave];
  int16_t* blk = blks[wave];
  uint4* blk4 = (uint4*)blk;
  for (int i = lane; i < JD_BLOCKS * 8; i += 64) blk4[i] = make_uint4(0, 0, 0, 0);
  jd_tables_to_lds(tables, tab, lut, t);                     // the workgroup's last barrier is in here
  const int seg = blockIdx.x * JS_WAVES + wave;
  if (seg >= n_seg) return;

  // the segment's own bytes and blocks, clamped to the buffers: offsets that leave the scan or run backwards give an empty segment,
  // blocks that leave the coefficients are not decoded
  int64_t lo = seg_offsets[seg], hi = seg_offsets[seg + 1];
  lo = min(max(lo, (int64_t)0), scan_bytes);
  hi = min(max(hi, lo), scan_bytes);
  const int64_t seg_bits = (hi - lo) * 8;
  const int64_t first = min(max((int64_t)seg_first_block[seg], (int64_t)0), coef_blocks);
  const int n_blocks = (int)min(max((int64_t)seg_blocks[seg], (int64_t)0), coef_blocks - first);

  int done_blocks = 0, st = EMO_JPEG_OK;                     // uniform over the wave
  int64_t bitpos = 0;                                        // the walker's place in the segment, uniform too
  int pred0 = 0, pred1 = 0, pred2 = 0;                       // lane 0's: the DC predictions start at 0 with the segment
  // every round decodes at least one block or ends the segment, so n_blocks rounds are enough
  for (int round = 0; round < n_blocks && done_blocks < n_blocks; round++) {
    const int64_t byte0 = bitpos >> 3;                       // the window starts at this byte of the segment
    for (int i = lane; i < (JD_STAGE_BYTES + JD_STAGE_SLACK) / 4; i += 64) win[i] = jd_stage_dword(scan, lo + byte0, i, hi);
    jd_wave_sync();
    int nb = 0;
    if (lane == 0) {
      jd_reader r;
      r.open(win, (int)(bitpos & 7));
      const bool holds_end = byte0 + JD_STAGE_BYTES >= hi - lo;
      for (; nb < JD_BLOCKS && done_blocks + nb < n_blocks; nb++) {
        if (!holds_end && (r.used() >> 3) + JD_BLOCK_BYTES_MAX > JD_STAGE_BYTES) break;    // the next block may leave the window
        const int comp = jd_component<BPM>((done_blocks + nb) % BPM);      // a segment starts with an MCU
        st = jd_block(r, tab + (comp ? 2 : 0) * JD_TABLE_INTS, lut[comp ? 2 : 0], comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2),
                      blk + nb * 64, byte0 * 8, seg_bits);
        if (st != EMO_JPEG_OK) break;                        // the block the error is in is dropped with the rest of the segment
      }
      bitpos = byte0 * 8 + r.used();
    }
    jd_wave_sync();
    nb = __builtin_amdgcn_readfirstlane(nb);                 // lane 0's, in scalar registers: the loop stays uniform for the compiler too
    st = __builtin_amdgcn_readfirstlane(st);
    bitpos = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(bitpos >> 32)) << 32 |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)bitpos));
    // flush: nb whole blocks, 128 contiguous bytes each, as 16-byte stores; then clear them for the next round
    uint4* dst = (uint4*)(coefs + (first + done_blocks) * 64);
    for (int i = lane; i < nb * 8; i += 64) {
      dst[i] = blk4[i];
      blk4[i] = make_uint4(0, 0, 0, 0);
    }
    done_blocks += nb;
    jd_wave_sync();
    if (st != EMO_JPEG_OK || nb == 0) break;
  }
  // a segment that ended early: its remaining coefficients are zeroed, so the outputs never hold stale memory
  uint4* rest = (uint4*)(coefs + (first + done_blocks) * 64);
  for (int i = lane; i < (n_blocks - done_blocks) * 8; i += 64) rest[i] = make_uint4(0, 0, 0, 0);
  if (lane == 0) status[seg] = st != EMO_JPEG_OK ? st : (done_blocks < n_blocks ? EMO_JPEG_PAST_END : EMO_JPEG_OK);
}

extern "C" int emo_jpeg_decode_segments(const uint8_t* scan, int64_t scan_bytes, const int64_t* seg_offsets, const int32_t* seg_first_block,
                                        const int32_t* seg_blocks, const int32_t* tables, int16_t* coefs, int64_t coef_blocks,
                                        int32_t* status, int n_seg, int ncomp, int hs, int vs, void* stream) {
  const char* who = "emo_jpeg_decode_segments";
  const int bpm = jpeg_bpm(ncomp, hs, vs);
  EMO_CHECK(bpm, EMO_ERR_BAD_SHAPE, JPEG_LAYOUTS_BUILT, who, ncomp, hs, vs);
  EMO_CHECK(scan && seg_offsets && seg_first_block && seg_blocks && tables && coefs && status, EMO_ERR_NULL, "%s: null pointer", who);
  EMO_CHECK(n_seg > 0 && n_seg <= (1 << 30) && coef_blocks > 0 && coef_blocks < (int64_t)1 << 31, EMO_ERR_BAD_SHAPE,
            "%s: n_seg=%d coef_blocks=%lld", who, n_seg, (long long)coef_blocks);
  EMO_CHECK(scan_bytes > 0 && scan_bytes % 4 == 0 && (uintptr_t)scan % 4 == 0, EMO_ERR_BAD_SHAPE,
            "%s: the scan buffer is read as 32-bit words: scan 4-byte aligned, scan_bytes (%lld) a multiple of 4", who, (long long)scan_bytes);
  EMO_CHECK((uintptr_t)coefs % 16 == 0 && (uintptr_t)seg_offsets % 8 == 0 && (uintptr_t)seg_first_block % 4 == 0 &&
                (uintptr_t)seg_blocks % 4 == 0,
            EMO_ERR_BAD_SHAPE, "%s: coefs must be 16-byte aligned, seg_offsets 8-byte, the block tables 4-byte aligned", who);
  const dim3 grid((n_seg + JS_WAVES - 1) / JS_WAVES), block(64 * JS_WAVES);
#define JS_LAUNCH(BPM)                                                                                                                \
  jpeg_decode_segments_kernel<BPM><<<grid, block, 0, as_stream(stream)>>>(scan, scan_bytes, seg_offsets, seg_first_block, seg_blocks, \
                                                                          tables, coefs, coef_blocks, status, n_seg)
  switch (bpm) {
    case 1: JS_LAUNCH(1); break;
    case 3: JS_LAUNCH(3); break;
    case 4: JS_LAUNCH(4); break;
    default: JS_LAUNCH(6); break;
  }
#undef JS_LAUNCH
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// ------------------------------------------------------------------------------------------------------------ dequantisation, IDCT
// jidctint.c (jpeg_idct_islow), CONST_BITS 13, PASS1_BITS 2.  Sums and products wrap in 32 bits (coefficients no encoder of 8-bit
// samples makes can overflow them: the result is then some value, never undefined behaviour); the shift is arithmetic.
template <int SHIFT>
__device__ __forceinline__ void jpeg_idct_1d(const int32_t* in, int32_t* out) {
  typedef uint32_t u;
  const u i0 = (u)in[0], i1 = (u)in[1], i2 = (u)in[2], i3 = (u)in[3], i4 = (u)in[4], i5 = (u)in[5], i6 = (u)in[6], i7 = (u)in[7];
  u z1 = (i2 + i6) * 4433u;
  const u t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
  const u t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
  const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  u a0 = i7, a1 = i5, a2 = i3, a3 = i1;
  z1 = a0 + a3;
  u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const u z5 = (z3 + z4) * 9633u;
  a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
  z1 *= (u)-7373; z2 *= (u)-20995;
  z3 = z3 * (u)-16069 + z5;
  z4 = z4 * (u)-3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  const u rnd = 1u << (SHIFT - 1);
  out[0] = (int32_t)(t10 + a3 + rnd) >> SHIFT;
  out[1] = (int32_t)(t11 + a2 + rnd) >> SHIFT;
  out[2] = (int32_t)(t12 + a1 + rnd) >> SHIFT;
  out[3] = (int32_t)(t13 + a0 + rnd) >> SHIFT;
  out[4] = (int32_t)(t13 - a0 + rnd) >> SHIFT;
  out[5] = (int32_t)(t12 - a1 + rnd) >> SHIFT;
  out[6] = (int32_t)(t11 - a2 + rnd) >> SHIFT;
  out[7] = (int32_t)(t10 - a3 + rnd) >> SHIFT;
}

#define JI_LD 72       // dwords between two blocks of a wavefront's workspace: 72 % 32 = 8 puts the 64 (block, column) lanes on 64 banks

// A wavefront takes 8 consecutive blocks (1024 contiguous bytes): lane = (block, eighth) loads 8 coefficients as one 16-byte vector,
// then lane = (block, column) runs pass 1 and lane = (block, row) pass 2, and stores its 8 samples as one 8-byte vector.
// One quantiser per component.  The planes are padded to whole MCUs: luminance rows of
// mcu_cols * 8 * HS bytes, chrominance rows of mcu_cols * 8, multiples of 8, so the 8-byte store stays aligned.
template <int NC, int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coefs, const uint16_t* __restrict__ quant,
                                                        uint8_t* __restrict__ yp, uint8_t* __restrict__ cp, int64_t n_blocks, int n_mcu,
                                                        int mcu_cols, int mcu_rows) {
  __shared__ __attribute__((aligned(16))) int32_t ws[4][8 * JI_LD];
  constexpr int NY = NC == 1 ? 1 : HS * VS, BPM = NC == 1 ? 1 : NY + 2;      // luminance blocks, all blocks of an MCU
  __shared__ uint16_t q[NC][64];
  __shared__ uint8_t nat[64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < NC * 64) q[t >> 6][t & 63] = quant[t];
  if (t < 64) nat[t] = JPEG_NATURAL_OF[t];
  __syncthreads();
  int32_t* w = ws[wave] + (lane >> 3) * JI_LD;              // this lane's block
  const int sub = lane & 7;
  const int64_t n_groups = (n_blocks + 7) / 8;
  for (int64_t g0 = (int64_t)blockIdx.x * 4; g0 < n_groups; g0 += (int64_t)gridDim.x * 4) {        // uniform over the workgroup
    const int64_t b = (g0 + wave) * 8 + (lane >> 3);
    const bool live = b < n_blocks;
    const int64_t frame = b / ((int64_t)n_mcu * BPM);
    const int in_frame = (int)(b - frame * n_mcu * BPM), m = in_frame / BPM, k = in_frame - m * BPM;
    if (live) {
      const uint4 v = *(const uint4*)(coefs + b * 64 + sub * 8);
      const uint32_t pk[4] = {v.x, v.y, v.z, v.w};
      const uint16_t* qq = q[k < NY ? 0 : k - NY + 1];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int c = (int16_t)(pk[j >> 1] >> ((j & 1) * 16));
        const int at = nat[sub * 8 + j];
        w[at] = c * (int)qq[at];
      }
    }
    __syncthreads();
    int32_t in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; r++) in[r] = w[r * 8 + sub];       // pass 1: column `sub`
    jpeg_idct_1d<11>(in, out);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) w[r * 8 + sub] = out[r];
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 8; x++) in[x] = w[sub * 8 + x];       // pass 2: row `sub`
    jpeg_idct_1d<18>(in, out);
    __syncthreads();
    if (live) {
      uint32_t p0 = 0, p1 = 0;
#pragma unroll
      for (int x = 0; x < 4; x++) {
        p0 |= (uint32_t)min(max(out[x] + 128, 0), 255) << (8 * x);
        p1 |= (uint32_t)min(max(out[4 + x] + 128, 0), 255) << (8 * x);
      }
      const int my = m / mcu_cols, mx = m - my * mcu_cols;
      uint8_t* dst;
      if (k < NY) {
        const int64_t row = (frame * mcu_rows + my) * (8 * VS) + (k / HS) * 8 + sub;
        dst = yp + row * ((int64_t)mcu_cols * (8 * HS)) + mx * (8 * HS) + (k % HS) * 8;
      } else {
        const int64_t row = ((frame * 2 + (k - NY)) * mcu_rows + my) * 8 + sub;
        dst = cp + row * ((int64_t)mcu_cols * 8) + mx * 8;
      }
      *(uint2*)dst = make_uint2(p0, p1);
    }
  }
}

// the MCU grid of n frames of H x W at luminance factors hs x vs, bpm blocks per MCU
static int jpeg_geometry(const char* who, int n, int H, int W, int hs, int vs, int bpm, int* mcu_rows, int* mcu_cols) {
  EMO_CHECK(n > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535, EMO_ERR_BAD_SHAPE, "%s: n=%d H=%d W=%d (1 .. 65535: SOF0 holds 16 bits)", who, n, H, W);
  *mcu_cols = (W + 8 * hs - 1) / (8 * hs);
  *mcu_rows = (H + 8 * vs - 1) / (8 * vs);
  EMO_CHECK((int64_t)*mcu_cols * *mcu_rows * n * bpm < (int64_t)1 << 31, EMO_ERR_BAD_SHAPE, "%s: %lld blocks", who,
            (long long)*mcu_cols * *mcu_rows * n * bpm);
  return EMO_OK;
}

template <int NC, int HS, int VS>
static int jpeg_idct_launch(const int16_t* coefs, const uint16_t* quant, uint8_t* y_plane, uint8_t* c_planes, int n, int H, int W, void* stream) {
  const char* who = "emo_jpeg_idct";
  constexpr int BPM = NC == 1 ? 1 : HS * VS + 2;
  EMO_CHECK(coefs && quant && y_plane && (c_planes || NC == 1), EMO_ERR_NULL, "%s: null pointer", who);
  int mcu_rows = 0, mcu_cols = 0;
  const int rc = jpeg_geometry(who, n, H, W, HS, VS, BPM, &mcu_rows, &mcu_cols);
  if (rc != EMO_OK) return rc;
  EMO_CHECK((uintptr_t)coefs % 16 == 0 && (uintptr_t)y_plane % 8 == 0 && (uintptr_t)c_planes % 8 == 0, EMO_ERR_BAD_SHAPE,
            "%s: coefs must be 16-byte aligned, the planes 8-byte aligned", who);
  const int n_mcu = mcu_rows * mcu_cols;
  const int64_t n_blocks = (int64_t)n * n_mcu * BPM, g = (n_blocks + 31) / 32;
  jpeg_idct_kernel<NC, HS, VS><<<(int)(g < 4096 ? g : 4096), 256, 0, as_stream(stream)>>>(coefs, quant, y_plane, c_planes, n_blocks, n_mcu,
                                                                                           mcu_cols, mcu_rows);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

extern "C" int emo_jpeg_idct(const int16_t* coefs, const uint16_t* quant, uint8_t* y_plane, uint8_t* c_planes, int n, int H, int W, int ncomp,
                             int hs, int vs, void* stream) {
  switch (jpeg_bpm(ncomp, hs, vs)) {
    case 1: return jpeg_idct_launch<1, 1, 1>(coefs, quant, y_plane, c_planes, n, H, W, stream);
    case 3: return jpeg_idct_launch<3, 1, 1>(coefs, quant, y_plane, c_planes, n, H, W, stream);
    case 4: return jpeg_idct_launch<3, 2, 1>(coefs, quant, y_plane, c_planes, n, H, W, stream);
    case 6: return jpeg_idct_launch<3, 2, 2>(coefs, quant, y_plane, c_planes, n, H, W, stream);
  }
  return emo_fail(EMO_ERR_BAD_SHAPE, JPEG_LAYOUTS_BUILT, "emo_jpeg_idct", ncomp, hs, vs);
}

// ------------------------------------------------------------------------------------------------------------ chroma up-sampling, colour
// ycc_rgb_convert (jdcolor.c): the 16-bit fixed-point transform, cb and cr less 128; R | G << 8 | B << 16
__device__ __forceinline__ uint32_t jpeg_ycc_rgb(int lum, int cb, int cr) {
  const int R = lum + ((91881 * cr + 32768) >> 16);
  const int G = lum + ((-22554 * cb - 46802 * cr + 32768) >> 16);
  const int B = lum + ((116130 * cb + 32768) >> 16);
  return (uint32_t)min(max(R, 0), 255) | (uint32_t)min(max(G, 0), 255) << 8 | (uint32_t)min(max(B, 0), 255) << 16;
}

// One pixel of a 4:2:0 frame: h2v2_fancy_upsample (jdsample.c) on the chroma plane of ch x cw real samples, then the transform.
__device__ __forceinline__ uint32_t jpeg_pixel_rgb(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cp, int64_t frame, int y, int x,
                                                   int ch, int cw, int64_t y_ld, int64_t y_rows, int64_t c_ld, int64_t c_rows) {
  const int r = y >> 1, c = x >> 1;
  const int rn = min(max((y & 1) ? r + 1 : r - 1, 0), ch - 1);      // the nearer of the two neighbouring rows, inside the plane
  const int cn = min(max((x & 1) ? c + 1 : c - 1, 0), cw - 1);
  const int bias = (x & 1) ? 7 : 8;
  int cc[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint8_t* p = cp + (frame * 2 + k) * c_rows * c_ld;
    const int s_here = 3 * (int)p[r * c_ld + c] + (int)p[rn * c_ld + c];
    const int s_side = 3 * (int)p[r * c_ld + cn] + (int)p[rn * c_ld + cn];
    cc[k] = ((3 * s_here + s_side + bias) >> 4) - 128;
  }
  return jpeg_ycc_rgb(yp[(frame * y_rows + y) * y_ld + x], cc[0], cc[1]);
}

// One pixel of a 4:2:2 frame: h2v1_fancy_upsample (jdsample.c) along the row - p the chroma sample at column x >> 1, even columns
// (3 p + left + 1) >> 2, odd ones (3 p + right + 2) >> 2, the neighbour clamped to the cw real samples, which gives libjpeg's first and
// last columns - and no filter down the columns.
__device__ __forceinline__ uint32_t jpeg_pixel_rgb_h2v1(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cp, int64_t frame, int y, int x,
                                                        int cw, int64_t y_ld, int64_t y_rows, int64_t c_ld, int64_t c_rows) {
  const int c = x >> 1;
  const int cn = min(max((x & 1) ? c + 1 : c - 1, 0), cw - 1);
  const int bias = (x & 1) ? 2 : 1;
  int cc[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint8_t* p = cp + ((frame * 2 + k) * c_rows + y) * c_ld;
    cc[k] = ((3 * (int)p[c] + (int)p[cn] + bias) >> 2) - 128;
  }
  return jpeg_ycc_rgb(yp[(frame * y_rows + y) * y_ld + x], cc[0], cc[1]);
}

// One pixel of a 4:4:4 frame (fullsize_upsample: the chroma sample of the pixel itself) or of a grey one (gray_rgb_convert: the sample
// in all three channels, no transform).
template <int NC>
__device__ __forceinline__ uint32_t jpeg_pixel_rgb_full(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cp, int64_t frame, int y, int x,
                                                        int64_t y_ld, int64_t y_rows) {
  const int64_t at = (frame * y_rows + y) * y_ld + x;
  const uint32_t lum = yp[at];
  if (NC == 1) return lum * 0x010101u;
  const int64_t plane = y_rows * y_ld;                       // chroma planes of the luminance plane's size
  return jpeg_ycc_rgb((int)lum, (int)cp[at + frame * plane] - 128, (int)cp[at + (frame + 1) * plane] - 128);
}

// lane = one dword of the packed output: bytes 4 d .. 4 d + 3 belong to pixels (4 d) / 3 and the one behind it
template <int NC, int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cp, uint8_t* __restrict__ rgb,
                                                       int64_t total_bytes, int H, int W, int mcu_rows, int mcu_cols) {
  const int ch = (H + 1) / 2, cw = (W + 1) / 2;
  const int64_t y_ld = (int64_t)mcu_cols * (8 * HS), y_rows = (int64_t)mcu_rows * (8 * VS), c_ld = (int64_t)mcu_cols * 8, c_rows = (int64_t)mcu_rows * 8;
  const int64_t n_pix = total_bytes / 3, n_dwords = (total_bytes + 3) / 4;
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_dwords; d += (int64_t)gridDim.x * 256) {
    const int64_t byte0 = d * 4, p0 = byte0 / 3;
    const int phase = (int)(byte0 - p0 * 3);                 // the channel of the dword's first byte
    uint64_t two = 0;                                        // the 6 bytes of pixels p0, p0 + 1
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int64_t p = p0 + k;
      if (p < n_pix) {
        const int64_t row = p / W;
        const int x = (int)(p - row * W);
        const int64_t frame = row / H;
        const int y = (int)(row - frame * H);
        uint32_t px;
        if (NC == 3 && HS == 2 && VS == 2) px = jpeg_pixel_rgb(yp, cp, frame, y, x, ch, cw, y_ld, y_rows, c_ld, c_rows);
        else if (NC == 3 && HS == 2) px = jpeg_pixel_rgb_h2v1(yp, cp, frame, y, x, cw, y_ld, y_rows, c_ld, c_rows);
        else px = jpeg_pixel_rgb_full<NC>(yp, cp, frame, y, x, y_ld, y_rows);
        two |= (uint64_t)px << (24 * k);
      }
    }
    const uint32_t v = (uint32_t)(two >> (8 * phase));
    if (byte0 + 4 <= total_bytes) {
      *(uint32_t*)(rgb + byte0) = v;
    } else {
      for (int k = 0; byte0 + k < total_bytes; k++) rgb[byte0 + k] = (uint8_t)(v >> (8 * k));
    }
  }
}

template <int NC, int HS, int VS>
static int jpeg_rgb_launch(const uint8_t* y_plane, const uint8_t* c_planes, uint8_t* rgb, int n, int H, int W, void* stream) {
  const char* who = "emo_jpeg_rgb";
  EMO_CHECK(y_plane && (c_planes || NC == 1) && rgb, EMO_ERR_NULL, "%s: null pointer", who);
  int mcu_rows = 0, mcu_cols = 0;
  const int rc = jpeg_geometry(who, n, H, W, HS, VS, NC == 1 ? 1 : HS * VS + 2, &mcu_rows, &mcu_cols);
  if (rc != EMO_OK) return rc;
  EMO_CHECK((uintptr_t)rgb % 4 == 0, EMO_ERR_BAD_SHAPE, "%s: rgb must be 4-byte aligned", who);
  const int64_t total = (int64_t)n * H * W * 3, g = ((total + 3) / 4 + 255) / 256;
  jpeg_rgb_kernel<NC, HS, VS><<<(int)(g < 65536 ? g : 65536), 256, 0, as_stream(stream)>>>(y_plane, c_planes, rgb, total, H, W, mcu_rows, mcu_cols);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

extern "C" int emo_jpeg_rgb(const uint8_t* y_plane, const uint8_t* c_planes, uint8_t* rgb, int n, int H, int W, int ncomp, int hs, int vs,
                            void* stream) {
  switch (jpeg_bpm(ncomp, hs, vs)) {
    case 1: return jpeg_rgb_launch<1, 1, 1>(y_plane, c_planes, rgb, n, H, W, stream);
    case 3: return jpeg_rgb_launch<3, 1, 1>(y_plane, c_planes, rgb, n, H, W, stream);
    case 4: return jpeg_rgb_launch<3, 2, 1>(y_plane, c_planes, rgb, n, H, W, stream);
    case 6: return jpeg_rgb_launch<3, 2, 2>(y_plane, c_planes, rgb, n, H, W, stream);
  }
  return emo_fail(EMO_ERR_BAD_SHAPE, JPEG_LAYOUTS_BUILT, "emo_jpeg_rgb", ncomp, hs, vs);
}
