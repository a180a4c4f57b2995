// video_in_progressive.hip - the entropy decoder of progressive JPEG files (ITU-T T.81 Annex G, SOF2, Huffman coding), the device half
// of decode_mjpeg(progressive=True) (emote_hack_amd/video_io.py is the host half: it walks the scans of a file, keeps the Huffman
// tables and the restart interval each scan saw, and refuses progressions that are not complete).
//   emo_jpeg_progressive_scan : ONE scan of a progression, for many frames at once, into the [n][n_mcu][bpm][64] zig-zag coefficient
//                               buffer that emo_jpeg_idct reads.  Like emo_jpeg_decode_segments: one WAVEFRONT per segment - a restart
//                               interval of the scan in one frame, or the frame's whole scan - four segments per workgroup.  A wave loads the tables its segment names into its own part of LDS, its 64 lanes
//                               stage the stream a window at a time and move blocks between the buffer and LDS (lane = coefficient), its
//                               lane 0 walks the codes in between.  A scan writes positions Ss .. Se of the blocks of its units only; the
//                               scans of a progression are launched one behind the other on a stream, which is their only ordering.
// The four procedures are those of jdphuff.c: decode_mcu_DC_first, decode_mcu_DC_refine, decode_mcu_AC_first, decode_mcu_AC_refine
// (T.81 G.1.2.1 - G.1.2.3, G.2).  Every loop is counted, every read of the stream is masked to the segment's bytes, the segment table
// is clamped to the buffers, an error ends the segment.
// The bit reader, the symbol look-up and the staging window are those of video_in.hip: jpeg_bits.h.
#include "jpeg_bits.h"

#define JP_ITEM_BYTES_MAX 216                      // a block of a scan is at most 63 * 26 + 30 bits (AC first), 63 * 18 + 30 (AC refine)
#define JP_BLOCKS 32                               // blocks walked between two flushes (4 KiB of coefficients per wave)
#define JP_WAVES 4                                 // segments (wavefronts) per workgroup
#define JP_TABLES 3                                // tables a segment can name: the DC tables of an interleaved scan's components

// what a launch is constant in
struct jp_scan {
  int ncomp, hs, vs, bpm;        // the layout; bpm blocks per MCU
  int mcu_cols, n_mcu;           // the MCU grid of a frame
  int bw, units;                 // a one-component scan: block columns of the component's own grid (A.2.2), its blocks; an
  //                                interleaved scan: units = n_mcu
  int Ss, Se, Al;
  int scan_comp;                 // -1: interleaved over all components, else the one component
};

// Block (of its frame's n_mcu * bpm) of item g of a scan.  Interleaved: item = MCU * bpm + block, the buffer's own order (A.2.3).  One
// component: item = block (by, bx) of the component's own grid in raster order (A.2.2) - luminance block (by, bx) lives in MCU
// (by / vs, bx / hs) at (by % vs) * hs + bx % hs, a chrominance block is its MCU's Cb or Cr block.
__device__ __forceinline__ int jp_block_of(const jp_scan& p, int g) {
  if (p.scan_comp < 0 || p.ncomp == 1) return g;
  const int by = g / p.bw, bx = g - by * p.bw;
  if (p.scan_comp == 0) return ((by / p.vs) * p.mcu_cols + bx / p.hs) * p.bpm + (by % p.vs) * p.hs + bx % p.hs;
  return (by * p.mcu_cols + bx) * p.bpm + p.hs * p.vs + p.scan_comp - 1;
}

enum { JP_DC_FIRST = 0, JP_DC_REFINE = 1, JP_AC_FIRST = 2, JP_AC_REFINE = 3 };
#define JP_NO_CODE (-1)                            // jp_item: no code of the table matches - undefined, or cut short by the segment's end

// One block of a scan, b[64] in zig-zag order as the buffer holds it (a first scan: its band zeroed).  items_left: the blocks the
// segment still has, this one included.  history: bit k set where b[k] is not 0 (read by an AC refinement only, which so passes the
// coefficients with a zero history in registers and reads b[k] only where a correction bit is 1).  Returns EMO_JPEG_OK or what ended the segment (the caller turns it into PAST_END when the
// reader has left the segment's bits).
template <int PROC>
__device__ __forceinline__ int jp_item(jd_reader& r, const int32_t* tab, const uint16_t* lut, int& pred, int& eobrun, int16_t* b,
                                       uint64_t history, const jp_scan& p, int items_left) {
  if (PROC == JP_DC_FIRST) {                                   // G.1.2.1, decode_mcu_DC_first: F.2.2.1, the value shifted left by Al
    const int s = jd_symbol(r, lut, tab);
    if (s < 0) return JP_NO_CODE;
    if (s > 11) return EMO_JPEG_BAD_CODE;
    pred = (int)((uint32_t)pred + (uint32_t)jd_extend(r, s));
    b[0] = (int16_t)((uint32_t)pred << p.Al);
    return EMO_JPEG_OK;
  }
  if (PROC == JP_DC_REFINE) {                                  // G.1.2.1, decode_mcu_DC_refine: one bit per block
    if (r.bits(1)) b[0] = (int16_t)(b[0] | (1 << p.Al));
    return EMO_JPEG_OK;
  }
  const int Ss = p.Ss, Se = p.Se;
  if (PROC == JP_AC_FIRST) {                                   // G.1.2.2, decode_mcu_AC_first
    if (eobrun > 0) {                                          // inside an EOB run: the band stays zero
      eobrun--;
      return EMO_JPEG_OK;
    }
    int k = Ss;
    for (int it = 0; it <= Se - Ss && k <= Se; it++) {         // every symbol moves k on by at least one
      const int rs = jd_symbol(r, lut, tab);
      if (rs < 0) return JP_NO_CODE;
      const int run = rs >> 4, s = rs & 15;
      if (s) {
        if (s > 10) return EMO_JPEG_BAD_CODE;
        const int v = jd_extend(r, s);
        k += run;
        if (k > Se) return EMO_JPEG_BAD_RUN;
        b[k++] = (int16_t)((uint32_t)v << p.Al);
      } else if (run == 15) {                                  // ZRL
        k += 16;
        if (k > Se + 1) return EMO_JPEG_BAD_RUN;
      } else {                                                 // EOBn: this block's band and those of the next EOBRUN - 1 units
        eobrun = (1 << run) + r.bits(run);
        if (eobrun > items_left) return EMO_JPEG_BAD_RUN;
        eobrun--;
        break;
      }
    }
    return EMO_JPEG_OK;
  }
  // G.1.2.3, decode_mcu_AC_refine
  const int p1 = 1 << p.Al, m1 = -p1;
  int k = Ss;
  if (eobrun == 0) {
    for (int it = 0; it <= Se - Ss && k <= Se; it++) {
      const int rs = jd_symbol(r, lut, tab);
      if (rs < 0) return JP_NO_CODE;
      int run = rs >> 4, val = 0;
      const int s = rs & 15;
      if (s) {
        if (s != 1) return EMO_JPEG_BAD_CODE;
        val = r.bits(1) ? p1 : m1;                             // the new coefficient's sign
      } else if (run != 15) {
        eobrun = (1 << run) + r.bits(run);
        if (eobrun > items_left) return EMO_JPEG_BAD_RUN;
        break;                                                 // the rest of the band is corrected below
      }
      // pass `run` coefficients with a zero history (ZRL: 15, and the 16th is passed as the new one's place); every coefficient with
      // a nonzero history on the way takes one correction bit
      bool placed = false;
      for (; k <= Se; k++) {
        if ((history >> k) & 1) {
          if (r.bits(1)) {
            const int c = b[k];
            if ((c & p1) == 0) b[k] = (int16_t)(c + (c >= 0 ? p1 : m1));
          }
        } else if (--run < 0) {
          placed = true;
          break;
        }
      }
      if (!placed) return EMO_JPEG_BAD_RUN;                    // the run leaves the band
      if (val) b[k] = (int16_t)val;
      k++;
    }
  }
  if (eobrun > 0) {                                            // an EOB run: the band's remaining nonzero coefficients are corrected
    for (; k <= Se; k++) {
      if (((history >> k) & 1) && r.bits(1)) {
        const int c = b[k];
        if ((c & p1) == 0) b[k] = (int16_t)(c + (c >= 0 ? p1 : m1));
      }
    }
    eobrun--;
  }
  return EMO_JPEG_OK;
}

template <int PROC>
__global__ __launch_bounds__(64 * JP_WAVES) void jpeg_progressive_scan_kernel(const uint8_t* __restrict__ scan, int64_t scan_bytes,
                                                                               const int64_t* __restrict__ seg_offsets,
                                                                               const int32_t* __restrict__ seg_frame,
                                                                               const int32_t* __restrict__ seg_first_unit,
                                                                               const int32_t* __restrict__ seg_units,
                                                                               const int32_t* __restrict__ seg_tables,
                                                                               const int32_t* __restrict__ tables, int n_tables,
                                                                               int16_t* __restrict__ coefs, int n, int32_t* __restrict__ status,
                                                                               int n_seg, jp_scan p) {
  __shared__ int32_t tabs[JP_WAVES][JP_TABLES][JD_TABLE_INTS];
  __shared__ uint16_t luts[JP_WAVES][JP_TABLES][256];        // length << 8 | symbol of the code that starts the 8 bits; 0: longer than 8
  __shared__ uint32_t wins[JP_WAVES][(JD_STAGE_BYTES + JD_STAGE_SLACK) / 4];
  __shared__ int16_t blks[JP_WAVES][JP_BLOCKS * 64];
  __shared__ uint64_t hists[JP_WAVES][JP_BLOCKS];            // per block of the round: which coefficients are not 0 (AC refinement)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = blockIdx.x * JP_WAVES + wave;
  if (seg >= n_seg) return;                                  // no workgroup barrier anywhere: the waves walk segments of different lengths
  uint32_t* win = wins[wave];
  int16_t* blk = blks[wave];

  // the tables this segment names, into the wave's own LDS, and figure F.16 on every 8-bit prefix of each
  const bool interleaved = p.scan_comp < 0;
  const int use_tables = PROC == JP_DC_REFINE ? 0 : (interleaved ? p.ncomp : 1);
  for (int s = 0; s < use_tables; s++) {
    const int which = min(max(seg_tables[seg * JP_TABLES + s], 0), n_tables - 1);
    for (int i = lane; i < JD_TABLE_INTS; i += 64) tabs[wave][s][i] = tables[(int64_t)which * JD_TABLE_INTS + i];
  }
  jd_wave_sync();
  for (int s = 0; s < use_tables; s++) {
    const int32_t* tb = tabs[wave][s];
    for (int q = lane; q < 256; q += 64) {
      uint16_t e = 0;
      for (int l = 1; l <= 8; l++) {
        const int code = q >> (8 - l);
        if (code <= tb[16 + l - 1]) {
          e = (uint16_t)(l << 8 | (tb[64 + ((tb[32 + l - 1] + code - tb[l - 1]) & 255)] & 255));
          break;
        }
      }
      luts[wave][s][q] = e;
    }
  }
  jd_wave_sync();

  // the segment's own bytes, frame and units, clamped to the buffers: offsets that leave the scan or run backwards give an empty
  // segment, units that leave the frame's grid are not decoded
  int64_t lo = seg_offsets[seg], hi = seg_offsets[seg + 1];
  lo = min(max(lo, (int64_t)0), scan_bytes);
  hi = min(max(hi, lo), scan_bytes);
  const int64_t seg_bits = (hi - lo) * 8;
  const int frame = min(max(seg_frame[seg], 0), n - 1);
  const int first_unit = min(max(seg_first_unit[seg], 0), p.units);
  const int n_units = min(max(seg_units[seg], 0), p.units - first_unit);
  const int per_unit = interleaved ? p.bpm : 1;
  const int item0 = first_unit * per_unit, n_items = n_units * per_unit;     // < 2^31: checked at the launch
  int16_t* frame_coefs = coefs + (int64_t)frame * p.n_mcu * p.bpm * 64;
  const bool in_band = lane >= p.Ss && lane <= p.Se;

  int done = 0, st = EMO_JPEG_OK;                            // uniform over the wave
  int64_t bitpos = 0;                                        // the walker's place in the segment, uniform too
  int pred0 = 0, pred1 = 0, pred2 = 0, eobrun = 0;           // lane 0's: predictions and the EOB run start at 0 with the segment
  // every round walks at least one block or ends the segment, so n_items rounds are enough
  for (int round = 0; round < n_items && done < n_items; round++) {
    const int cnt = min(JP_BLOCKS, n_items - done);
    // the blocks of the round: lane = coefficient.  A refinement reads what the scans before it left; a first scan starts from zeros
    for (int j = 0; j < cnt; j++) {
      int16_t v = 0;
      if (PROC & 1) v = frame_coefs[(int64_t)jp_block_of(p, item0 + done + j) * 64 + lane];
      blk[j * 64 + lane] = v;
      if (PROC == JP_AC_REFINE) {
        const uint64_t nonzero = __builtin_amdgcn_ballot_w64(v != 0);          // all 64 lanes are here: bit k = coefficient k
        if (lane == 0) hists[wave][j] = nonzero;
      }
    }
    const int64_t byte0 = bitpos >> 3;                       // the window starts at this byte of the segment
    for (int i = lane; i < (JD_STAGE_BYTES + JD_STAGE_SLACK) / 4; i += 64) win[i] = jd_stage_dword(scan, lo + byte0, i, hi);
    jd_wave_sync();
    int nb = 0;
    if (lane == 0) {
      jd_reader r;
      r.open(win, (int)(bitpos & 7));
      const bool holds_end = byte0 + JD_STAGE_BYTES >= hi - lo;
      for (; nb < cnt; nb++) {
        if (!holds_end && (r.used() >> 3) + JP_ITEM_BYTES_MAX > JD_STAGE_BYTES) break;     // the next block may leave the window
        int slot = 0;
        if (interleaved && p.bpm > 1) {                      // block k of an MCU: the luminance blocks first, then Cb, then Cr
          const int k = (item0 + done + nb) % p.bpm;
          slot = k < p.bpm - 2 ? 0 : k - (p.bpm - 3);
        }
        st = jp_item<PROC>(r, tabs[wave][slot], luts[wave][slot], slot == 0 ? pred0 : (slot == 1 ? pred1 : pred2), eobrun,
                           blk + nb * 64, PROC == JP_AC_REFINE ? hists[wave][nb] : 0, p, n_items - done - nb);
        const int64_t at = byte0 * 8 + r.used();
        if (st == JP_NO_CODE) st = at + 16 > seg_bits ? EMO_JPEG_PAST_END : EMO_JPEG_BAD_CODE;     // fewer than 16 bits left: a code cut short
        else if (at > seg_bits) st = EMO_JPEG_PAST_END;     // the bits behind the segment's end read as zeros: whatever they gave
        if (st != EMO_JPEG_OK) break;                        // the block the error is in is dropped with the rest of the segment
      }
      bitpos = byte0 * 8 + r.used();
    }
    jd_wave_sync();
    nb = __builtin_amdgcn_readfirstlane(nb);                 // lane 0's, in scalar registers: the loop stays uniform for the compiler too
    st = __builtin_amdgcn_readfirstlane(st);
    bitpos = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(bitpos >> 32)) << 32 |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)bitpos));
    // flush: positions Ss .. Se of the nb blocks walked, nothing else of them
    if (in_band)
      for (int j = 0; j < nb; j++) frame_coefs[(int64_t)jp_block_of(p, item0 + done + j) * 64 + lane] = blk[j * 64 + lane];
    done += nb;
    jd_wave_sync();
    if (st != EMO_JPEG_OK || nb == 0) break;
  }
  if (lane == 0) status[seg] = st != EMO_JPEG_OK ? st : (done < n_items ? EMO_JPEG_PAST_END : EMO_JPEG_OK);
}

extern "C" int emo_jpeg_progressive_scan(const uint8_t* scan, int64_t scan_bytes, const int64_t* seg_offsets, const int32_t* seg_frame,
                                         const int32_t* seg_first_unit, const int32_t* seg_units, const int32_t* seg_tables,
                                         const int32_t* tables, int n_tables, int16_t* coefs, int32_t* status, int n_seg, int n, int H, int W,
                                         int ncomp, int hs, int vs, int Ss, int Se, int Ah, int Al, int scan_comp, void* stream) {
  const char* who = "emo_jpeg_progressive_scan";
  EMO_CHECK(scan && seg_offsets && seg_frame && seg_first_unit && seg_units && seg_tables && tables && coefs && status, EMO_ERR_NULL,
            "%s: null pointer", who);
  const int bpm = jpeg_bpm(ncomp, hs, vs);
  EMO_CHECK(bpm, EMO_ERR_BAD_SHAPE, JPEG_LAYOUTS_BUILT, who, ncomp, hs, vs);
  EMO_CHECK(n > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535, EMO_ERR_BAD_SHAPE, "%s: n=%d H=%d W=%d (1 .. 65535: SOF2 holds 16 bits)", who, n,
            H, W);
  const int mcu_cols = (W + 8 * hs - 1) / (8 * hs), mcu_rows = (H + 8 * vs - 1) / (8 * vs);
  EMO_CHECK((int64_t)mcu_cols * mcu_rows * n * bpm < (int64_t)1 << 31, EMO_ERR_BAD_SHAPE, "%s: %lld blocks", who,
            (long long)mcu_cols * mcu_rows * n * bpm);
  EMO_CHECK(n_seg > 0 && n_seg <= (1 << 30) && n_tables > 0, EMO_ERR_BAD_SHAPE, "%s: n_seg=%d n_tables=%d", who, n_seg, n_tables);
  EMO_CHECK(scan_comp >= -1 && scan_comp < ncomp, EMO_ERR_BAD_SHAPE, "%s: scan_comp=%d of %d component(s) (-1: interleaved)", who, scan_comp,
            ncomp);
  // T.81 G.1.1.1.1: a DC scan holds coefficient 0 alone; an AC scan holds a band of 1 .. 63 of ONE component
  EMO_CHECK(Ss >= 0 && Ss <= Se && Se <= 63 && (Ss == 0 ? Se == 0 : scan_comp >= 0), EMO_ERR_BAD_SHAPE,
            "%s: Ss=%d Se=%d scan_comp=%d: a DC scan is 0 .. 0, an AC scan a band inside 1 .. 63 of one component", who, Ss, Se, scan_comp);
  EMO_CHECK(Al >= 0 && Al <= 13 && Ah >= 0 && Ah <= 13 && (Ah == 0 || Al == Ah - 1), EMO_ERR_BAD_SHAPE,
            "%s: Ah=%d Al=%d: 0 .. 13 each, a refinement (Ah > 0) steps down by one bit", who, Ah, Al);
  EMO_CHECK(scan_bytes > 0 && scan_bytes % 4 == 0 && (uintptr_t)scan % 4 == 0, EMO_ERR_BAD_SHAPE,
            "%s: the scan buffer is read as 32-bit words: scan 4-byte aligned, scan_bytes (%lld) a multiple of 4", who, (long long)scan_bytes);
  EMO_CHECK((uintptr_t)coefs % 2 == 0 && (uintptr_t)seg_offsets % 8 == 0 && (uintptr_t)seg_frame % 4 == 0 && (uintptr_t)seg_first_unit % 4 == 0 &&
                (uintptr_t)seg_units % 4 == 0 && (uintptr_t)seg_tables % 4 == 0 && (uintptr_t)tables % 4 == 0 && (uintptr_t)status % 4 == 0,
            EMO_ERR_BAD_SHAPE, "%s: seg_offsets must be 8-byte aligned, the other tables 4-byte, coefs 2-byte aligned", who);
  jp_scan p;
  p.ncomp = ncomp; p.hs = hs; p.vs = vs; p.bpm = bpm;
  p.mcu_cols = mcu_cols; p.n_mcu = mcu_cols * mcu_rows;
  p.Ss = Ss; p.Se = Se; p.Al = Al; p.scan_comp = scan_comp;
  if (scan_comp < 0 || ncomp == 1) {
    p.bw = mcu_cols; p.units = p.n_mcu;
  } else {                                                   // A.1.1: the component's own ceil(X h / hmax) x ceil(Y v / vmax) samples
    const int hc = scan_comp == 0 ? hs : 1, vc = scan_comp == 0 ? vs : 1;
    p.bw = ((W * hc + hs - 1) / hs + 7) / 8;
    p.units = p.bw * (((H * vc + vs - 1) / vs + 7) / 8);
  }
  const dim3 grid((n_seg + JP_WAVES - 1) / JP_WAVES), block(64 * JP_WAVES);
#define JP_LAUNCH(PROC)                                                                                                                     \
  jpeg_progressive_scan_kernel<PROC><<<grid, block, 0, as_stream(stream)>>>(scan, scan_bytes, seg_offsets, seg_frame, seg_first_unit,      \
                                                                            seg_units, seg_tables, tables, n_tables, coefs, n, status, n_seg, p)
  if (Ss == 0) {
    if (Ah == 0) JP_LAUNCH(JP_DC_FIRST); else JP_LAUNCH(JP_DC_REFINE);
  } else {
    if (Ah == 0) JP_LAUNCH(JP_AC_FIRST); else JP_LAUNCH(JP_AC_REFINE);
  }
#undef JP_LAUNCH
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}
