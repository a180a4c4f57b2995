"""The video writer behind the pipeline: what `save_videos_grid`, `images2video` and `video2images` (magicanimate/utils/util.py:21-33,
:102-113) do through imageio and ffmpeg, as Motion-JPEG in an AVI container with a 16-bit PCM audio stream - a file every player opens.

  jpeg_tables       the quantisation tables of a quality (T.81 Annex K.1 / K.2 under the IJG scaling rule) and the four Huffman tables of
                    Annex K.3 - K.6, with the code / length arrays derived from BITS / HUFFVAL as Annex C does
  encode_mjpeg      packed uint8 frames on the device -> one baseline JPEG file per frame: emo_jpeg_blocks, emo_jpeg_count_bits,
                    emo_jpeg_emit_bits (csrc/video_out.hip), ONE device-to-host copy of the entropy-coded streams, then per frame on the
                    host the padding of the last byte, the 0x00 behind every 0xFF and the marker segments (T.81 Annex B).  With
                    restart_interval= (MCUs, or "row") the scan is cut into restart intervals (T.81 E.1.4): a DRI segment, every interval
                    coded from DC predictions 0 (emo_jpeg_count_bits_ri, emo_jpeg_emit_bits_ri), padded and stuffed on its own, RSTm
                    markers between them - a file whose intervals decode_mjpeg decodes in parallel
  avi_container, write_avi      a classic RIFF `AVI ` file: hdrl (avih, a vids / MJPG stream, optionally an auds / PCM stream), movi with the 00dc and
                    01wb chunks interleaved per frame, idx1.  Below 2^31 bytes (OpenDML is not written)
  read_avi          the reverse, for files write_avi made
  parse_jpeg        one baseline 4:2:0 file -> its size, tables and scan with the stuffed 0x00 bytes taken out (the reverse of jpeg_header
                    and finish_scan); anything else a JPEG file may be is refused by name.  restart=True also takes files with restart
                    intervals: the RSTm markers are checked and taken out, and the intervals' boundaries kept.  layouts=True also takes
                    4:2:2, 4:4:4 and grey files and one quantiser per component; ParsedJpeg.layout says what the file is
  decode_mjpeg      JPEG files (4:2:0, 4:2:2, 4:4:4, grey) -> packed uint8 frames on the device: per set of tables and layout ONE
                    host-to-device copy of the scans and the segment table, then emo_jpeg_decode_segments (one wavefront per restart
                    interval; emo_jpeg_decode_bits, one workgroup per frame, where no frame has restart intervals), emo_jpeg_idct,
                    emo_jpeg_rgb (csrc/video_in.hip) and one read of the segments' status - the bytes libjpeg's default decoder gives
  read_image        one JPEG file -> an (H, W, 3) uint8 frame on the device through decode_mjpeg, resized there under size=
  read_video        read_avi + decode_mjpeg: what `VideoReader(path).read()` is to magicanimate/pipelines/animation.py:174-185
  resize_taps       the per-axis coefficient table of Pillow's `Image.resize` for 8-bit images (Resample.c), in 22-bit fixed point
  resize_frames     `Image.fromarray(f).resize((width, height), filter)` of device frames, byte for byte: emo_image_resize
                    (csrc/image_resize.hip) on the tables above; read_video(size=) applies it to what it decodes
  load_control_clip, comparison_videos      animation.py:174-194 (read, resize, cut, pad to whole context windows) and :217-228 (the
                    source / control / sample clips cut back to the original length), on the device
  median_cut, quantize_frames, gif_delays, encode_gif, write_gif      the other file `imageio.mimsave` is asked for, an animated GIF
                    (GIF89a): emo_gif_histogram -> median cut on the host (table building, like the resize taps) -> emo_gif_map
                    -> emo_gif_lzw_count / emo_gif_lzw_emit (csrc/gif_out.hip; strips of rows coded independently between Clear codes),
                    ONE device-to-host copy of the code streams, then the header, the colour tables, the extensions and the sub-blocks
                    of at most 255 bytes on the host
  deflate_tables, png_zlib_streams, encode_png, encode_apng, write_png, write_apng      the lossless files: PNG stills and animated PNG
                    (ISO 15948, RFC 1950 / 1951): emo_png_filter -> emo_png_lz_count (csrc/png_out.hip; strips of scanlines matched
                    independently) -> ONE small read of the frames' symbol counts -> the Huffman code lengths, the canonical codes and
                    the header of one dynamic block per frame on the host (table building, like median cut) -> emo_png_deflate_bits /
                    emo_png_deflate_emit, one copy of the streams, then header, end-of-block, Adler-32 and the chunks on the host
  parse_png, decode_png, decode_apng      the reverse: the chunks, CRCs, sequence numbers and zlib headers of a PNG / APNG file on the host,
                    then ONE copy of all frames' deflate streams, emo_png_inflate (one wavefront per frame: stored, fixed and dynamic
                    blocks, the 32 KiB window a ring in LDS) and emo_png_unfilter (a skewed wavefront over bands of 64 rows;
                    csrc/png_in.hip), one small read of the statuses and the rows' Adler-32 pairs - the bytes Pillow gives.  read_image
                    takes a `.png`, read_video an `.apng`, an animated `.png` and a numbered pattern through them
  parse_gif, decode_gif      the GIF reader: header, screen descriptor, colour tables, NETSCAPE2.0, graphic control extensions, image
                    descriptors and joined sub-blocks on the host, with the sticky disposal, the fill index and the table row of every
                    frame resolved there; then ONE copy of all frames' LZW data, descriptors and tables, emo_gif_lzw_decode (one
                    wavefront per frame) and emo_gif_compose (the frames replayed per pixel: transparency, disposal, sub-rectangles,
                    interlace; csrc/gif_in.hip), one small read of the statuses - the bytes Pillow's seek + convert("RGB") give.
                    read_image and read_video take a `.gif` through them
  FORMATS           the one table of the files a clip is written as - avi, gif, apng, numbered png stills: per format its extension,
                    the keywords it owns, whether it plays and holds sound, the checks of its options and of its rate, its encoder.
                    Every writer of a clip runs one sequence over its record (_write_clip), and save_plan does for the pipeline's
                    save_path= what the writers do for format=; all of them lay their streams out with _stream_layout
  write_video, save_videos_grid, images2video, video2images, save_images_grid      the reference surface: `.avi`, with format="gif" a
                    `.gif`, with format="apng" an `.apng` (mp4 needs an encoder that is not here); the image grid as `.png` or `.jpg`

File IO and byte framing live here, on the host, like audio_io.read_wav; no arithmetic on pixels does (the grid of save_videos_grid is
assembled by torch copies on the device; its `(x * 255)` truncated to uint8 is the reference's own line; the resize tables hold
coefficients, the pixels meet them in the kernel)."""
from __future__ import annotations

import dataclasses
import functools
import os
import struct
from fractions import Fraction

import numpy as np
import torch

from . import ops

# ---------------------------------------------------------------------------------------------------------------------- T.81 tables
# zig-zag index -> natural (row-major) index, T.81 figure A.6
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
                  dtype=np.int64)
# Annex K.1 (luminance) and K.2 (chrominance), natural order
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Annex K.3 - K.6: (BITS: codes of length 1 .. 16, HUFFVAL), in the order DC luminance, AC luminance, DC chrominance, AC chrominance
_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f0"
    "2433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a"
    "92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9ca"
    "d2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0"
    "156272d10a162434e125f11718191a262728292a35363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a82838485868788898a"
    "92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9ca"
    "d2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_SPECS = (
    ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),                          # K.3
    ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), _AC_LUMA_VALS),                          # K.5
    ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),                          # K.4
    ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), _AC_CHROMA_VALS),                        # K.6
)
HUFFMAN_IDS = ((0, 0), (1, 0), (0, 1), (1, 1))       # (table class Tc: 0 DC / 1 AC, destination Th) of the four, as DHT and SOS name them


def huffman_codes(bits, huffval):
    """Annex C (figures C.1 - C.3): BITS / HUFFVAL -> (code, length) arrays indexed by symbol; length 0 where the symbol has no code"""
    if sum(bits) != len(huffval):
        raise ValueError(f"BITS counts {sum(bits)} codes, HUFFVAL lists {len(huffval)}")
    code, length = np.zeros(256, np.uint32), np.zeros(256, np.uint32)
    c, k = 0, 0
    for size in range(1, 17):
        for _ in range(bits[size - 1]):
            code[huffval[k]], length[huffval[k]] = c, size
            c, k = c + 1, k + 1
        c <<= 1
    return code, length


@dataclasses.dataclass(frozen=True)
class JpegTables:
    quality: int
    quant: np.ndarray          # uint16 (2, 64): luminance, chrominance, NATURAL order (DQT stores them in zig-zag order)
    specs: tuple               # the four (BITS, HUFFVAL) of HUFFMAN_SPECS
    huff: np.ndarray           # uint32 (4, 256): length << 16 | code per symbol, the layout emo_jpeg_count_bits / emo_jpeg_emit_bits read


def _check_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"JPEG quality runs from 1 to 100, got {quality!r}")
    return int(quality)


@functools.lru_cache(maxsize=None)
def _jpeg_tables(quality: int) -> JpegTables:
    s = 5000 // quality if quality < 50 else 200 - 2 * quality          # the IJG rule (jpeg_quality_scaling)
    quant = np.stack([np.clip((np.array(base, np.int64) * s + 50) // 100, 1, 255) for base in (K1_LUMA, K2_CHROMA)]).astype(np.uint16)
    huff = np.stack([(ln << 16) | cd for cd, ln in (huffman_codes(*spec) for spec in HUFFMAN_SPECS)]).astype(np.uint32)
    quant.setflags(write=False)
    huff.setflags(write=False)
    return JpegTables(quality, quant, HUFFMAN_SPECS, huff)


def jpeg_tables(quality: int = 90) -> JpegTables:
    """The tables of a baseline file at `quality` (1 .. 100): base * s, s = 5000 / q below 50 and 200 - 2 q from there, each entry
    clamp((base * s + 50) // 100, 1, 255) - what libjpeg's jpeg_set_quality makes, so a file written here and one Pillow writes at the
    same quality carry the same DQT and DHT segments."""
    return _jpeg_tables(_check_quality(quality))


# ---------------------------------------------------------------------------------------------------------------------- JPEG framing
def _segment(marker: int, body: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


JPEG_MAX_RESTART = 65535      # DRI holds 16 bits (B.2.4.4)


def restart_mcus(restart_interval, width):
    """restart_interval= as the writers take it -> None (no restart intervals: the files written without the keyword) or the interval
    in MCUs: a positive int below 65536, or "row" for one row of 16x16 MCUs, ceil(width / 16)"""
    if restart_interval is None:
        return None
    if isinstance(restart_interval, str) and restart_interval == "row":
        restart_interval = (int(width) + 15) // 16
    if (isinstance(restart_interval, bool) or not isinstance(restart_interval, (int, np.integer))
            or not 1 <= int(restart_interval) <= JPEG_MAX_RESTART):
        raise ValueError(f"restart_interval= takes None, \"row\" (one row of MCUs) or a number of MCUs from 1 to {JPEG_MAX_RESTART} (DRI holds 16 "
                         f"bits), got {restart_interval!r}")
    return int(restart_interval)


@functools.lru_cache(maxsize=64)
def jpeg_header(height: int, width: int, quality: int, restart: int = 0) -> bytes:
    """SOI, JFIF APP0, DQT x 2, SOF0, DHT x 4, [DRI,] SOS (T.81 B.2): everything in front of the entropy-coded segment of a 4:2:0 frame.
    restart: the restart interval in MCUs (B.2.4.4), 0 for a file without one - part of the cache's key"""
    t = jpeg_tables(quality)
    if not (1 <= height <= 65535 and 1 <= width <= 65535):
        raise ValueError(f"a JPEG frame is 1 .. 65535 pixels each way, got {height} x {width}")
    out = [b"\xFF\xD8", _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    for i in range(2):
        out.append(_segment(0xDB, bytes([i]) + t.quant[i][ZIGZAG].astype(np.uint8).tobytes()))
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for (bits, vals), (tc, th) in zip(t.specs, HUFFMAN_IDS):
        out.append(_segment(0xC4, bytes([tc << 4 | th]) + bytes(bits) + bytes(vals)))
    if not 0 <= restart <= JPEG_MAX_RESTART:
        raise ValueError(f"a restart interval is 0 (none) .. {JPEG_MAX_RESTART} MCUs, got {restart}")
    if restart:
        out.append(_segment(0xDD, struct.pack(">H", restart)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def finish_scan(stream: np.ndarray, n_bits: int) -> bytes:
    """An unstuffed entropy-coded stream of n_bits bits (uint8 array, zero beyond the last bit) -> the scan's bytes: the last byte filled
    with 1-bits (F.1.2.3), a 0x00 behind every 0xFF (B.1.1.5), EOI"""
    n = (n_bits + 7) // 8
    a = np.array(stream[:n], dtype=np.uint8)
    if n_bits & 7:
        a[-1] |= (1 << (8 - (n_bits & 7))) - 1
    a = np.insert(a, np.flatnonzero(a == 0xFF) + 1, 0)
    return a.tobytes() + b"\xFF\xD9"


def finish_restart_scan(stream: np.ndarray, interval_bits) -> bytes:
    """The unstuffed streams of a frame's restart intervals, laid end to end with every interval starting on a byte (uint8 array, zero
    beyond each interval's last bit), and the bits of each -> the scan's bytes (T.81 B.2.1, E.1.4): every interval's last byte filled
    with 1-bits and a 0x00 behind every 0xFF (also one that ends an interval), RSTm between two intervals with m counting 0 .. 7 and
    round again, no marker behind the last, EOI"""
    bits = np.asarray(interval_bits, np.int64).reshape(-1)
    if bits.size < 1 or (bits < 1).any():
        raise ValueError(f"finish_restart_scan: every interval holds at least one bit, got {bits.tolist()[:8]}")
    ends = np.cumsum((bits + 7) // 8)                                            # byte end of every interval
    a = np.array(stream[:int(ends[-1])], dtype=np.uint8)
    ragged = np.flatnonzero(bits & 7)
    a[ends[ragged] - 1] |= ((1 << (8 - (bits[ragged] & 7))) - 1).astype(np.uint8)
    ff = np.flatnonzero(a == 0xFF) + 1
    cuts = ends[:-1]
    markers = np.stack([np.full(len(cuts), 0xFF), 0xD0 + np.arange(len(cuts)) % 8], axis=1).reshape(-1)
    # np.insert keeps the given order among values that go to one place: the 0x00 of an 0xFF that ends an interval, then the marker
    a = np.insert(a, np.concatenate([ff, np.repeat(cuts, 2)]), np.concatenate([np.zeros(len(ff)), markers]).astype(np.uint8))
    return a.tobytes() + b"\xFF\xD9"


@functools.lru_cache(maxsize=8)
def _device_tables(quality: int, device: str):
    t = jpeg_tables(quality)
    return (torch.from_numpy(t.quant.copy()).to(device), torch.from_numpy(t.huff.astype(np.int64).astype(np.int32)).to(device))


def _frames_u8(frames_u8, who, channels=(3,), dims=(4, 5), limit=None):
    """The one check of the frames an encoder is handed, before any launch -> them as (n, H, W, C): a uint8 tensor of one of `dims`
    dimensions ((H, W, C) is one frame, (1, n, H, W, C) is folded) whose last is one of `channels`, at least one frame.  limit=(name,
    most) also holds every side to 1 .. most pixels (None: only to at least 1) and names the file format in the refusal."""
    if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() not in dims or frames_u8.shape[-1] not in channels:
        c, what = ("3", "RGB frames") if tuple(channels) == (3,) else ("C", "frames with 1 (grey), 3 (RGB) or 4 (RGBA) channels")
        shapes = {3: f"(H, W, {c})", 4: f"(n, H, W, {c})", 5: f"(1, n, H, W, {c}) as output_type=\"uint8\" returns them"}
        raise ValueError(f"{who} takes packed uint8 {what}, {' or '.join(shapes[d] for d in dims)}, got "
                         f"{getattr(frames_u8, 'dtype', type(frames_u8))} {tuple(getattr(frames_u8, 'shape', ()))}")
    if frames_u8.dim() != 4:
        frames_u8 = frames_u8.reshape(-1, *frames_u8.shape[-3:])
    n, height, width = (int(s) for s in frames_u8.shape[:3])
    if n < 1:
        raise ValueError(f"{who}: no frames")
    if limit is not None and not (1 <= height <= (limit[1] or height) and 1 <= width <= (limit[1] or width)):
        raise ValueError(f"{who}: a {limit[0]} frame is {f'1 .. {limit[1]} pixels' if limit[1] else 'at least 1 pixel'} each way, got {height} x {width}")
    return frames_u8


def _stream_layout(bits, head_bits=None, tail_bytes=0, totals=None):
    """Where every unit's bits go in one buffer of streams.  bits: integer device tensor (rows, units), the bits of every unit (a JPEG
    block, a GIF or PNG strip); a row - a frame, or one restart interval - is whatever must start on a byte, and inside it the units
    follow each other bit by bit.  -> (offsets, starts, nbytes, out, totals): the bit offset of every unit in the buffer (int64,
    contiguous, on bits' device), the byte start and the bytes of every row (int64 numpy), the zeroed uint8 buffer on that device, its
    length rounded up to a multiple of 4 (the kernels OR whole dwords), and the rows' bit totals.  head_bits (per row, host) are left
    free in front of a row's first unit, tail_bytes behind every row's last byte; totals= are the rows' bit totals behind the head
    where the host knows them (they may count bits the caller adds behind the units) - without them they are read from the device,
    the one read of a layout."""
    ends = torch.cumsum(bits, dim=1, dtype=torch.int64)                         # bits, inside each row
    totals = ends[:, -1].cpu().numpy() if totals is None else np.asarray(totals, np.int64)
    head = np.zeros(len(totals), np.int64) if head_bits is None else np.asarray(head_bits, np.int64)
    nbytes = (head + totals + 7) // 8 + int(tail_bytes)
    starts = np.cumsum(nbytes) - nbytes
    offsets = (ends - bits + torch.from_numpy(starts * 8 + head).to(ends.device)[:, None]).contiguous()
    out = torch.zeros((int(nbytes.sum()) + 3) // 4 * 4, device=bits.device, dtype=torch.uint8)
    return offsets, starts, nbytes, out, totals


def encode_streams(frames_u8: torch.Tensor, quality: int = 90, restart_interval=None):
    """The device part of encode_mjpeg: (n, H, W, 3) uint8 device frames -> (streams uint8 device buffer, byte start of every frame, bits
    of every frame); three launches, one read of the n frame totals.  With restart_interval (restart_mcus) every restart interval starts
    on a byte: the starts and the bits come per interval, int64 (n, ceil(MCUs / interval)), from one read of as many totals."""
    quality = _check_quality(quality)
    frames_u8 = _frames_u8(frames_u8, "encode_mjpeg")
    ri = restart_mcus(restart_interval, frames_u8.shape[2])
    frames_u8 = frames_u8.contiguous()
    quant, huff = _device_tables(quality, str(frames_u8.device))
    coefs = ops.jpeg_blocks(frames_u8, quant)
    n, n_mcu = int(coefs.shape[0]), int(coefs.shape[1])
    ri = None if ri is None else min(ri, n_mcu)
    counts = ops.jpeg_count_bits(coefs, huff, restart_mcus=ri)
    if ri is None:
        offsets, starts, _, out, bits = _stream_layout(counts)
    else:      # a row of the layout is one restart interval: k per frame, the last padded with blocks of no bits where it is short
        k = -(-n_mcu // ri)
        per = torch.nn.functional.pad(counts.to(torch.int64), (0, (k * ri - n_mcu) * 6)).view(n * k, ri * 6)
        offsets, starts, _, out, bits = _stream_layout(per)
        offsets, starts, bits = offsets.view(n, k * ri * 6)[:, :n_mcu * 6].contiguous(), starts.reshape(n, k), bits.reshape(n, k)
    ops.jpeg_emit_bits(coefs, huff, offsets, out, restart_mcus=ri)
    return out, starts, bits


def encode_mjpeg(frames_u8: torch.Tensor, quality: int = 90, restart_interval=None) -> list:
    """Packed uint8 RGB frames on the device, (n, H, W, 3) (or the (1, n, H, W, 3) of output_type="uint8") -> n baseline JPEG files
    (bytes; 4:2:0, the standard Huffman tables).  The colour transform, the DCT, the quantisation and the Huffman coding run on the device;
    the compressed streams come back in one copy, and the host pads, stuffs and wraps each.
    restart_interval: None writes one entropy-coded segment per frame.  A positive int of MCUs below 65536, or "row" for one row of
    MCUs (ceil(W / 16)), writes a DRI segment and restart intervals of that many MCUs with RSTm markers between them (T.81 E.1.4): the
    same coefficients, a few bytes more per interval, and a file decode_mjpeg decodes one wavefront per interval.  An interval of at
    least the frame's MCUs writes the DRI segment and no marker."""
    out, starts, bits = encode_streams(frames_u8, quality, restart_interval)    # (checks the arguments)
    host = out.cpu().numpy()
    height, width = int(frames_u8.shape[-3]), int(frames_u8.shape[-2])
    ri = restart_mcus(restart_interval, width)
    if ri is None:
        head = jpeg_header(height, width, int(quality))
        return [head + finish_scan(host[s:], int(b)) for s, b in zip(starts, bits)]
    head = jpeg_header(height, width, int(quality), ri)
    return [head + finish_restart_scan(host[int(s[0]):], b) for s, b in zip(starts, bits)]


# ---------------------------------------------------------------------------------------------------------------------- JPEG parsing
JPEG_MIN_WIDTH = 5      # where chroma is halved along the rows (4:2:0, 4:2:2): libjpeg replicates chroma samples instead of filtering when
#                         the chroma plane is at most 2 wide; that is not built


def huffman_decode_table(bits, huffval) -> np.ndarray:
    """Annex C and F.2.2.3 (figure F.15): BITS / HUFFVAL -> int32 (ops.JPEG_DECODE_TABLE_INTS), the layout emo_jpeg_decode_bits reads:
    MINCODE[16] | MAXCODE[16] | VALPTR[16] | 16 unused | HUFFVAL[256]; entry l - 1 belongs to code length l, MAXCODE is -1 where no
    code has that length"""
    bits, huffval = tuple(int(b) for b in bits), bytes(huffval)
    if len(bits) != 16 or sum(bits) != len(huffval) or len(huffval) > 256:
        raise ValueError(f"a Huffman table has 16 BITS entries that count its at most 256 HUFFVAL entries, got {len(bits)} counting {sum(bits)} "
                         f"for {len(huffval)}")
    t = np.zeros(ops.JPEG_DECODE_TABLE_INTS, np.int32)
    t[16:32] = -1
    code, k = 0, 0
    for l in range(16):
        if bits[l]:
            if code + bits[l] > 1 << (l + 1):
                raise ValueError(f"a Huffman table with {bits[l]} codes of length {l + 1} behind {code} taken is over-subscribed")
            t[l], t[16 + l], t[32 + l] = code, code + bits[l] - 1, k
            code, k = code + bits[l], k + bits[l]
        code <<= 1
    t[64:64 + len(huffval)] = np.frombuffer(huffval, np.uint8)
    return t


@dataclasses.dataclass(frozen=True)
class JpegLayout:
    """How a baseline scan lays its components out (T.81 A.1.1, A.2): one entry per component in the three tuples."""
    components: int            # 3 (Y, Cb, Cr) or 1 (grey)
    factors: tuple             # (h, v) per component; a grey scan is not interleaved, so its factors count as (1, 1) (T.81 A.2.2)
    quant: tuple               # per component the quantisation table destination Tq the frame header gives it (B.2.2)
    huffman: tuple             # per component the (DC, AC) Huffman table destinations (Td, Ta) the scan header gives it (B.2.3)

    @property
    def key(self):
        """(components, luminance h, luminance v): what ops.JPEG_LAYOUTS names and the emo_jpeg_* decode entries take"""
        return (self.components,) + tuple(self.factors[0])

    @property
    def name(self):
        return ops.JPEG_LAYOUTS[self.key]

    @property
    def blocks_per_mcu(self):
        return ops.jpeg_bpm(self.key)


@dataclasses.dataclass(frozen=True)
class JpegScan:
    """One scan of a progressive file (T.81 B.2.3, G.1.1.1.1) with what held when it started."""
    components: tuple          # indices into the frame's components, in the scan header's order
    Ss: int                    # the band of the zig-zag sequence, 0 .. 0 for a DC scan
    Se: int
    Ah: int                    # 0: the band's first scan, else the Al of the scan this one refines
    Al: int                    # the bits below this one are left to later scans
    huffman: tuple             # per component of the scan the (Td, Ta) its header gives it
    specs: tuple               # per component of the scan the ((BITS, HUFFVAL) of DC destination Td, of AC destination Ta) as the DHT
    #                            segments in front of THIS scan left them; None for a destination not defined (and not needed) then
    restart: int               # the restart interval in force at this scan, in its own units (MCUs, or blocks of its one component); 0: none
    scan: np.ndarray           # uint8: the scan's entropy-coded bytes, unstuffed, RSTm markers taken out
    intervals: np.ndarray      # int64 (intervals + 1): as ParsedJpeg.intervals

    @property
    def script(self):
        """what a progression's scan is, without its tables: frames that share these share launches"""
        return self.components, self.Ss, self.Se, self.Ah, self.Al

    def __str__(self):
        return f"{self.Ss}..{self.Se}, Ah/Al {self.Ah}/{self.Al}"


@dataclasses.dataclass(frozen=True)
class ParsedJpeg:
    height: int
    width: int
    quants: np.ndarray         # uint16 (3, 64): the quantiser of every component, NATURAL order (a grey file: its one table three times)
    specs: tuple               # four (BITS tuple, HUFFVAL bytes): DC luminance, AC luminance, DC chrominance, AC chrominance (a grey
    #                            file: the luminance pair twice)
    scan: np.ndarray           # uint8: the entropy-coded segment without the 0x00 behind every 0xFF, up to the marker that ends it
    restart: int = 0           # the restart interval in MCUs (DRI), 0: none
    intervals: np.ndarray = None      # int64 (intervals + 1): restart interval k lies in scan[intervals[k]:intervals[k + 1]] (the RSTm
    #                                   markers are taken out); (0, len(scan)) for a file without restart intervals
    layout: JpegLayout = None
    scans: tuple = None        # a progressive file (parse_jpeg(progressive=True)): one JpegScan per scan in file order; specs is then
    #                            empty, scan and intervals hold no bytes, restart is the interval in force at the first scan.  None: baseline

    @property
    def mcus(self):
        """MCUs of the frame in its own layout (the 8x8 blocks of a grey frame)"""
        return ops.jpeg_mcus(self.height, self.width, self.layout.key)

    @property
    def quant(self):
        """uint16 (2, 64): luminance, chrominance (Cb's) - what jpeg_tables(quality).quant is for a file encode_mjpeg wrote"""
        return self.quants[:2]

    def table_key(self):
        if self.scans is not None:      # Huffman tables and restart intervals may differ inside a group: libjpeg optimises tables per file
            return self.quants.tobytes(), self.layout.key, tuple(s.script for s in self.scans)
        return self.quants.tobytes(), self.specs, self.layout.key


_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic-coded sequential (SOF9)",
              0xCA: "arithmetic-coded progressive (SOF10)", 0xCB: "arithmetic-coded lossless (SOF11)", 0xCD: "arithmetic-coded differential (SOF13)",
              0xCE: "arithmetic-coded differential progressive (SOF14)", 0xCF: "arithmetic-coded differential lossless (SOF15)"}
_ONLY = ("decode_mjpeg reads 8-bit baseline (SOF0) files in one scan: three components (YCbCr) at 2x2 / 1x1 / 1x1 (4:2:0), 2x1 / 1x1 / 1x1 "
         "(4:2:2) or 1x1 / 1x1 / 1x1 (4:4:4), interleaved, or one component (grey)")
_NO_LAYOUTS = "without layouts=True parse_jpeg takes 4:2:0 with one chrominance quantiser only"
_FACTOR_NAMES = {((1, 2), (1, 1), (1, 1)): " (4:4:0)", ((4, 1), (1, 1), (1, 1)): " (4:1:1)", ((2, 2), (1, 1), (1, 1)): " (4:2:0)",
                 ((2, 1), (1, 1), (1, 1)): " (4:2:2)", ((1, 1), (1, 1), (1, 1)): " (4:4:4)"}


def _entropy_bytes(data: bytes, pos: int, units: int, ri: int, what: str, unit: str = "units", restart: bool = True, open_end: bool = False):
    """the entropy-coded bytes that start at data[pos] -> (unstuffed bytes without the RSTm markers, intervals as in ParsedJpeg, the
    position of the marker that ends them); the markers must cut `units` units (called `unit` in messages) at a restart interval of
    `ri` into ceil(units / ri).  restart=False refuses the first RSTm marker; open_end=True takes bytes that run to the end of the data
    with no marker behind them, as the baseline path always has"""
    rst, end, at = [], None, pos                                                 # forward from pos to the first marker that is no RSTm:
    while True:                                                                  # a file of many scans is not searched to its end per scan
        at = data.find(b"\xFF", at)
        if at < 0 or at + 1 >= len(data):
            break
        if data[at + 1] == 0x00:                                                 # a stuffed byte
            at += 2
        elif 0xD0 <= data[at + 1] <= 0xD7:
            if not restart:
                raise ValueError(f"parse_jpeg: a restart marker inside {what}; restart markers are not built; {_ONLY}")
            rst.append(at - pos)
            at += 2
        else:
            end = at - pos
            break
    if end is None:
        if not open_end:
            raise ValueError(f"parse_jpeg: {what} runs to the end of the file: no marker ends it (a cut file)")
        end = len(data) - pos
    a = np.frombuffer(data, np.uint8, count=end, offset=pos)
    if rst or ri:
        if not ri:
            raise ValueError(f"parse_jpeg: {len(rst)} restart marker{'s' if len(rst) != 1 else ''} in {what} (the first at byte {pos + rst[0]}) "
                             "and no restart interval defined by a DRI segment")
        found = [int(a[e + 1]) - 0xD0 for e in rst]
        wrong = [k for k, m in enumerate(found) if m != k % 8]
        if wrong:
            k = wrong[0]
            raise ValueError(f"parse_jpeg: restart marker {k} of {what} is RST{found[k]} (FF{0xD0 + found[k]:02X} at byte {pos + rst[k]}), "
                             f"RST{k % 8} is expected there: the markers count 0 .. 7 and round again (a damaged file; resynchronisation is "
                             "not built)")
        want = -(-units // ri)
        if len(rst) + 1 != want:
            raise ValueError(f"parse_jpeg: {len(rst) + 1} restart interval{'s' if rst else ''} in {what}, {units} {unit} at a restart interval "
                             f"of {ri} make {want} (a damaged file; resynchronisation is not built)")
    keep = np.ones(len(a), bool)
    if len(a) > 1:
        keep[np.flatnonzero((a[:-1] == 0xFF) & (a[1:] == 0x00)) + 1] = False       # the stuffed bytes
    if rst:
        keep[np.array(rst)] = keep[np.array(rst) + 1] = False                    # the markers
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    scan, intervals = a[keep], before[[0] + rst + [len(a)]]
    scan.setflags(write=False)
    intervals.setflags(write=False)
    return scan, intervals, pos + end


_NO_SMOOTHING = ("libjpeg smooths the blocks of such a file from their neighbours (jdcoefct.c smoothing_ok finds coefficients whose bits "
                 "are not all known), which is not built")


def _progressive_scans(data: bytes, pos: int, body: bytes, frame, quant: dict, huff: dict, ri: int) -> tuple:
    """the scans of a progressive file (T.81 G.1.1.1.1) from the body of its first SOS segment, whose entropy-coded bytes start at
    data[pos], to EOI -> a tuple of JpegScan; ValueError for a progression that is not built or not complete"""
    height, width, comps, factors = frame
    nf, key = len(comps), (len(comps),) + factors[0]
    ids = [c[0] for c in comps]
    huff, quant = dict(huff), dict(quant)
    known = [[None] * 64 for _ in range(nf)]                                     # per coefficient the Al of its last scan; None: not coded yet
    scans = []
    while True:
        ns = body[0] if body else 0
        if ns < 1 or len(body) != 4 + 2 * ns:
            raise ValueError(f"parse_jpeg: scan {len(scans)}: a malformed SOS segment")
        sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
        Ss, Se, Ah, Al = body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15
        what = f"scan {len(scans)} (component ids {[c for c, _, _ in sel]}, coefficients {Ss} .. {Se}, Ah / Al {Ah} / {Al})"
        for c, _, _ in sel:
            if c not in ids:
                raise ValueError(f"parse_jpeg: {what} names component {c}, the frame has {ids}")
        idx = tuple(ids.index(c) for c, _, _ in sel)
        if list(idx) != sorted(set(idx)):
            raise ValueError(f"parse_jpeg: {what} lists its components out of the frame's order {ids} (B.2.3)")
        if Ss == 0:
            if Se != 0:
                raise ValueError(f"parse_jpeg: {what}: a scan that starts at the DC coefficient holds it alone (Se = 0; T.81 G.1.1.1.1)")
            if ns not in (1, nf):
                raise ValueError(f"parse_jpeg: {what} is interleaved over {ns} of the frame's {nf} components; all of them or one are built")
        elif ns != 1:
            raise ValueError(f"parse_jpeg: {what}: an AC scan interleaved over {ns} components; it holds one (T.81 G.1.1.1.1)")
        elif Se < Ss or Se > 63:
            raise ValueError(f"parse_jpeg: {what}: an AC band runs from Ss up to Se <= 63 (T.81 G.1.1.1.1)")
        if Al > 13:
            raise ValueError(f"parse_jpeg: {what}: Al above 13 (T.81 G.1.1.1.1)")
        for c in idx:
            if Ss > 0 and known[c][0] is None:
                raise ValueError(f"parse_jpeg: {what}: an AC scan of component {ids[c]} in front of that component's first DC scan")
            for k in range(Ss, Se + 1):
                if known[c][k] is None:
                    if Ah != 0:
                        raise ValueError(f"parse_jpeg: {what}: the first scan of coefficient {k} of component {ids[c]} with Ah = {Ah}, not 0")
                elif Ah != known[c][k] or Ah == 0:
                    raise ValueError(f"parse_jpeg: {what}: a refinement of coefficient {k} of component {ids[c]} with Ah = {Ah}, the scan "
                                     f"before it left Al = {known[c][k]}")
                elif Al != Ah - 1:
                    raise ValueError(f"parse_jpeg: {what}: a refinement steps down by one bit, Al = Ah - 1")
                known[c][k] = Al
            if comps[c][3] not in quant:
                raise ValueError(f"parse_jpeg: quantisation table {comps[c][3]} is used and never defined")
        specs = []
        for c, td, ta in sel:
            need = (0, td) if Ss == 0 else (1, ta)
            if need not in huff and not (Ss == 0 and Ah):                        # a DC refinement reads single bits
                raise ValueError(f"parse_jpeg: {what}: Huffman table (class {need[0]}, destination {need[1]}) is used and never defined")
            specs.append((huff.get((0, td)), huff.get((1, ta))))
        units = ops.jpeg_scan_units(height, width, key, -1 if ns == nf else idx[0])
        scan, intervals, pos = _entropy_bytes(data, pos, units, ri, what)
        scans.append(JpegScan(idx, Ss, Se, Ah, Al, tuple((td, ta) for _, td, ta in sel), tuple(specs), int(ri), scan, intervals))
        while True:                                                              # the marker segments up to the next SOS, or EOI
            while pos + 1 < len(data) and data[pos] == 0xFF and data[pos + 1] == 0xFF:
                pos += 1
            if pos + 2 > len(data) or data[pos] != 0xFF:
                raise ValueError(f"parse_jpeg: no marker at byte {pos} behind scan {len(scans) - 1}: the file ends or is damaged before its EOI")
            marker = data[pos + 1]
            if marker == 0xD9:
                break
            if pos + 4 > len(data):
                raise ValueError(f"parse_jpeg: the file ends inside marker FF{marker:02X} at byte {pos}")
            size = struct.unpack_from(">H", data, pos + 2)[0]
            body = data[pos + 4:pos + 2 + size]
            if size < 2 or pos + 2 + size > len(data):
                raise ValueError(f"parse_jpeg: segment FF{marker:02X} at byte {pos} runs past the end of the file")
            pos += 2 + size
            if marker == 0xDA:
                break
            if marker == 0xC4:
                while body:
                    if len(body) < 17 or len(body) < 17 + sum(body[1:17]):
                        raise ValueError("parse_jpeg: a DHT segment ends inside a table")
                    bits = tuple(body[1:17])
                    huff[(body[0] >> 4, body[0] & 15)], body = (bits, bytes(body[17:17 + sum(bits)])), body[17 + sum(bits):]
            elif marker == 0xDD:
                if len(body) != 2:
                    raise ValueError("parse_jpeg: a malformed DRI segment")
                ri = struct.unpack(">H", body)[0]
            elif marker == 0xDB:
                while body:
                    if body[0] >> 4 or len(body) < 65:
                        raise ValueError(f"parse_jpeg: a DQT segment behind scan {len(scans) - 1} with 16-bit entries or cut short")
                    nat = np.zeros(64, np.uint16)
                    nat[ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                    tq, body = body[0] & 15, body[65:]
                    if tq in quant and any(c[3] == tq for c in comps) and not np.array_equal(quant[tq], nat):
                        raise ValueError(f"parse_jpeg: a DQT segment behind scan {len(scans) - 1} changes quantisation table {tq}, which the "
                                         "frame uses: libjpeg keeps the table a component had at its first scan; one table per component is built")
                    quant[tq] = nat
            elif marker == 0xDC:
                raise ValueError(f"parse_jpeg: a DNL segment behind scan {len(scans) - 1}: the frame header holds the height here; {_ONLY_PROGRESSIVE}")
            elif marker in (0xC0, 0xC2, 0xD8) or marker in _SOF_NAMES:
                raise ValueError(f"parse_jpeg: marker FF{marker:02X} at byte {pos - 2 - size} behind scan {len(scans) - 1}: a second frame")
        if marker == 0xD9:
            break
    for c in range(nf):
        missing = [k for k in range(64) if known[c][k] is None]
        coarse = [k for k in range(64) if known[c][k]]
        if missing or coarse:
            said = (f"coefficient{'s' if len(missing) != 1 else ''} {missing[0]}{' .. ' + str(missing[-1]) if len(missing) > 1 else ''} of "
                    f"component {ids[c]} never coded") if missing else \
                   f"coefficient {coarse[0]} of component {ids[c]} coded down to Al = {known[c][coarse[0]]} only, not to 0"
            raise ValueError(f"parse_jpeg: the progression is not complete at EOI after {len(scans)} scans: {said}; {_NO_SMOOTHING}")
    return tuple(scans), quant


_ONLY_PROGRESSIVE = ("progressive=True reads 8-bit Huffman-coded progressive (SOF2) files with a complete progression next to baseline ones, "
                     "in the same layouts")


def parse_jpeg(data, restart: bool = False, layouts: bool = False, progressive: bool = False) -> ParsedJpeg:
    """One JPEG file -> ParsedJpeg, walking its marker segments (T.81 Annex B).  A file without DHT segments gets the tables of Annex
    K.3 - K.6 (the Motion-JPEG convention in AVI files).  ValueError, saying what was found, for everything but 8-bit baseline 4:2:0 in
    one interleaved scan without restart intervals: progressive, extended or arithmetic-coded files, other sampling factors, grey
    images, a restart interval, 16-bit quantisers, Cb and Cr on different tables, frames narrower than JPEG_MIN_WIDTH.
    layouts=True (what decode_mjpeg passes) also takes 4:2:2 (2x1 / 1x1 / 1x1), 4:4:4 (1x1 / 1x1 / 1x1) and grey files (one component,
    whose stated factors count as 1x1: T.81 A.2.2), and Cb and Cr on different quantisation tables; ParsedJpeg.layout says which and
    which tables each component uses.  Still refused by name: 4:4:0, 4:1:1 and every other set of factors, four components, Cb and Cr
    on different Huffman tables, and frames narrower than JPEG_MIN_WIDTH where chroma is halved along the rows (4:2:0, 4:2:2 - 4:4:4
    and grey take any width).  With or without the keyword, a three-component file libjpeg would read as RGB rather than YCbCr is
    refused: an Adobe APP14 segment with transform 0, or component ids 'R', 'G', 'B' with neither a JFIF nor an Adobe segment.
    restart=True takes restart intervals too (B.2.4.4, E.1.4): Ri is that of the last DRI segment in front of the scan (0: none), the
    entropy-coded bytes are split at the RSTm markers and every interval is unstuffed; the markers must count 0, 1, .. 7, 0, .. and cut
    the scan into exactly ceil(MCUs / Ri) intervals, anything else is a ValueError that says what was found - a decoder's
    resynchronisation on damaged files is not built, and neither are fill bytes in front of a marker.
    progressive=True (it implies the other two) also takes Huffman-coded progressive files (SOF2, T.81 Annex G) in those layouts and
    walks them to EOI: ParsedJpeg.scans then holds one JpegScan per scan - components, Ss, Se, Ah, Al, the tables its destinations held
    and the restart interval in force AT THAT SCAN (DHT and DRI segments between scans change both; in a one-component scan the
    interval counts that component's blocks), its entropy-coded bytes - and specs / scan / intervals are empty.  Cb and Cr on
    different Huffman tables are fine there.  Refused, saying what was found: a scan outside T.81 G.1.1.1.1 (a DC scan with Se != 0,
    an AC scan over several components or with a band outside Ss .. 63, Al > 13), a first scan with Ah != 0, a refinement whose Ah is
    not the Al before it or whose Al is not Ah - 1, an AC scan in front of its component's DC, a component the frame lacks, a DC scan interleaved over some but not all
    of the frame's components (T.81 allows it; the kernel's table slots take all components or one), scan components listed out of the
    frame's order, a DQT
    behind the first scan that changes a table in use, a DNL segment, and a progression that is NOT COMPLETE at EOI (some coefficient
    never coded, or not down to Al = 0): libjpeg smooths such files between blocks, which is not built.  A baseline file parses as
    without the keyword, with scans None."""
    data = bytes(data)
    if progressive:
        restart = layouts = True
    ri, sof2 = 0, False
    if len(data) < 4 or data[:2] != b"\xFF\xD8":
        raise ValueError("parse_jpeg: no SOI marker at the start: not a JPEG file")
    pos, quant, huff, frame, jfif, adobe = 2, {}, {}, None, False, None
    while True:
        while pos < len(data) and data[pos] == 0xFF and pos + 1 < len(data) and data[pos + 1] == 0xFF:
            pos += 1                                                             # fill bytes (B.1.1.2)
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise ValueError(f"parse_jpeg: no marker at byte {pos}: the file ends or is damaged before its scan")
        marker, size = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        body = data[pos + 4:pos + 2 + size]
        if size < 2 or pos + 2 + size > len(data):
            raise ValueError(f"parse_jpeg: segment FF{marker:02X} at byte {pos} runs past the end of the file")
        pos += 2 + size
        if marker == 0xDB:                                                       # DQT (B.2.4.1)
            while body:
                pq, tq = body[0] >> 4, body[0] & 15
                if pq != 0:
                    raise ValueError(f"parse_jpeg: quantisation table {tq} has 16-bit entries; {_ONLY}")
                if len(body) < 65:
                    raise ValueError("parse_jpeg: a DQT segment ends inside a table")
                nat = np.zeros(64, np.uint16)
                nat[ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                quant[tq], body = nat, body[65:]
        elif marker == 0xC4:                                                     # DHT (B.2.4.2)
            while body:
                if len(body) < 17 or len(body) < 17 + sum(body[1:17]):
                    raise ValueError("parse_jpeg: a DHT segment ends inside a table")
                bits = tuple(body[1:17])
                huff[(body[0] >> 4, body[0] & 15)], body = (bits, bytes(body[17:17 + sum(bits)])), body[17 + sum(bits):]
        elif marker == 0xC0 or (marker == 0xC2 and progressive):                 # SOF0, SOF2 (B.2.2)
            sof2 = marker == 0xC2
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError(f"parse_jpeg: a malformed SOF{2 if sof2 else 0} segment")
            precision, height, width, nf = struct.unpack_from(">BHHB", body, 0)
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)]
            if precision != 8:
                raise ValueError(f"parse_jpeg: {precision}-bit samples; {_ONLY}")
            if nf not in (1, 3) or (nf == 1 and not layouts):
                raise ValueError(f"parse_jpeg: {nf} component{'s' if nf != 1 else ' (a grey image)'}; {_NO_LAYOUTS if nf == 1 else _ONLY}")
            factors = ((1, 1),) if nf == 1 else tuple((h, v) for _, h, v, _ in comps)
            said = "sampling factors " + " / ".join(f"{h}x{v}" for h, v in factors) + _FACTOR_NAMES.get(factors, "")
            if nf == 3 and ((3,) + factors[0] not in ops.JPEG_LAYOUTS or factors[1:] != ((1, 1), (1, 1))):
                raise ValueError(f"parse_jpeg: {said}; {_ONLY}")
            if factors[0] != (2, 2) and not layouts:
                raise ValueError(f"parse_jpeg: {said}; {_NO_LAYOUTS}")
            if height == 0:
                raise ValueError(f"parse_jpeg: the frame header leaves the height to a DNL segment; {_ONLY}")
            if factors[0][0] == 2 and width < JPEG_MIN_WIDTH:
                raise ValueError(f"parse_jpeg: a frame {width} pixels wide at {said}: below {JPEG_MIN_WIDTH} libjpeg replicates chroma samples "
                                 "instead of filtering them, which is not built")
            frame = (height, width, comps, factors)
        elif marker in _SOF_NAMES:
            raise ValueError(f"parse_jpeg: a {_SOF_NAMES[marker]} file; {_ONLY}")
        elif marker == 0xDD:                                                     # DRI (B.2.4.4)
            if len(body) != 2:
                raise ValueError("parse_jpeg: a malformed DRI segment")
            ri = struct.unpack(">H", body)[0]                                    # the last one in front of the scan holds
            if ri and not restart:
                raise ValueError(f"parse_jpeg: a restart interval of {ri} MCUs; restart markers are not built; {_ONLY}")
        elif marker == 0xDA:                                                     # SOS (B.2.3): the scan follows
            break
        elif marker in (0xD8, 0xD9) or 0xD0 <= marker <= 0xD7 or marker == 0x01:
            raise ValueError(f"parse_jpeg: marker FF{marker:02X} at byte {pos - 2 - size} before any scan")
        elif marker == 0xE0 and body[:5] == b"JFIF\0":                           # APP0: JFIF implies YCbCr
            jfif = True
        elif marker == 0xEE and len(body) >= 12 and body[:5] == b"Adobe":        # APP14: the colour transform flag
            adobe = body[11]
        # the other APPn, COM and the rest: skipped
    if frame is None:
        raise ValueError("parse_jpeg: a scan without a frame header in front of it")
    height, width, comps, factors = frame
    nf = len(comps)
    # jdapimin.c default_decompress_parms: which colour space libjpeg takes three components for
    if nf == 3 and adobe == 0:
        raise ValueError("parse_jpeg: an Adobe APP14 segment with transform 0: the three components are RGB, not YCbCr; " + _ONLY)
    if nf == 3 and not jfif and adobe is None and bytes(c[0] for c in comps) == b"RGB":
        raise ValueError("parse_jpeg: neither a JFIF nor an Adobe segment and component ids 'R', 'G', 'B': the three components are RGB, not "
                         "YCbCr; " + _ONLY)
    if sof2:
        if not huff:
            huff = dict(zip(HUFFMAN_IDS, HUFFMAN_SPECS))
        scans, quant = _progressive_scans(data, pos, body, frame, quant, huff, ri)
        quants = np.stack([quant[comps[min(k, nf - 1)][3]] for k in range(3)])
        empty, none = np.zeros(0, np.uint8), np.zeros(2, np.int64)
        for arr in (quants, empty, none):
            arr.setflags(write=False)
        return ParsedJpeg(int(height), int(width), quants, (), empty, scans[0].restart, none, JpegLayout(nf, factors, tuple(c[3] for c in comps), ()),
                          scans)
    if len(body) != 4 + 2 * nf or body[0] != nf:
        raise ValueError(f"parse_jpeg: a scan of {body[0] if body else 0} of the frame's {nf} components (not interleaved); {_ONLY}")
    sel = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(nf)]
    if [c for c, _, _ in sel] != [c[0] for c in comps]:
        raise ValueError(f"parse_jpeg: the scan lists components {[c for c, _, _ in sel]}, the frame {[c[0] for c in comps]}")
    if tuple(body[1 + 2 * nf:]) != (0, 63, 0):
        raise ValueError(f"parse_jpeg: a scan of coefficients {body[1 + 2 * nf]} .. {body[2 + 2 * nf]} with approximation "
                         f"{body[3 + 2 * nf]:#04x} (progressive); {_ONLY}")
    if nf == 3 and sel[1][1:] != sel[2][1:]:
        raise ValueError(f"parse_jpeg: Cb decodes with Huffman tables {sel[1][1:]} and Cr with {sel[2][1:]}; one chrominance pair is built")
    for c in comps:
        if c[3] not in quant:
            raise ValueError(f"parse_jpeg: quantisation table {c[3]} is used and never defined")
    if nf == 3 and not np.array_equal(quant[comps[1][3]], quant[comps[2][3]]) and not layouts:
        raise ValueError(f"parse_jpeg: Cb and Cr use different quantisation tables; one chrominance table is built; {_NO_LAYOUTS}")
    if not huff:
        huff = dict(zip(HUFFMAN_IDS, HUFFMAN_SPECS))                             # no DHT at all: the Motion-JPEG convention
    specs = []
    for key in ((0, sel[0][1]), (1, sel[0][2]), (0, sel[-1][1]), (1, sel[-1][2])):
        if key not in huff:
            raise ValueError(f"parse_jpeg: Huffman table (class {key[0]}, destination {key[1]}) is used and never defined")
        specs.append(huff[key])
    scan, intervals, _ = _entropy_bytes(data, pos, ops.jpeg_mcus(height, width, (nf,) + factors[0]), ri, "the scan", unit="MCUs", restart=restart,
                                        open_end=True)
    quants = np.stack([quant[comps[min(k, nf - 1)][3]] for k in range(3)])
    quants.setflags(write=False)
    layout = JpegLayout(nf, factors, tuple(c[3] for c in comps), tuple((td, ta) for _, td, ta in sel))
    return ParsedJpeg(int(height), int(width), quants, tuple(specs), scan, int(ri), intervals, layout)


@functools.lru_cache(maxsize=16)
def _decode_header(quant_bytes: bytes, specs: tuple) -> np.ndarray:
    """what a group of frames shares, as bytes: the four decoding tables (int32 (4, 320)) and the quantisers (uint16 (3, 64), one per
    component)"""
    tables = np.stack([huffman_decode_table(*spec) for spec in specs])
    return np.concatenate([tables.view(np.uint8).reshape(-1), np.frombuffer(quant_bytes, np.uint8)])


@functools.lru_cache(maxsize=64)
def _decode_table_bytes(spec: tuple) -> bytes:
    return huffman_decode_table(*spec).tobytes()


def _progressive_group_plan(parsed, members, device) -> dict:
    """the progressive frames parsed[i], i in members - one layout, one set of quantisers, one scan script - uploaded in one copy:
    decoding tables (each once), quantisers, the segment tables of every scan, the scans.  -> what _decode_progressive_group runs:
    `launches`, one (JpegScan of the first frame, a function that launches emo_jpeg_progressive_scan for that scan of all frames) per
    scan in file order; `coefs` (not zeroed yet) and `status`, which they fill; `quant`; `seg_frame` / `seg_scan` / `seg_interval`, which
    frame, scan and restart interval a status belongs to"""
    first = parsed[members[0]]
    n, H, W = len(members), first.height, first.width
    layout = first.layout.key
    n_mcu, bpm, nf = first.mcus, ops.jpeg_bpm(layout), first.layout.components
    table_of, table_bytes = {}, []                                               # the decoding tables the group uses, each once

    def table(spec):
        if spec not in table_of:
            table_of[spec] = len(table_bytes)
            table_bytes.append(_decode_table_bytes(spec))
        return table_of[spec]

    seg_offsets, seg_frame, seg_first, seg_units, seg_tables, seg_scan, seg_interval, chunks, launches = [], [], [], [], [], [], [], [], []
    at = n_seg = 0                                                               # bytes and segments so far; the buffers are scan-major
    for k, sc in enumerate(first.scans):
        scan_comp = -1 if len(sc.components) == nf and nf > 1 else sc.components[0]
        units = ops.jpeg_scan_units(H, W, layout, scan_comp)
        seg0 = n_seg
        for f, i in enumerate(members):
            s = parsed[i].scans[k]
            tabs = [0, 0, 0]
            if not (s.Ss == 0 and s.Ah):                                         # a DC refinement reads no table
                for c, pair in enumerate(s.specs):
                    tabs[c] = table(pair[0] if s.Ss == 0 else pair[1])
            n_int = len(s.intervals) - 1
            first_unit = np.arange(n_int, dtype=np.int64) * (s.restart or units)
            seg_offsets.append(at + s.intervals[:-1])
            seg_first.append(first_unit)
            seg_units.append(np.minimum(first_unit + (s.restart or units), units) - first_unit)
            seg_frame.append(np.full(n_int, f, np.int64))
            seg_scan.append(np.full(n_int, k, np.int64))
            seg_interval.append(np.arange(n_int, dtype=np.int64))
            seg_tables.append(np.tile(np.array(tabs, np.int64), (n_int, 1)))
            chunks.append(s.scan)
            at += len(s.scan)
            n_seg += n_int
        launches.append((seg0, n_seg, sc, scan_comp))
    seg_offsets = np.concatenate(seg_offsets + [np.array([at], np.int64)]).astype(np.int64)
    seg_frame, seg_first, seg_units, seg_tables, seg_scan, seg_interval = (np.concatenate(x) for x in (seg_frame, seg_first, seg_units, seg_tables,
                                                                                                       seg_scan, seg_interval))
    quant_bytes = first.quants.tobytes()
    pad = -at % 4 or (4 if at == 0 else 0)
    ints = [x.astype(np.int32).reshape(-1).view(np.uint8) for x in (seg_frame, seg_first, seg_units, seg_tables)]
    host = np.concatenate([np.frombuffer(b"".join(table_bytes), np.uint8), np.frombuffer(quant_bytes, np.uint8), seg_offsets.view(np.uint8)]
                          + ints + chunks + [np.zeros(pad, np.uint8)])
    dev = torch.from_numpy(host).to(device)                                      # the one copy
    t_end = 4 * ops.JPEG_DECODE_TABLE_INTS * len(table_bytes)
    q_end = t_end + len(quant_bytes)
    o_end = q_end + 8 * (n_seg + 1)                                              # every part is a multiple of 8 bytes up to here
    tables = dev[:t_end].view(torch.int32).view(-1, ops.JPEG_DECODE_TABLE_INTS)
    quant = dev[t_end:q_end].view(torch.uint16).view(3, 64)
    d_off = dev[q_end:o_end].view(torch.int64)
    d_frame, d_first, d_units = (dev[o_end + 4 * j * n_seg:o_end + 4 * (j + 1) * n_seg].view(torch.int32) for j in range(3))
    d_tabs = dev[o_end + 12 * n_seg:o_end + 24 * n_seg].view(torch.int32).view(n_seg, 3)
    scans = dev[o_end + 24 * n_seg:]
    coefs = torch.empty(n, n_mcu, bpm, 64, device=device, dtype=torch.int16)
    status = torch.empty(n_seg, device=device, dtype=torch.int32)

    def launch(a, b, sc, scan_comp):
        return lambda: ops.jpeg_progressive_scan(scans, d_off[a:b + 1], d_frame[a:b], d_first[a:b], d_units[a:b], d_tabs[a:b], tables, coefs, H, W,
                                                 layout, sc.Ss, sc.Se, sc.Ah, sc.Al, scan_comp, status=status[a:b])
    return dict(launches=[(sc, launch(a, b, sc, scan_comp)) for a, b, sc, scan_comp in launches], coefs=coefs, status=status, quant=quant,
                seg_frame=seg_frame, seg_scan=seg_scan, seg_interval=seg_interval)


def _coefs_to_frames(coefs, quant, H, W, layout, out, members) -> None:
    """the tail every group shares: emo_jpeg_idct and emo_jpeg_rgb on the group's coefficients, into frames `members` of out - straight
    into out where the group is all of it, else through a tensor of its own, copied as one slice where the members are consecutive and
    scattered by index where they are not"""
    n = len(members)
    whole = n == out.shape[0]
    y, c = ops.jpeg_idct(coefs, quant, H, W, layout)
    rgb = ops.jpeg_rgb(y, c, H, W, layout, out=out if whole else None)
    if whole:
        return
    if members == list(range(members[0], members[0] + n)):
        out[members[0]:members[0] + n] = rgb
    else:
        out[torch.tensor(members, device=out.device)] = rgb


def _decode_progressive_group(parsed, members, out) -> None:
    """_progressive_group_plan's group decoded into its frames of out: the coefficient buffer zeroed once, one emo_jpeg_progressive_scan
    launch per scan of the script in file order, the baseline IDCT and colour launches, one read of every segment's status"""
    first = parsed[members[0]]
    H, W, layout = first.height, first.width, first.layout.key
    plan = _progressive_group_plan(parsed, members, out.device)
    coefs, status, quant, seg_frame, seg_scan, seg_interval = (plan[k] for k in ("coefs", "status", "quant", "seg_frame", "seg_scan", "seg_interval"))
    coefs.zero_()                                                                # once: every scan adds to it
    for _, run in plan["launches"]:                                              # file order on one stream is the only synchronisation
        run()
    _coefs_to_frames(coefs, quant, H, W, layout, out, members)
    st = status.cpu().numpy()                                                    # the one read, for all scans
    if st.any():
        bad = np.flatnonzero(st)
        bad = int(bad[np.lexsort((seg_scan[bad], seg_frame[bad]))[0]])        # the first frame, its first scan: later scans build on it
        f, k = int(seg_frame[bad]), int(seg_scan[bad])
        s = parsed[members[f]].scans[k]
        where = f" in restart interval {int(seg_interval[bad])} of {len(s.intervals) - 1}" if s.restart else ""
        raise ValueError(f"decode_mjpeg: frame {members[f]} does not decode: {ops.JPEG_STATUS.get(int(st[bad]), f'status {int(st[bad])}')} in scan "
                         f"{k} of {len(first.scans)} ({s}){where} (emo_jpeg_progressive_scan status {int(st[bad])})")


def decode_mjpeg(jpegs, device=None, progressive: bool = False) -> torch.Tensor:
    """Baseline JPEG files of one size (bytes each; what encode_mjpeg, Pillow or a Motion-JPEG AVI hold) - 4:2:0, 4:2:2, 4:4:4 or grey,
    mixed freely, with or without restart intervals -> packed uint8 RGB frames (n, H, W, 3) on the device, byte for byte what
    libjpeg's default decoder (Pillow's `Image.open(f).convert("RGB")`) gives; a grey frame comes back with R = G = B.  The host only
    parses markers and takes the stuffed bytes out; frames that share their tables and their layout go up in ONE copy (tables,
    quantisers, the segment table, scans) and through one set of three launches (emo_jpeg_decode_segments, emo_jpeg_idct,
    emo_jpeg_rgb), followed by one read of the segments' status.  A segment is a restart interval, or a whole frame that has none:
    frames with different restart intervals and frames without share a launch, and a frame decodes as many wavefronts wide as it has
    intervals.  (A group in which no frame is cut into intervals goes through emo_jpeg_decode_bits, one workgroup per frame.)
    ValueError naming the frame for a file parse_jpeg refuses, a frame of another size, or a scan that does not decode (naming the
    restart interval too when the frame has them).  There is no host decoder behind this.
    progressive=True also takes Huffman-coded progressive files (SOF2) with a complete progression, mixed freely with baseline ones
    (parse_jpeg(progressive=True) says what is refused).  Progressive frames that share layout, quantisers and scan script - the
    (components, Ss, Se, Ah, Al) of every scan; Huffman tables and restart intervals may differ from frame to frame - go up in one copy
    too; their coefficient buffer is zeroed once and filled by ONE emo_jpeg_progressive_scan launch per scan of the script, in file
    order, before the same IDCT and colour launches, and the status of every segment of every scan is read once.  An error names the
    frame, the scan (its number, Ss .. Se, Ah / Al) and the restart interval where the scan has them."""
    jpegs = list(jpegs)
    if not jpegs:
        raise ValueError("decode_mjpeg: no frames")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ops._lib.EmoHipError(f"decode_mjpeg decodes on the HIP device, got device {device} (there is no host decoder here; "
                                   "video2images keeps Pillow's)")
    parsed = []
    for i, j in enumerate(jpegs):
        try:
            parsed.append(parse_jpeg(j, restart=True, layouts=True, progressive=progressive))
        except ValueError as e:
            raise ValueError(f"decode_mjpeg: frame {i}: {e}") from None
    H, W = parsed[0].height, parsed[0].width
    for i, p in enumerate(parsed):
        if (p.height, p.width) != (H, W):
            raise ValueError(f"decode_mjpeg: frame {i} is {p.height} x {p.width}, frame 0 is {H} x {W}: the frames of a clip share one size")
    groups = {}
    for i, p in enumerate(parsed):
        groups.setdefault(p.table_key(), []).append(i)
    out = torch.empty(len(parsed), H, W, 3, device=device, dtype=torch.uint8)
    for key, members in groups.items():
        n = len(members)
        if parsed[members[0]].scans is not None:
            _decode_progressive_group(parsed, members, out)
            continue
        head = _decode_header(*key[:2])
        layout = parsed[members[0]].layout.key
        n_mcu, bpm = parsed[members[0]].mcus, ops.jpeg_bpm(layout)
        # the segment table: one segment per restart interval, one for a frame without; frame f of the group owns blocks f * n_mcu * bpm ..
        sizes = np.array([len(parsed[i].scan) for i in members], np.int64)
        frame_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        seg_offsets, seg_first, seg_blocks, seg_frame = [], [], [], []
        for f, i in enumerate(members):
            p = parsed[i]
            first_mcu = np.arange(len(p.intervals) - 1, dtype=np.int64) * (p.restart or n_mcu)
            seg_offsets.append(frame_start[f] + p.intervals[:-1])
            seg_first.append((f * n_mcu + first_mcu) * bpm)
            seg_blocks.append((np.minimum(first_mcu + (p.restart or n_mcu), n_mcu) - first_mcu) * bpm)
            seg_frame.append(np.full(len(first_mcu), f, np.int64))
        seg_offsets = np.concatenate(seg_offsets + [frame_start[-1:]]).astype(np.int64)
        seg_first, seg_blocks, seg_frame = (np.concatenate(x) for x in (seg_first, seg_blocks, seg_frame))
        n_seg = len(seg_first)
        pad = -int(frame_start[-1]) % 4 or (4 if frame_start[-1] == 0 else 0)
        host = np.concatenate([head, seg_offsets.view(np.uint8), seg_first.astype(np.int32).view(np.uint8), seg_blocks.astype(np.int32).view(np.uint8)]
                              + [parsed[i].scan for i in members] + [np.zeros(pad, np.uint8)])
        dev = torch.from_numpy(host).to(device)                                  # the one copy
        t_end, q_end = 16 * ops.JPEG_DECODE_TABLE_INTS, len(head)
        o_end = q_end + 8 * (n_seg + 1)                                          # head is t_end + 384 bytes: every table stays 8-byte aligned
        tables = dev[:t_end].view(torch.int32).view(4, ops.JPEG_DECODE_TABLE_INTS)
        quant = dev[t_end:q_end].view(torch.uint16).view(3, 64)
        scans, seg_off = dev[o_end + 8 * n_seg:], dev[q_end:o_end].view(torch.int64)
        if n_seg > n:
            seg_tabs = dev[o_end:o_end + 4 * n_seg].view(torch.int32), dev[o_end + 4 * n_seg:o_end + 8 * n_seg].view(torch.int32)
            entry = "emo_jpeg_decode_segments"
            coefs, status = ops.jpeg_decode_segments(scans, seg_off, *seg_tabs, tables, n, n_mcu, layout)
        else:               # no frame of the group is cut into intervals: a segment is a frame, which a workgroup of its own decodes faster
            entry = "emo_jpeg_decode_bits"
            coefs, status = ops.jpeg_decode_bits(scans, seg_off, tables, n_mcu, layout)
        _coefs_to_frames(coefs, quant, H, W, layout, out, members)
        st = status.cpu().numpy()                                                # the one read
        if st.any():
            bad = int(np.flatnonzero(st)[0])                                     # the first in frame order, whichever wave ended first
            f = int(seg_frame[bad])
            p = parsed[members[f]]
            where = f" in restart interval {bad - int(np.searchsorted(seg_frame, f))} of {len(p.intervals) - 1}" if p.restart else ""
            raise ValueError(f"decode_mjpeg: frame {members[f]} does not decode: {ops.JPEG_STATUS.get(int(st[bad]), f'status {int(st[bad])}')}"
                             f"{where} ({entry} status {int(st[bad])})")
    return out


# ---------------------------------------------------------------------------------------------------------------------- resizing
RESIZE_PRECISION_BITS = 22      # Resample.c PRECISION_BITS = 32 - 8 - 2: the fixed point of the coefficients of 8-bit images


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


# Resample.c writes the two constants of its Hamming window as single-precision literals (0.54f, 0.46f) inside a double expression: the
# doubles 0.54 and 0.46 give coefficients one unit off in a few rows (seen at 1080 -> 512)
_HAMMING_A, _HAMMING_B = float(np.float32(0.54)), float(np.float32(0.46))


def _hamming(x):
    import math
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x *= math.pi
    return math.sin(x) / x * (_HAMMING_A + _HAMMING_B * math.cos(x))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    import math
    if x == 0.0:
        return 1.0
    x *= math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


RESIZE_FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0),
                  "lanczos": (_lanczos, 3.0)}                      # name -> (filter, support), Resample.c


def _resize_filter(resample):
    if not isinstance(resample, str) or resample.lower() not in RESIZE_FILTERS:
        what = "nearest-neighbour resizing is not built: " if isinstance(resample, str) and resample.lower() == "nearest" else ""
        raise ValueError(f"{what}resample= takes one of {', '.join(map(repr, RESIZE_FILTERS))} (\"bicubic\" is what Image.resize does when "
                         f"it is given no filter), got {resample!r}")
    return resample.lower()


@functools.lru_cache(maxsize=64)
def _resize_taps(in_size: int, out_size: int, name: str):
    filt, filter_support = RESIZE_FILTERS[name]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filter_support * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    bounds, coef = np.zeros((out_size, 2), np.int32), np.zeros((out_size, ksize), np.int32)
    one = float(1 << RESIZE_PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) / filterscale) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = xmin, xmax
        coef[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def resize_taps(in_size: int, out_size: int, filter: str = "bicubic"):
    """The table of one axis of `Image.resize` for 8-bit images, as Pillow's Resample.c builds it (precompute_coeffs,
    normalize_coeffs_8bpc), in Python doubles: (bounds int32 (out_size, 2) = (first input index, tap count), coef int32 (out_size, ksize),
    22-bit fixed point, zero behind the taps).  With scale = in / out and filterscale = max(scale, 1): support = the filter's support *
    filterscale, ksize = ceil(support) * 2 + 1; output xx is centred at (xx + 0.5) * scale, takes the inputs xmin = max(int(center -
    support + 0.5), 0) up to min(int(center + support + 0.5), in) with weights filter((x + xmin - center + 0.5) / filterscale) divided by
    their sum, each rounded half away from zero to 1 / 2^22.  Cached per (in_size, out_size, filter); the arrays are read-only.
    filter: "box", "bilinear", "hamming", "bicubic" (a = -0.5) or "lanczos"; "nearest" is not built."""
    name = _resize_filter(filter)
    if any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 1 for s in (in_size, out_size)):
        raise ValueError(f"resize_taps: sizes are positive ints, got {in_size!r} -> {out_size!r}")
    return _resize_taps(int(in_size), int(out_size), name)


@functools.lru_cache(maxsize=16)
def _device_resize_taps(in_size: int, out_size: int, name: str, device: str):
    return tuple(torch.from_numpy(t.copy()).to(device) for t in _resize_taps(in_size, out_size, name))


def _resize_size(size, who):
    if (not isinstance(size, (tuple, list)) or len(size) != 2
            or any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 1 for s in size)):
        raise ValueError(f"{who}: size=(width, height), two positive ints as Image.resize takes them, got {size!r}")
    return int(size[0]), int(size[1])


def resize_frames(frames_u8, size, resample="bicubic", box=None, reducing_gap=None) -> torch.Tensor:
    """`Image.fromarray(f).resize(size, resample)` of every frame, on the device and byte for byte (ops.image_resize): uint8 RGB frames
    (n, H, W, 3) or one frame (H, W, 3), a device tensor or a host array (which is uploaded) -> the same rank at size=(width, height),
    on the device.  resample: a filter of RESIZE_FILTERS; Image.resize without a filter is "bicubic".  Image.resize's box= and
    reducing_gap= are not built."""
    if box is not None or reducing_gap is not None:
        raise ValueError("resize_frames: box= (resizing a region of the frame) and reducing_gap= (a draft reduction in front of the resize) "
                         "are not built: crop the frames first, and expect the one-step resize")
    name = _resize_filter(resample)
    width, height = _resize_size(size, "resize_frames")
    x = frames_u8 if torch.is_tensor(frames_u8) else torch.from_numpy(np.ascontiguousarray(frames_u8))
    if x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-1] != 3 or 0 in x.shape:
        raise ValueError(f"resize_frames takes packed uint8 RGB frames, (n, H, W, 3) or (H, W, 3), got {x.dtype} {tuple(x.shape)}")
    if not x.is_cuda:
        x = x.to("cuda")
    single = x.dim() == 3
    x = (x[None] if single else x).contiguous()
    H, W, dev = int(x.shape[1]), int(x.shape[2]), str(x.device)
    out = ops.image_resize(x, height, width, None if W == width else _device_resize_taps(W, width, name, dev),
                           None if H == height else _device_resize_taps(H, height, name, dev))
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------------------------- AVI container
AVI_MAX_BYTES = 2 ** 31 - 1
AVIF_HASINDEX, AVIF_ISINTERLEAVED, AVIIF_KEYFRAME = 0x10, 0x100, 0x10


def fps_fraction(fps) -> Fraction:
    """an int, a Fraction or a (num, den) pair -> a positive Fraction whose terms fit dwRate / dwScale"""
    if isinstance(fps, (tuple, list)):
        if len(fps) != 2:
            raise ValueError(f"fps: a pair is (numerator, denominator), got {fps!r}")
        f = Fraction(int(fps[0]), int(fps[1]))
    elif isinstance(fps, bool) or not isinstance(fps, (int, np.integer, Fraction)):
        raise ValueError(f"fps is an int, a Fraction or a (numerator, denominator) pair, got {fps!r}")
    else:
        f = Fraction(fps)
    if f <= 0 or f.numerator >= 2 ** 32 or f.denominator >= 2 ** 32:
        raise ValueError(f"fps must be positive with terms below 2^32, got {fps!r}")
    return f


def pcm16(samples) -> np.ndarray:
    """float samples (n,) or (n, channels) -> int16 (n, channels): round(clip(x, -1, 1) * 32767)"""
    x = samples.detach().cpu().numpy() if torch.is_tensor(samples) else np.asarray(samples)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError(f"audio samples are (n,) or (n, channels), got {x.shape}")
    return np.rint(np.clip(x.astype(np.float64), -1.0, 1.0) * 32767.0).astype("<i2")


def _chunk(cid: bytes, body: bytes) -> bytes:
    return cid + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")


def avi_container(jpegs, width: int, height: int, fps, audio=None) -> bytes:
    """JPEG frames (bytes each) -> a RIFF `AVI ` file as bytes: one vids / MJPG stream at fps = dwRate / dwScale and, with
    audio=(float samples (n,) | (n, channels), rate), one auds stream of 16-bit PCM.  movi holds, per frame, the 00dc chunk followed by
    the 01wb chunk of that frame's samples: sample boundaries are round(i * rate / fps), so no sample is lost or repeated, and whatever
    the audio has beyond the last frame goes with the last frame.  ValueError when the file would pass 2^31 - 1 bytes."""
    jpegs = [bytes(j) for j in jpegs]
    f = fps_fraction(fps)
    n = len(jpegs)
    if n < 1 or not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
        raise ValueError(f"write_avi: {n} frames of {width} x {height}")
    pcm = rate = None
    if audio is not None:
        pcm, rate = pcm16(audio[0]), int(audio[1])
        if rate < 1:
            raise ValueError(f"write_avi: audio rate {rate}")
        channels, align = pcm.shape[1], 2 * pcm.shape[1]
        cut = [min((2 * i * rate * f.denominator + f.numerator) // (2 * f.numerator), len(pcm)) for i in range(n)] + [len(pcm)]
    largest = max(len(j) for j in jpegs)
    movi_size = 4 + sum(8 + len(j) + (len(j) & 1) for j in jpegs)
    n_wb = 0
    if pcm is not None:
        n_wb = sum(1 for i in range(n) if cut[i + 1] > cut[i])
        movi_size += 8 * n_wb + align * len(pcm)                                 # 2-byte samples: no pad bytes
    hdrl_size = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40)) + (0 if pcm is None else 12 + (8 + 56) + (8 + 18))
    idx_size = 16 * (n + n_wb)
    total = 12 + (8 + hdrl_size) + (8 + movi_size) + (8 + idx_size)
    if total > AVI_MAX_BYTES:
        raise ValueError(f"write_avi: the file would be {total} bytes; a classic AVI file ends at 2^31 - 1 = {AVI_MAX_BYTES} (OpenDML is not written): "
                         "write shorter clips or lower the quality")
    usec = (1000000 * f.denominator * 2 + f.numerator) // (2 * f.numerator)
    per_sec = int(sum(len(j) for j in jpegs) * f / n) + (0 if pcm is None else rate * align)
    avih = struct.pack("<14I", usec, min(per_sec, 2 ** 32 - 1), 0, AVIF_HASINDEX | AVIF_ISINTERLEAVED, n, 0, 1 if pcm is None else 2, largest,
                       int(width), int(height), 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, f.denominator, f.numerator, 0, n, largest, 0xFFFFFFFF, 0,
                         0, 0, int(width), int(height))
    strf_v = struct.pack("<IiiHH4sIiiII", 40, int(width), int(height), 1, 24, b"MJPG", int(width) * int(height) * 3, 0, 0, 0, 0)
    hdrl = b"hdrl" + _chunk(b"avih", avih) + b"LIST" + struct.pack("<I", 4 + 8 + 56 + 8 + 40) + b"strl" + _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v)
    if pcm is not None:
        strh_a = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\x00\x00\x00\x00", 0, 0, 0, 0, 1, rate, 0, len(pcm),
                             max(cut[i + 1] - cut[i] for i in range(n)) * align, 0xFFFFFFFF, align, 0, 0, 0, 0)
        strf_a = struct.pack("<HHIIHHH", 1, channels, rate, rate * align, align, 16, 0)
        hdrl += b"LIST" + struct.pack("<I", 4 + 8 + 56 + 8 + 18) + b"strl" + _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a)
    assert len(hdrl) == hdrl_size, (len(hdrl), hdrl_size)
    movi, index, pos = [b"movi"], [], 4                                          # idx1 offsets count from the `movi` fourcc
    for i, j in enumerate(jpegs):
        c = _chunk(b"00dc", j)
        index.append(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, pos, len(j)))
        movi.append(c)
        pos += len(c)
        if pcm is not None and cut[i + 1] > cut[i]:
            body = pcm[cut[i]:cut[i + 1]].tobytes()
            c = _chunk(b"01wb", body)
            index.append(struct.pack("<4sIII", b"01wb", AVIIF_KEYFRAME, pos, len(body)))
            movi.append(c)
            pos += len(c)
    assert pos == movi_size, (pos, movi_size)
    body = b"AVI " + b"LIST" + struct.pack("<I", hdrl_size) + hdrl + b"LIST" + struct.pack("<I", movi_size) + b"".join(movi) + _chunk(b"idx1", b"".join(index))
    assert len(body) + 8 == total, (len(body) + 8, total)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def write_avi(path, jpegs, width: int, height: int, fps, audio=None) -> None:
    """avi_container into the file at path"""
    _write_file(path, avi_container(jpegs, width, height, fps, audio=audio))


def _chunks(raw: bytes, pos: int, end: int):
    """(id, body start, size) of the chunks in raw[pos:end]"""
    while pos + 8 <= end:
        cid, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        if pos + 8 + size > end:
            raise ValueError(f"read_avi: chunk {cid!r} at {pos} runs past its parent")
        yield cid, pos + 8, size
        pos += 8 + size + (size & 1)


def read_avi(path):
    """A file write_avi made -> (jpegs list[bytes], fps Fraction, audio): audio is None or (int16 samples (n, channels), rate) - the
    stored PCM, undivided.  Anything else (another codec, OpenDML, more streams) is a ValueError."""
    with open(os.fspath(path), "rb") as fh:
        raw = fh.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"AVI " or struct.unpack_from("<I", raw, 4)[0] + 8 != len(raw):
        raise ValueError(f"read_avi: {path!r} is not a RIFF AVI file of the size its header states")
    top = {}
    for cid, body, size in _chunks(raw, 12, len(raw)):
        key = raw[body:body + 4] if cid == b"LIST" else cid
        if cid == b"LIST" and size < 4 or key in top:
            raise ValueError(f"read_avi: unexpected chunk {key!r}")
        top[key] = (body, size)
    if set(top) != {b"hdrl", b"movi", b"idx1"}:
        raise ValueError(f"read_avi: expected hdrl, movi and idx1, found {sorted(top)}")
    streams = []
    for cid, body, size in _chunks(raw, top[b"hdrl"][0] + 4, sum(top[b"hdrl"])):
        if cid == b"LIST" and raw[body:body + 4] == b"strl":
            parts = {c: raw[b:b + s] for c, b, s in _chunks(raw, body + 4, body + size)}
            if set(parts) != {b"strh", b"strf"} or len(parts[b"strh"]) != 56:
                raise ValueError("read_avi: a stream list without strh + strf")
            streams.append(parts)
        elif cid != b"avih":
            raise ValueError(f"read_avi: unexpected chunk {cid!r} in hdrl")
    if not 1 <= len(streams) <= 2 or streams[0][b"strh"][:8] != b"vidsMJPG" or streams[0][b"strf"][16:20] != b"MJPG":
        raise ValueError("read_avi: the first stream is not Motion-JPEG video")
    scale, rate_v, _, n_frames = struct.unpack_from("<4I", streams[0][b"strh"], 20)
    if scale < 1 or rate_v < 1:
        raise ValueError(f"read_avi: dwRate / dwScale = {rate_v} / {scale}")
    audio_fmt = None
    if len(streams) == 2:
        if streams[1][b"strh"][:4] != b"auds" or len(streams[1][b"strf"]) < 16:
            raise ValueError("read_avi: the second stream is not audio")
        tag, channels, rate_a, _, align, bits = struct.unpack_from("<HHIIHH", streams[1][b"strf"], 0)
        if tag != 1 or bits != 16 or channels < 1 or align != 2 * channels:
            raise ValueError(f"read_avi: audio format tag {tag} with {bits} bits is not 16-bit PCM")
        audio_fmt = (channels, rate_a)
    jpegs, pcm = [], []
    for cid, body, size in _chunks(raw, top[b"movi"][0] + 4, sum(top[b"movi"])):
        if cid == b"00dc":
            jpegs.append(raw[body:body + size])
        elif cid == b"01wb" and audio_fmt is not None:
            pcm.append(raw[body:body + size])
        else:
            raise ValueError(f"read_avi: unexpected chunk {cid!r} in movi")
    if len(jpegs) != n_frames:
        raise ValueError(f"read_avi: the header counts {n_frames} frames, movi holds {len(jpegs)}")
    audio = None
    if audio_fmt is not None:
        audio = (np.frombuffer(b"".join(pcm), dtype="<i2").reshape(-1, audio_fmt[0]).copy(), audio_fmt[1])
    return jpegs, Fraction(rate_v, scale), audio


# ---------------------------------------------------------------------------------------------------------------------- animated GIF
GIF_STRIP_ROWS = 8      # rows per independently coded strip: the payload stays near the single-stream size (profiles/gif_encode.md)
GIF_OPTIONS = ("loop", "colors", "palette", "dither", "dither_strength", "strip_rows")


def _int_in(value, lo, hi, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{what} takes an int from {lo} to {hi}, got {value!r}")
    return int(value)


def gif_delays(fps, n) -> list:
    """The delay of each of n frames in centiseconds (GIF89a section 23, Delay Time), d_i = r(100 (i + 1) / fps) - r(100 i / fps) with r
    rounding halves up, in exact fractions: the delays add up to the clip's duration rounded once (30 fps: 3, 4, 3, 3, 4, ... , 100 for
    30 frames).  fps as fps_fraction takes it.  ValueError when a delay falls below 2: players show such frames at 10, so a rate above
    50 cannot be kept; and when one passes 65535."""
    f = fps_fraction(fps)
    n = _int_in(n, 1, 2 ** 31 - 1, "gif_delays: the number of frames")
    at = [(200 * i * f.denominator + f.numerator) // (2 * f.numerator) for i in range(n + 1)]
    delays = [b - a for a, b in zip(at, at[1:])]
    if min(delays) < 2 or max(delays) > 65535:
        raise ValueError(f"a GIF frame is shown for 2 .. 65535 hundredths of a second (players show shorter delays as 10): fps = {f} gives "
                         f"delays of {min(delays)} .. {max(delays)}; at most 50 frames per second can be kept")
    return delays


def median_cut(hist, colors: int = 256):
    """A histogram as emo_gif_histogram makes it - (32768, 4) integers: per bin (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3) the pixel count
    and the sums of R, G, B - -> (palette uint8 (k, 3), k), k <= colors.  All pixels start in one box.  While there are fewer than
    `colors` boxes, the box with the MOST PIXELS among those that hold at least two occupied bins is split (the box made first on a tie)
    along the axis on which its occupied bins span the most bin steps (R before G before B on a tie), between two bin coordinates: at
    the first coordinate t at which the bins up to t hold at least half of the box's pixels, one lower where that would leave the upper
    part empty.  The lower part keeps the box's place, the upper part goes to the end of the list.  It stops early when no box can be
    split, so k may be below `colors` (one colour bin: k = 1).  Entry i is the mean colour of box i from the sums, each channel rounded
    half up - not the centre of its bins.  Integer arithmetic throughout: the same histogram gives the same palette everywhere."""
    colors = _int_in(colors, 2, 256, "colors=")
    h = np.asarray(hist)
    if h.shape != (32768, 4) or h.dtype.kind not in "iu":
        raise ValueError(f"median_cut takes an integer histogram (32768, 4), got {h.dtype} {h.shape}")
    h = h.astype(np.int64)
    occ = np.flatnonzero(h[:, 0] > 0)
    if occ.size == 0:
        raise ValueError("median_cut: the histogram counts no pixels")
    coords = np.stack([occ >> 10, (occ >> 5) & 31, occ & 31], axis=1)
    count, sums = h[occ, 0], h[occ, 1:]
    boxes = [np.arange(occ.size)]
    pixels, sizes = np.zeros(colors, np.int64), np.zeros(colors, np.int64)       # per box: its pixels, its occupied bins
    pixels[0], sizes[0] = count.sum(), occ.size
    while len(boxes) < colors:
        pick = int(np.argmax(np.where(sizes >= 2, pixels, -1)))                   # argmax keeps the first of equals
        if sizes[pick] < 2:
            break
        box = boxes[pick]
        c = coords[box]
        lo, hi = c.min(axis=0), c.max(axis=0)
        axis = int(np.argmax(hi - lo))                                           # the first of equal extents
        v = c[:, axis]
        if pixels[pick] < 2 ** 53:                                               # bincount sums in float64: whole numbers below 2^53, exact
            per = np.bincount(v - lo[axis], weights=count[box], minlength=int(hi[axis] - lo[axis]) + 1).astype(np.int64)
        else:
            per = np.zeros(int(hi[axis] - lo[axis]) + 1, np.int64)
            np.add.at(per, v - lo[axis], count[box])
        t = int(lo[axis]) + int(np.searchsorted(np.cumsum(per) * 2, pixels[pick], side="left"))
        t = min(t, int(hi[axis]) - 1)
        low, high = box[v <= t], box[v > t]
        new = len(boxes)
        boxes[pick] = low
        boxes.append(high)
        pixels[pick], sizes[pick], pixels[new], sizes[new] = count[low].sum(), low.size, count[high].sum(), high.size
    palette = np.zeros((len(boxes), 3), np.uint8)
    for i, box in enumerate(boxes):
        palette[i] = (2 * sums[box].sum(axis=0) + int(pixels[i])) // (2 * int(pixels[i]))
    return palette, len(boxes)


def _gif_quantize_options(colors, palette, dither, dither_strength):
    colors = _int_in(colors, 2, 256, "colors=")
    if palette not in ("global", "frame"):
        raise ValueError(f"palette= takes \"global\" (one colour table for the clip) or \"frame\" (one per frame), got {palette!r}")
    if dither not in (None, "bayer"):
        raise ValueError(f"dither= takes None or \"bayer\" (the 8x8 ordered dither), got {dither!r}")
    strength = _int_in(dither_strength, 1, 128, "dither_strength=")
    return colors, palette, strength if dither == "bayer" else 0


def quantize_frames(frames_u8: torch.Tensor, colors: int = 256, palette: str = "global", dither=None, dither_strength: int = 32):
    """Packed uint8 RGB device frames (n, H, W, 3) -> (indices uint8 (n, H, W) on the device, palettes uint8 numpy (1, 256, 3) for
    palette="global" or (n, 256, 3) for "frame", n_colors): emo_gif_histogram, one read of the histogram (512 KiB of counts and sums as
    64-bit figures: 1 MiB per table), median_cut on the host, emo_gif_map.  n_colors is the number of entries in use - an int for
    "global", a tuple of n ints for "frame"; the entries behind them are zero and never indexed.  Every pixel gets the nearest entry
    of its table (squared distance on the 8-bit values, the lowest index on a tie), after the ordered dither when dither="bayer":
    v + floor((2 B8[y & 7][x & 7] - 63) * dither_strength / 128) clamped to 0 .. 255, dither_strength 1 .. 128."""
    colors, palette, strength = _gif_quantize_options(colors, palette, dither, dither_strength)
    frames_u8 = _frames_u8(frames_u8, "quantize_frames", limit=("GIF", 65535)).contiguous()
    n = int(frames_u8.shape[0])
    hist = ops.gif_histogram(frames_u8, per_frame=palette == "frame").cpu().numpy()
    palettes = np.zeros((hist.shape[0], 256, 3), np.uint8)
    used = []
    for i in range(hist.shape[0]):
        entries, k = median_cut(hist[i], colors)
        palettes[i, :k] = entries
        used.append(k)
    device_palettes = torch.from_numpy(palettes).to(frames_u8.device)
    if len(set(used)) == 1:
        indices = ops.gif_map(frames_u8, device_palettes, used[0], strength)
    else:                                                                        # tables of different sizes: one launch per frame
        indices = torch.cat([ops.gif_map(frames_u8[i:i + 1], device_palettes[i:i + 1], used[i], strength) for i in range(n)])
    return indices, palettes, (used[0] if palette == "global" else tuple(used))


def _gif_strip_rows(strip_rows, height):
    return int(height) if strip_rows is None else _int_in(strip_rows, 1, 65535, "strip_rows= (None: the frame as one stream)")


def _gif_check(loop=0, colors=256, palette="global", dither=None, dither_strength=32, strip_rows=GIF_STRIP_ROWS, prefix=""):
    """the values of a GIF's options (prefix: how the caller spells loop=), before any launch"""
    _int_in(loop, 0, 65535, f"{prefix}loop= (0: forever)")
    _gif_quantize_options(colors, palette, dither, dither_strength)
    _gif_strip_rows(strip_rows, 1)


def gif_code_streams(indices: torch.Tensor, strip_rows=GIF_STRIP_ROWS):
    """The device part of the LZW coding: palette indices uint8 (n, H, W) on the device -> (streams uint8 device buffer, byte start of
    every frame, bytes of every frame); two launches and one read of the n frame totals between them.  Every frame starts on a byte;
    inside a frame the strips follow each other bit by bit."""
    rows = _gif_strip_rows(strip_rows, indices.shape[1])
    codes, n_codes, bits = ops.gif_lzw_count(indices, rows)
    offsets, starts, nbytes, out, _ = _stream_layout(bits)                       # the one read before the streams themselves
    ops.gif_lzw_emit(codes, n_codes, offsets, out, int(indices.shape[1]), int(indices.shape[2]), rows)
    return out, starts, nbytes


def gif_sub_blocks(stream) -> bytes:
    """image data -> data sub-blocks (GIF89a section 15): a size byte of 1 .. 255 in front of every 255 bytes, a block terminator behind"""
    a = np.frombuffer(stream, np.uint8) if isinstance(stream, (bytes, bytearray)) else np.asarray(stream, np.uint8)
    at = np.arange(0, len(a), 255)
    sizes = np.minimum(len(a) - at, 255).astype(np.uint8)
    return np.insert(a, at, sizes).tobytes() + b"\x00"


def gif_container(width: int, height: int, palettes: np.ndarray, streams, delays, loop: int = 0) -> bytes:
    """The file around the frames' LZW streams (bytes or uint8 arrays, code size 8): header `GIF89a`, logical screen descriptor (section
    18) with a 256-entry global colour table (19) - palettes[0] -, the NETSCAPE2.0 application extension (26) with the loop count
    (0: forever), and per frame a graphic control extension (23: disposal 1, no transparency, the delay), an image descriptor (20) for
    the whole frame - with a 256-entry local colour table (21) when palettes holds one table per frame -, the code size and the
    sub-blocks; the trailer (27)."""
    palettes = np.asarray(palettes)
    n = len(streams)
    if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
        raise ValueError(f"a GIF frame is 1 .. 65535 pixels each way, got {height} x {width}")
    loop = _int_in(loop, 0, 65535, "loop= (0: forever)")
    if palettes.dtype != np.uint8 or palettes.ndim != 3 or palettes.shape[1:] != (256, 3) or palettes.shape[0] not in (1, n) or len(delays) != n or n < 1:
        raise ValueError(f"gif_container: {n} frames, {len(delays)} delays, colour tables {palettes.dtype} {palettes.shape} (uint8 (1 | n, 256, 3))")
    local = palettes.shape[0] == n and n > 1
    out = [b"GIF89a", struct.pack("<HHBBB", int(width), int(height), 0xF7, 0, 0), palettes[0].tobytes(),
           b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"]
    for i in range(n):
        out.append(b"\x21\xF9\x04\x04" + struct.pack("<H", _int_in(delays[i], 0, 65535, "a frame's delay")) + b"\x00\x00")
        out.append(b"\x2C" + struct.pack("<HHHHB", 0, 0, int(width), int(height), 0x87 if local else 0x00))
        if local:
            out.append(palettes[i].tobytes())
        out.append(b"\x08" + gif_sub_blocks(streams[i]))
    out.append(b"\x3B")
    return b"".join(out)


def encode_gif(frames_u8: torch.Tensor, fps, loop: int = 0, colors: int = 256, palette: str = "global", dither=None, dither_strength: int = 32,
               strip_rows=GIF_STRIP_ROWS) -> bytes:
    """Packed uint8 RGB frames on the device, (n, H, W, 3) (or the (1, n, H, W, 3) of output_type="uint8") -> an animated GIF89a file
    as bytes, playing at fps (gif_delays: at most 50) and repeating `loop` times (0: forever).  quantize_frames picks the colours
    (colors=2 .. 256; palette="global": one table for the clip, "frame": a local table per frame, the global one then holds frame 0's;
    dither=None | "bayer" at dither_strength=1 .. 128) and maps the pixels on the device; the LZW coding runs there too, every frame
    cut into strips of strip_rows rows that are coded independently between Clear codes (None: one stream per frame), and the code
    streams come back in one copy.  Every frame is a whole frame: no differences between frames, no transparency.  All arguments are
    checked before the first launch."""
    frames_u8 = _frames_u8(frames_u8, "encode_gif", limit=("GIF", 65535))
    n, height, width = (int(s) for s in frames_u8.shape[:3])
    delays = gif_delays(fps, n)
    _gif_check(loop, colors, palette, dither, dither_strength, strip_rows)
    indices, palettes, _ = quantize_frames(frames_u8, colors, palette, dither, dither_strength)
    out, starts, nbytes = gif_code_streams(indices, strip_rows)
    host = out.cpu().numpy()
    return gif_container(width, height, palettes, [host[s:s + b] for s, b in zip(starts, nbytes)], delays, loop)


def write_gif(frames_u8: torch.Tensor, path, fps, **options) -> None:
    """encode_gif (with its options) into the `.gif` file at path"""
    _write_clip("write_gif", lambda: frames_u8, path, fps, FORMATS["gif"], None, options)


# ---------------------------------------------------------------------------------------------------------------------- PNG / APNG
PNG_STRIP_ROWS = 1      # scanlines per independently tokenised strip: one row gave the smallest files AND the shortest walk (profiles/png_encode.md)
PNG_OPTIONS = ("filter", "strip_rows", "loop")
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_COLOUR_TYPES = {1: 0, 3: 2, 4: 6}      # channels -> IHDR colour type: grey, RGB, RGBA
ADLER = 65521
DEFLATE_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)      # RFC 1951 3.2.7
# extra bits behind every slot of the device's histogram (RFC 1951 3.2.5): length symbols 265 .. 284, distance symbols 4 .. 29 at 288 +
DEFLATE_EXTRA_BITS = np.zeros(ops.PNG_SYMBOLS, np.int64)
DEFLATE_EXTRA_BITS[265:285] = (np.arange(265, 285) - 261) // 4
DEFLATE_EXTRA_BITS[288 + 4:288 + 30] = np.arange(4, 30) // 2 - 1
DEFLATE_EXTRA_BITS.setflags(write=False)


def huffman_code_lengths(freq, limit: int, complete: bool = False) -> list:
    """Code lengths of at most `limit` bits for the symbols with freq > 0 (0 for the others) that minimise sum(freq * length): a plain
    Huffman tree where its deepest leaf fits, else package-merge (Larmore / Hirschberg), which is optimal under the limit.  Two or more
    used symbols always give a complete code (Kraft sum exactly 1).  One used symbol gets length 1, no used symbol no code at all (RFC
    1951 3.2.7 for the distance alphabet); complete=True - the code-length alphabet, which inflate wants complete - then gives a second,
    unused symbol length 1 too.  Ties are broken by symbol index, so the same histogram gives the same lengths everywhere."""
    import heapq
    freq = [int(f) for f in freq]
    used = [i for i, f in enumerate(freq) if f > 0]
    lengths = [0] * len(freq)
    if len(used) > (1 << limit):
        raise ValueError(f"{len(used)} symbols do not fit codes of {limit} bits")
    if len(used) < 2:
        for i in used:
            lengths[i] = 1
        for i in range(len(freq) if complete else 0):                            # a second code of one bit, never used
            if sum(lengths) < 2 and lengths[i] == 0:
                lengths[i] = 1
        return lengths
    heap = [(freq[i], i, k) for k, i in enumerate(used)]                          # (weight, tie-break, node); nodes 0 .. n - 1 are the leaves
    heapq.heapify(heap)
    children = []                                                                # of node n + j
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), len(used) + len(children)))
        children.append((a[2], b[2]))
    below = [0] * (len(used) + len(children))                                    # depth of every node, from the root (the last one made) down
    for j in range(len(children) - 1, -1, -1):
        for c in children[j]:
            below[c] = below[len(used) + j] + 1
    depth = dict(zip(used, below))
    if max(depth.values()) > limit:
        leaves = sorted((freq[i], i) for i in used)
        n = len(leaves)
        leaf_w, leaf_m = np.array([w for w, _ in leaves], np.int64), np.eye(n, dtype=np.uint8)      # a row: how often each leaf is in the item
        level_w, level_m = leaf_w, leaf_m
        for _ in range(limit - 1):                                               # packages of the level below, merged with the leaves
            k = len(level_w) // 2
            both_w = np.concatenate([leaf_w, level_w[0:2 * k:2] + level_w[1:2 * k:2]])
            both_m = np.concatenate([leaf_m, level_m[0:2 * k:2] + level_m[1:2 * k:2]])
            order = np.argsort(both_w, kind="stable")                            # stable: leaves in front of packages of equal weight
            level_w, level_m = both_w[order], both_m[order]
        depth = {i: int(d) for (_, i), d in zip(leaves, level_m[:2 * n - 2].sum(axis=0, dtype=np.int64))}
    for i, d in depth.items():
        lengths[i] = d
    return lengths


def canonical_codes(lengths) -> list:
    """RFC 1951 3.2.2: code lengths -> the codes, as integers read most significant bit first; 0 where the length is 0"""
    lengths = [int(l) for l in lengths]
    top = max(lengths, default=0)
    count = [0] * (top + 2)
    for l in lengths:
        if l:
            count[l] += 1
    nxt, code = [0] * (top + 2), 0
    for l in range(1, top + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


@functools.lru_cache(maxsize=None)
def _reversed16() -> np.ndarray:
    v = np.arange(65536, dtype=np.uint32)
    out = np.zeros(65536, np.uint32)
    for k in range(16):
        out |= ((v >> k) & 1) << (15 - k)
    return out


def _reversed_bits(code: int, n: int) -> int:
    """the n-bit code with its bits in reverse order: deflate packs from bit 0 up and wants a Huffman code's first bit first"""
    return int(_reversed16()[code]) >> (16 - n) if n else 0


def deflate_length_runs(lengths) -> list:
    """The code lengths of a dynamic block as (code-length symbol, extra bits, their value) (RFC 1951 3.2.7), greedily: a run of zeros
    goes out as 18 (11 .. 138 zeros) while 11 or more are left, then as 17 (3 .. 10), then one by one; a run of another length as the
    length itself once, then 16 (repeat the previous 3 .. 6 times) while 3 or more are left, then one by one."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, 7, k - 11))
                run -= k
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, 2, k - 3))
                run -= k
        out.extend([(v, 0, 0)] * run)
        i = j
    return out


@dataclasses.dataclass(frozen=True)
class DeflateTables:
    """One frame's dynamic Huffman block (RFC 1951 3.2.7), from the histogram emo_png_lz_count leaves."""
    lengths: np.ndarray        # int64 (320): the code length of every slot of the histogram (0 .. 285 literal / length, 288 .. 317 distance)
    codes: np.ndarray          # uint32 (320): length << 16 | the canonical code with its bits reversed - what emo_png_deflate_* read
    header: int                # BFINAL .. the last code length, the first bit on the wire in bit 0
    header_bits: int

    @property
    def end_of_block(self):
        """(the bit-reversed code of symbol 256, its length)"""
        return int(self.codes[256] & 0xFFFF), int(self.lengths[256])

    def token_bits(self, hist) -> int:
        """the bits of all the tokens a histogram counts, its end-of-block symbols left out"""
        h = np.asarray(hist).astype(np.int64)
        return int((h * (self.lengths + DEFLATE_EXTRA_BITS)).sum()) - int(h[256]) * int(self.lengths[256])


def deflate_tables(hist) -> DeflateTables:
    """A frame's symbol counts (320 integers as emo_png_lz_count adds them: literal / length symbols at 0 .. 285 with the end-of-block
    at 256, distance symbols at 288 .. 317) -> its Huffman codes, at most 15 bits each, and the header of its one dynamic block:
    BFINAL = 1, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code's lengths (at most 7 bits, in the order of 3.2.7) and the run-length
    coded lengths of both alphabets as one sequence (deflate_length_runs).  No distance symbol used: one distance code of length 0; one
    used: length 1."""
    h = np.asarray(hist)
    if h.shape != (ops.PNG_SYMBOLS,) or h.dtype.kind not in "iu":
        raise ValueError(f"deflate_tables takes {ops.PNG_SYMBOLS} integer counts, got {h.dtype} {h.shape}")
    h = h.astype(np.int64)
    if h[256] < 1:
        raise ValueError("deflate_tables: the histogram counts no end-of-block symbol")
    lit = huffman_code_lengths(h[:286], 15)
    dist = huffman_code_lengths(h[288:318], 15)
    n_lit = max(257, max(i for i, l in enumerate(lit) if l) + 1)
    n_dist = max([1] + [i + 1 for i, l in enumerate(dist) if l])
    runs = deflate_length_runs(lit[:n_lit] + dist[:n_dist])
    cl_freq = [0] * 19
    for sym, _, _ in runs:
        cl_freq[sym] += 1
    cl = huffman_code_lengths(cl_freq, 7, complete=True)
    cl_codes = canonical_codes(cl)
    n_cl = max(4, max(k for k, sym in enumerate(DEFLATE_CL_ORDER) if cl[sym]) + 1)
    value = nbits = 0

    def put(v, n):
        nonlocal value, nbits
        value |= v << nbits
        nbits += n

    put(1, 1)
    put(2, 2)
    put(n_lit - 257, 5)
    put(n_dist - 1, 5)
    put(n_cl - 4, 4)
    for sym in DEFLATE_CL_ORDER[:n_cl]:
        put(cl[sym], 3)
    for sym, nx, x in runs:
        put(_reversed_bits(cl_codes[sym], cl[sym]), cl[sym])
        put(x, nx)
    lengths = np.zeros(ops.PNG_SYMBOLS, np.int64)
    lengths[:286], lengths[288:318] = lit, dist
    plain = np.zeros(ops.PNG_SYMBOLS, np.int64)
    plain[:286], plain[288:318] = canonical_codes(lit), canonical_codes(dist)
    codes = (lengths << 16 | (_reversed16()[plain] >> np.where(lengths, 16 - lengths, 0))).astype(np.uint32)
    lengths.setflags(write=False)
    codes.setflags(write=False)
    return DeflateTables(lengths, codes, value, nbits)


def adler32_combine(pairs, nbytes) -> int:
    """The Adler-32 (RFC 1950 8.2) of consecutive pieces from the (s1, s2) each has on its own (the state after its bytes from (1, 0),
    as emo_png_filter leaves per row) and their lengths in bytes (one int for all, or one per piece): a stream in state (s1, s2)
    followed by a piece (r1, r2) of R bytes is in (s1 + r1 - 1, s2 + r2 + R (s1 - 1)), both mod 65521.  -> s2 << 16 | s1"""
    p = np.asarray(pairs).astype(np.int64).reshape(-1, 2)
    if len(p) < 1:
        return 1
    lens = np.broadcast_to(np.asarray(nbytes, np.int64), (len(p),)) % ADLER
    before = np.concatenate([[0], np.cumsum((p[:-1, 0] - 1) % ADLER)]) % ADLER    # s1 - 1 in front of every piece
    s1 = (1 + int(((p[:, 0] - 1) % ADLER).sum())) % ADLER
    s2 = int(((p[:, 1] + lens * before) % ADLER).sum()) % ADLER
    return s2 << 16 | s1


def _or_bits(buf: np.ndarray, at: int, value: int, nbits: int) -> None:
    """ORs nbits bits of value into the uint8 array, least significant bit first from bit `at`"""
    if nbits:
        raw = np.frombuffer((value << (at & 7)).to_bytes(((at & 7) + nbits + 7) // 8, "little"), np.uint8)
        buf[at >> 3:(at >> 3) + len(raw)] |= raw


def zlib_stream(tokens_at_their_bits: np.ndarray, tables: DeflateTables, token_bits: int, adler: int) -> bytes:
    """What the host adds to a frame's bytes as emo_png_deflate_emit leaves them (uint8, the tokens in place from bit 16 +
    tables.header_bits on, zero elsewhere): the zlib header 78 01 (deflate, 32 KiB window, no dictionary, fastest-level flag), the block
    header, the end-of-block code behind the tokens, and the Adler-32 big-endian behind the block's last byte"""
    buf = np.array(tokens_at_their_bits, dtype=np.uint8)
    end = 16 + tables.header_bits + int(token_bits)
    code, length = tables.end_of_block
    if len(buf) != (end + length + 7) // 8 + 4:
        raise ValueError(f"zlib_stream: {len(buf)} bytes for a block of {end + length} bits behind the 2-byte header")
    buf[0], buf[1] = 0x78, 0x01
    _or_bits(buf, 16, tables.header, tables.header_bits)
    _or_bits(buf, end, code, length)
    buf[-4:] = np.frombuffer(struct.pack(">I", adler), np.uint8)
    return buf.tobytes()


def png_chunk(kind: bytes, body: bytes) -> bytes:
    import zlib
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def _png_ihdr(width: int, height: int, channels: int) -> bytes:
    if channels not in PNG_COLOUR_TYPES or not (1 <= int(width) < 2 ** 31 and 1 <= int(height) < 2 ** 31):
        raise ValueError(f"a PNG frame is 1 .. 2^31 - 1 pixels each way with 1 (grey), 3 (RGB) or 4 (RGBA) channels, got {height} x {width} x {channels}")
    return png_chunk(b"IHDR", struct.pack(">IIBBBBB", int(width), int(height), 8, PNG_COLOUR_TYPES[channels], 0, 0, 0))


def png_container(width: int, height: int, channels: int, stream: bytes) -> bytes:
    """One still around its zlib stream (PNG section 5): signature, IHDR (bit depth 8, colour type 0 / 2 / 6, no interlace), one IDAT, IEND"""
    return PNG_SIGNATURE + _png_ihdr(width, height, channels) + png_chunk(b"IDAT", bytes(stream)) + png_chunk(b"IEND", b"")


def apng_delay(fps):
    """the (numerator, denominator) of a frame's delay in seconds, 1 / fps exactly (fps as fps_fraction takes it); ValueError when a
    term of the reduced fraction passes the 16 bits fcTL holds"""
    f = fps_fraction(fps)
    if f.denominator > 65535 or f.numerator > 65535:
        raise ValueError(f"an APNG frame's delay is a fraction of two 16-bit numbers: 1 / fps = {f.denominator} / {f.numerator} for fps = {fps!r} "
                         "does not fit 65535")
    return f.denominator, f.numerator


def apng_container(width: int, height: int, channels: int, streams, fps, loop: int = 0) -> bytes:
    """An animated PNG (APNG 1.0) around the frames' zlib streams: IHDR, acTL (frames, plays; 0: forever), then per frame an fcTL - the
    whole frame at (0, 0), the delay apng_delay(fps), dispose 0 (none), blend 0 (source) - and the stream, frame 0's in IDAT (the still
    a plain PNG reader shows), the others' in fdAT; fcTL and fdAT share one running sequence number.  IEND."""
    num, den = apng_delay(fps)
    loop = _int_in(loop, 0, 2 ** 31 - 1, "loop= (0: forever)")
    if len(streams) < 1:
        raise ValueError("apng_container: no frames")
    out, seq = [PNG_SIGNATURE, _png_ihdr(width, height, channels), png_chunk(b"acTL", struct.pack(">II", len(streams), loop))], 0
    for i, stream in enumerate(streams):
        out.append(png_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, int(width), int(height), 0, 0, num, den, 0, 0)))
        seq += 1
        if i == 0:
            out.append(png_chunk(b"IDAT", bytes(stream)))
        else:
            out.append(png_chunk(b"fdAT", struct.pack(">I", seq) + bytes(stream)))
            seq += 1
    out.append(png_chunk(b"IEND", b""))
    return b"".join(out)


def _png_check(filter="adaptive", strip_rows=PNG_STRIP_ROWS, loop=0, prefix=""):
    """the values of the PNG writers' options (prefix: how the caller spells loop=), before any launch"""
    _int_in(loop, 0, 2 ** 31 - 1, f"{prefix}loop= (0: forever)")
    _png_filter(filter)
    png_strip_rows(strip_rows, 1, 1, 1)


def _png_filter(filter):
    if not isinstance(filter, str) or filter not in ops.PNG_FILTERS:
        raise ValueError(f"filter= takes one of {', '.join(repr(k) for k in ops.PNG_FILTERS)}, got {filter!r}")
    return ops.PNG_FILTERS[filter]


def png_strip_rows(strip_rows, height: int, width: int, channels: int) -> int:
    """strip_rows= as the PNG writers take it (None: the frame as one strip) -> the scanlines per strip the kernels get: lowered to the
    frame's height and to what fits the 65535 bytes a strip may hold; ValueError where one scanline (1 + width * channels bytes) does not"""
    rows = int(height) if strip_rows is None else _int_in(strip_rows, 1, 2 ** 31 - 1, "strip_rows= (None: the frame as one strip)")
    row = 1 + int(width) * int(channels)
    if row > ops.PNG_MAX_STRIP_BYTES:
        raise ValueError(f"a scanline of {width} pixels of {channels} bytes is {row} bytes with its filter byte: above the "
                         f"{ops.PNG_MAX_STRIP_BYTES} bytes of a strip (the match table holds 16-bit offsets)")
    return max(1, min(rows, int(height), ops.PNG_MAX_STRIP_BYTES // row))


def png_zlib_streams(frames_u8: torch.Tensor, filter: str = "adaptive", strip_rows=PNG_STRIP_ROWS) -> list:
    """The device part of encode_png: (n, H, W, C) uint8 device frames -> the n zlib streams (bytes) an IDAT chunk holds.  Five
    launches - emo_png_filter, emo_png_lz_count, [the tables], emo_png_deflate_bits, a scan, emo_png_deflate_emit - around ONE small
    read (the n histograms and the rows' Adler-32 pairs) and the copy of the streams.  The sizes of all frames follow from the
    histograms and the code lengths, so the buffer is sized without a second read."""
    frames_u8 = _frames_u8(frames_u8, "png_zlib_streams", tuple(PNG_COLOUR_TYPES), (3, 4, 5), ("PNG", None)).contiguous()
    n, height, width, channels = (int(s) for s in frames_u8.shape)
    rows = png_strip_rows(strip_rows, height, width, channels)
    filtered, adler = ops.png_filter(frames_u8, _png_filter(filter))
    tokens, n_tokens, hist = ops.png_lz_count(filtered, channels, rows)
    hist_host, adler_host = hist.cpu().numpy(), adler.cpu().numpy()              # the one small read
    tables = [deflate_tables(h) for h in hist_host]
    codes = torch.from_numpy(np.stack([t.codes for t in tables]).view(np.int32)).to(frames_u8.device)
    bits = ops.png_deflate_bits(tokens, n_tokens, codes, height, width, channels, rows)
    token_bits = np.array([t.token_bits(h) for t, h in zip(tables, hist_host)], np.int64)
    head = np.array([16 + t.header_bits for t in tables], np.int64)
    # in front of a frame's tokens the zlib and block headers, behind them the end-of-block code, then 4 bytes of Adler-32
    offsets, starts, nbytes, out, _ = _stream_layout(bits, head, 4, token_bits + np.array([t.end_of_block[1] for t in tables], np.int64))
    ops.png_deflate_emit(tokens, n_tokens, codes, offsets, out, height, width, channels, rows)
    host = out.cpu().numpy()
    return [zlib_stream(host[s:s + b], t, tb, adler32_combine(a, 1 + width * channels))
            for s, b, t, tb, a in zip(starts, nbytes, tables, token_bits, adler_host)]


def encode_png(frames_u8: torch.Tensor, filter: str = "adaptive", strip_rows=PNG_STRIP_ROWS) -> list:
    """Packed uint8 frames on the device, (n, H, W, C) or (H, W, C) (or the (1, n, H, W, 3) of output_type="uint8") with C = 1 (grey),
    3 (RGB) or 4 (RGBA) -> n PNG files (bytes), lossless: the filtering, the LZ77 matching and the Huffman coding run on the device
    (png_zlib_streams), the host builds each frame's code tables from its histogram and wraps the stream in signature, IHDR, one IDAT
    and IEND.  filter="adaptive" picks per scanline the filter type with the smallest sum of absolute differences (libpng's
    heuristic); "none" | "sub" | "up" | "average" | "paeth" forces one.  strip_rows scanlines form a strip whose matches stay inside
    it (None: the whole frame; lowered where a strip would pass 65535 bytes); one dynamic Huffman block per frame either way."""
    frames_u8 = _frames_u8(frames_u8, "encode_png", tuple(PNG_COLOUR_TYPES), (3, 4, 5), ("PNG", None))
    height, width, channels = (int(s) for s in frames_u8.shape[1:])
    _png_check(filter, strip_rows)
    png_strip_rows(strip_rows, height, width, channels)
    return [png_container(width, height, channels, s) for s in png_zlib_streams(frames_u8, filter, strip_rows)]


def encode_apng(frames_u8: torch.Tensor, fps, loop: int = 0, filter: str = "adaptive", strip_rows=PNG_STRIP_ROWS) -> bytes:
    """The same frames -> one animated PNG as bytes, playing at exactly fps (apng_delay: the reduced fraction's terms must fit 16
    bits) and repeating `loop` times (0: forever).  Every frame is a whole frame (dispose 0, blend 0): no differences between frames.
    All arguments are checked before the first launch."""
    frames_u8 = _frames_u8(frames_u8, "encode_apng", tuple(PNG_COLOUR_TYPES), (3, 4, 5), ("PNG", None))
    height, width, channels = (int(s) for s in frames_u8.shape[1:])
    apng_delay(fps)
    _png_check(filter, strip_rows, loop)
    png_strip_rows(strip_rows, height, width, channels)
    return apng_container(width, height, channels, png_zlib_streams(frames_u8, filter, strip_rows), fps, loop)


def _png_pattern(path, who):
    """a `.png` path -> (path, whether its file name holds one %d-style field for the frame's number)"""
    import re
    path = _path_with(path, who, (".png",), "PNG stills (one, or numbered ones with a field for the frame's number as in `frame_%04d.png`)")
    name = os.path.basename(path).replace("%%", "")
    numbered = re.findall(r"%0?\d*d", name)
    if name.count("%") != len(numbered) or len(numbered) > 1 or "%" in os.path.dirname(path):
        raise ValueError(f"{who}: a pattern holds one field for the frame's number in the file's name, as in `frame_%04d.png`, got {path!r}")
    return path, bool(numbered)


def write_png(frames_u8: torch.Tensor, path, filter: str = "adaptive", strip_rows=PNG_STRIP_ROWS) -> list:
    """encode_png into files: a path whose name holds a %d-style field (`frames/frame_%04d.png`) takes any number of frames as numbered
    stills, counted from 0; a plain `.png` path takes exactly one frame.  -> the paths written"""
    path, numbered = _png_pattern(path, "write_png")
    frames_u8 = _frames_u8(frames_u8, "write_png", tuple(PNG_COLOUR_TYPES), (3, 4, 5), ("PNG", None))
    n = int(frames_u8.shape[0])
    if n > 1 and not numbered:
        raise ValueError(f"write_png: {n} frames and one file name {path!r}: put a field for the frame's number into it, as in `frame_%04d.png`, "
                         "for numbered stills, or write an animated `.apng` (encode_apng, write_video(format=\"apng\"))")
    files = encode_png(frames_u8, filter, strip_rows)
    paths = [path % i for i in range(n)] if numbered else [path]
    for p, data in zip(paths, files):
        _write_file(p, data)
    return paths


def write_apng(frames_u8: torch.Tensor, path, fps, **options) -> None:
    """encode_apng (with its options) into the `.apng` file at path"""
    _write_clip("write_apng", lambda: frames_u8, path, fps, FORMATS["apng"], None, options)


# ---------------------------------------------------------------------------------------------------------------------- reading PNG / APNG
PNG_CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}      # IHDR colour type -> channels at bit depth 8: grey, grey + alpha, RGB, RGBA
_PNG_ONLY = ("decode_png reads PNG and APNG files at bit depth 8 without interlace: grey, grey + alpha, RGB or RGBA; APNG frames that "
             "cover the whole canvas and replace it (blend_op 0)")


@dataclasses.dataclass(frozen=True)
class ParsedPng:
    """What parse_png takes from a PNG / APNG file: everything but the pixels."""
    width: int
    height: int
    channels: int              # 1 grey, 2 grey + alpha, 3 RGB, 4 RGBA
    still: bytes               # the raw deflate stream (RFC 1951) of the IDAT image: zlib header and Adler-32 taken off
    still_adler: int           # the Adler-32 its zlib stream ends with
    frames: tuple              # the animation's frames as (raw deflate stream, Adler-32); for a file without acTL the still alone
    delays: tuple              # a Fraction of a second per frame of the animation; () for a file without acTL
    loop: int                  # acTL num_plays (0: forever); 0 for a still
    animated: bool             # the file holds acTL
    still_in_animation: bool   # the IDAT image is the animation's first frame (an fcTL stands in front of it)


def _zlib_body(stream: bytes, what: str):
    """a zlib stream (RFC 1950) -> (the deflate stream inside, the Adler-32 behind it); the header is checked here"""
    if len(stream) < 6:
        raise ValueError(f"{what}: a zlib stream of {len(stream)} bytes holds no header and checksum")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8:
        raise ValueError(f"{what}: zlib compression method {cmf & 15}, PNG takes 8 (deflate)")
    if cmf >> 4 > 7:
        raise ValueError(f"{what}: a zlib window of 2^{(cmf >> 4) + 8} bytes, deflate stops at 32 KiB")
    if (cmf << 8 | flg) % 31:
        raise ValueError(f"{what}: the zlib header's check bits (FCHECK) are wrong")
    if flg & 0x20:
        raise ValueError(f"{what}: a zlib stream with a preset dictionary, which PNG does not allow")
    return bytes(stream[2:-4]), struct.unpack(">I", stream[-4:])[0]


def parse_png(data) -> ParsedPng:
    """A PNG (ISO/IEC 15948) or APNG 1.0 file's bytes -> ParsedPng.  The signature, every chunk's CRC, the order IHDR .. IDAT .. IEND, the
    sequence numbers of fcTL / fdAT and the zlib header of every frame are checked; the bodies of a frame's IDAT (or fdAT, less their
    sequence numbers) chunks are joined.  ValueError, naming what, for: a bit depth other than 8, a palette image (colour type 3), an
    interlaced (Adam7) file, an APNG frame that does not cover the whole canvas or blends over the one before (blend_op 1), a CRC
    mismatch, a missing IEND, an unknown critical chunk - and for a damaged structure.  Ancillary chunks are skipped; so is tRNS on
    grey and RGB files, as Pillow's `np.asarray(Image.open(f))` and `.convert("RGB")` leave the samples of such a file as they are."""
    import zlib
    data = bytes(data)
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("not a PNG file: the signature is missing")
    pos, ihdr, seq, ended = 8, None, 0, False
    n_frames = loop = None
    idat, groups, control = [], [], []      # groups: per fcTL the list its data chunks join; control: per fcTL (num, den)
    current, idat_state = None, 0           # idat_state: 0 in front of the IDAT chunks, 1 among them, 2 behind them
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError(f"a chunk header at byte {pos} runs past the file's end ({_PNG_ONLY}: no IEND)")
        size, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if pos + 12 + size > len(data):
            raise ValueError(f"chunk {kind!r} at byte {pos} runs past the file's end: no IEND")
        body = data[pos + 8:pos + 8 + size]
        if zlib.crc32(kind + body) != struct.unpack(">I", data[pos + 8 + size:pos + 12 + size])[0]:
            raise ValueError(f"chunk {kind!r} at byte {pos}: CRC mismatch")
        pos += 12 + size
        if kind != b"IDAT" and idat_state == 1:
            idat_state = 2
        if ihdr is None and kind != b"IHDR":
            raise ValueError(f"the first chunk is {kind!r}, not IHDR")
        if kind == b"IHDR":
            if ihdr is not None or size != 13:
                raise ValueError("a second or malformed IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
            width, height, depth, colour, comp, filt, lace = ihdr
            if colour == 3:
                raise ValueError(f"a palette image (colour type 3): {_PNG_ONLY}")
            if colour not in PNG_CHANNELS:
                raise ValueError(f"colour type {colour}: {_PNG_ONLY}")
            if depth != 8:
                raise ValueError(f"bit depth {depth}: {_PNG_ONLY}")
            if lace:
                raise ValueError(f"an interlaced (Adam7) file: {_PNG_ONLY}")
            if comp or filt or not width or not height or width >= 2 ** 31 or height >= 2 ** 31:
                raise ValueError(f"IHDR: {width} x {height}, compression method {comp}, filter method {filt}")
        elif kind == b"IDAT":
            if idat_state == 2:
                raise ValueError("IDAT chunks are not consecutive")
            idat_state = 1
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
        elif kind == b"acTL":
            if n_frames is not None or idat_state or size != 8:
                raise ValueError("a second, late or malformed acTL")
            n_frames, loop = struct.unpack(">II", body)
        elif kind == b"fcTL":
            if size != 26 or n_frames is None:
                raise ValueError("an fcTL of the wrong size or without acTL")
            s, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", body)
            if s != seq:
                raise ValueError(f"fcTL sequence number {s}, {seq} is next")
            seq += 1
            if (w, h, x, y) != (width, height, 0, 0):
                raise ValueError(f"an APNG frame of {w} x {h} at ({x}, {y}) on a canvas of {width} x {height}, a partial frame: {_PNG_ONLY}")
            if blend != 0:
                raise ValueError(f"an APNG frame that blends over the one before (blend_op {blend}): {_PNG_ONLY}")
            if idat_state == 0 and groups:
                raise ValueError("two fcTL chunks in front of IDAT")
            current = idat if idat_state == 0 else []
            groups.append(current)
            control.append(Fraction(num, den or 100))
        elif kind == b"fdAT":
            if size < 4 or current is None or current is idat:
                raise ValueError("an fdAT without its fcTL")
            s = struct.unpack(">I", body[:4])[0]
            if s != seq:
                raise ValueError(f"fdAT sequence number {s}, {seq} is next")
            seq += 1
            current.append(body[4:])
        elif not kind[0] & 0x20 and kind != b"PLTE":
            raise ValueError(f"unknown critical chunk {kind!r}")
    if not ended:
        raise ValueError("no IEND chunk: the file is cut")
    if ihdr is None or not idat:
        raise ValueError("no IDAT chunk")
    channels = PNG_CHANNELS[colour]
    still, still_adler = _zlib_body(b"".join(idat), "IDAT")
    if n_frames is None:
        return ParsedPng(width, height, channels, still, still_adler, ((still, still_adler),), (), 0, False, True)
    if len(groups) != n_frames or n_frames < 1:
        raise ValueError(f"acTL counts {n_frames} frames, the file holds {len(groups)} fcTL chunks")
    frames = []
    for i, g in enumerate(groups):
        if not g:
            raise ValueError(f"APNG frame {i} has no data")
        frames.append((still, still_adler) if g is idat else _zlib_body(b"".join(g), f"APNG frame {i}"))
    return ParsedPng(width, height, channels, still, still_adler, tuple(frames), tuple(control), int(loop), True, groups[0] is idat)


def _png_device(device, who):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ops._lib.EmoHipError(f"{who} decodes on the HIP device, got device {device} (there is no host decoder here)")
    return device


def _decode_png_streams(streams, height: int, width: int, channels: int, device, who: str) -> torch.Tensor:
    """[(raw deflate stream, Adler-32)] of frames of one shape -> uint8 (n, height, width, channels) on the device: ONE upload (offsets and
    streams), emo_png_inflate, emo_png_unfilter, ONE small read (both statuses, the byte counts, the rows' Adler pairs)"""
    n, row = len(streams), 1 + width * channels
    sizes = np.array([len(s) for s, _ in streams], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pad = -int(offsets[-1]) % 4 or (4 if offsets[-1] == 0 else 0)
    host = np.concatenate([offsets.view(np.uint8)] + [np.frombuffer(s, np.uint8) for s, _ in streams] + [np.zeros(pad, np.uint8)])
    dev = torch.from_numpy(host).to(device)                                       # the one copy
    filtered, produced, inflated = ops.png_inflate(dev[8 * (n + 1):], dev[:8 * (n + 1)].view(torch.int64), height, width, channels)
    frames, adler, unfiltered = ops.png_unfilter(filtered, channels)
    back = torch.cat([inflated, unfiltered, produced, adler.reshape(-1)]).cpu().numpy()                       # the one read
    for i in range(n):
        for entry, st in (("emo_png_inflate", int(back[i])), ("emo_png_unfilter", int(back[n + i]))):
            if st:
                at = f" after {int(back[2 * n + i])} of {height * row} bytes" if entry == "emo_png_inflate" else ""
                raise ValueError(f"{who}: frame {i} does not decode: {ops.PNG_STATUS.get(st, f'status {st}')}{at} ({entry} status {st})")
        got = adler32_combine(back[3 * n + 2 * height * i:3 * n + 2 * height * (i + 1)].view(np.uint32), row)
        if got != streams[i][1]:
            raise ValueError(f"{who}: frame {i}: the Adler-32 of the decoded scanlines is {got:08x}, the zlib stream ends with {streams[i][1]:08x}")
    return frames


def decode_png(files, device=None) -> torch.Tensor:
    """PNG files of one size and colour type (bytes each; what encode_png, Pillow or libpng write: bit depth 8, grey, grey + alpha, RGB
    or RGBA, no interlace) -> packed uint8 frames (n, H, W, C) on the device, byte for byte `np.asarray(Image.open(f))`.  The host walks
    the chunks only (parse_png); all streams go up in ONE copy and through two launches - emo_png_inflate, one wavefront per frame, and
    emo_png_unfilter - followed by one small read: the statuses and the scanlines' Adler-32 pairs, which the host combines and compares
    with every stream's trailer.  Of an APNG file the IDAT image is taken (decode_apng reads the animation).  ValueError naming the
    frame for a file parse_png refuses, a frame of another size or colour type, a stream that does not inflate (with the status), a
    filter type above 4, or a checksum that does not match.  There is no host decoder behind this."""
    files = list(files)
    if not files:
        raise ValueError("decode_png: no frames")
    device = _png_device(device, "decode_png")
    parsed = []
    for i, f in enumerate(files):
        try:
            parsed.append(parse_png(f))
        except ValueError as e:
            raise ValueError(f"decode_png: frame {i}: {e}") from None
    shape = (parsed[0].height, parsed[0].width, parsed[0].channels)
    for i, p in enumerate(parsed):
        if (p.height, p.width, p.channels) != shape:
            raise ValueError(f"decode_png: frame {i} is {p.height} x {p.width} x {p.channels}, frame 0 is {shape[0]} x {shape[1]} x {shape[2]}: "
                             "the frames of a clip share one size and colour type")
    return _decode_png_streams([(p.still, p.still_adler) for p in parsed], *shape, device, "decode_png")


def decode_apng(data, device=None, select=None):
    """An APNG file's bytes -> (uint8 frames (n, H, W, C) on the device, the delays as exact Fractions of a second, loop: acTL's
    num_plays, 0 forever).  The frames of the animation: the IDAT image is left out when no fcTL stands in front of it.  A PNG without
    acTL gives its one image, no delays and loop 0.  select= (a slice) picks frames before anything is decoded."""
    device = _png_device(device, "decode_apng")
    try:
        p = parse_png(data)
    except ValueError as e:
        raise ValueError(f"decode_apng: {e}") from None
    frames, delays = list(p.frames), list(p.delays)
    if select is not None:
        frames, delays = frames[select], delays[select]
        if not frames:
            raise ValueError(f"decode_apng: the file holds {len(p.frames)} frames; {select} selects none")
    return _decode_png_streams(frames, p.height, p.width, p.channels, device, "decode_apng"), delays, p.loop


def _png_rgb(frames: torch.Tensor) -> torch.Tensor:
    """(n, H, W, C) -> (n, H, W, 3) as Pillow's `.convert("RGB")`: grey in all three channels, alpha dropped"""
    c = int(frames.shape[-1])
    if c == 3:
        return frames
    return (frames[..., :1].expand(*frames.shape[:-1], 3) if c < 3 else frames[..., :3]).contiguous()


def _numbered_pngs(path, who) -> list:
    """the files a numbered pattern names: consecutive numbers from the first that exists, 0 or 1"""
    first = next((k for k in (0, 1) if os.path.exists(path % k)), None)
    if first is None:
        raise ValueError(f"{who}: neither {path % 0!r} nor {path % 1!r} exists")
    paths, k = [], first
    while os.path.exists(path % k):
        paths.append(path % k)
        k += 1
    return paths


def _read_png_clip(path, step, length, start, who):
    """read_video for `.apng`, an animated or still `.png` and a numbered pattern -> (RGB frames on the device, fps or None)"""
    path = os.fspath(path)
    if path.lower().endswith(".png") and _png_pattern(path, who)[1]:
        paths = _numbered_pngs(path, who)
        picked = paths[start::step][:length]
        if not picked:
            raise ValueError(f"{who}: {path!r} names {len(paths)} files; [{start}::{step}][:{length}] selects none")
        files = []
        for p in picked:
            with open(p, "rb") as f:
                files.append(f.read())
        return _png_rgb(decode_png(files)), None
    with open(path, "rb") as f:
        data = f.read()
    try:
        p = parse_png(data)
    except ValueError as e:
        raise ValueError(f"{who}: {path!r}: {e}") from None
    picked = list(p.frames)[start::step][:length]
    if not picked:
        raise ValueError(f"{who}: {path!r} holds {len(p.frames)} frames; [{start}::{step}][:{length}] selects none")
    delays = set(p.delays)
    fps = 1 / p.delays[0] if len(delays) == 1 and p.delays[0] > 0 else None
    return _png_rgb(_decode_png_streams(picked, p.height, p.width, p.channels, _png_device(None, who), f"{who}: {path!r}")), fps


# ---------------------------------------------------------------------------------------------------------------------- reading GIF
GIF_SIGNATURES = (b"GIF87a", b"GIF89a")
_GIF_ONLY = ("decode_gif reads GIF87a / GIF89a files whose frames have a colour table, global or local, and lie inside the logical screen, "
             "with LZW minimum code sizes 2 .. 8")


@dataclasses.dataclass(frozen=True)
class GifFrame:
    """One image of a GIF file as parse_gif finds it, with what the host resolves for the device."""
    left: int
    top: int
    width: int
    height: int
    interlace: bool
    transparent: object        # the transparent index of the frame's graphic control extension, or None
    delay: Fraction            # seconds; 0 without a graphic control extension
    disposal_bits: int         # the frame's own disposal bits (0 without a graphic control extension)
    disposal: int              # the EFFECTIVE disposal 0 .. 3: the most recent non-zero bits among the frames up to this one
    fill: int                  # the index a disposal 2 fills with: transparent, else the background index (0 where the table has no such entry)
    table_row: int             # the row of ParsedGif.tables the frame reads: 0 the global table where there is one
    table_entries: int         # that table's entries, 2 .. 256
    code_size: int             # the LZW minimum code size, 2 .. 8
    data: bytes                # the image data, sub-blocks joined


@dataclasses.dataclass(frozen=True)
class ParsedGif:
    """What parse_gif takes from a GIF file: everything but the pixels."""
    version: bytes             # b"GIF87a" or b"GIF89a"
    width: int                 # the logical screen
    height: int
    background: int            # the header's background index where there is a global table, else 0
    global_entries: int        # entries of the global colour table, 0 without one
    tables: np.ndarray         # uint8 (n_tables, 256, 3): the global table (if any) first, then the local ones in file order; unused entries zero
    frames: tuple              # GifFrame each
    loop: object               # the NETSCAPE2.0 loop count (0: forever), None without the extension (the clip plays once)
    trailer: bool              # the file ends with the trailer byte

    @property
    def delays(self):
        return tuple(f.delay for f in self.frames)


def parse_gif(data) -> ParsedGif:
    """A GIF87a / GIF89a file's bytes -> ParsedGif; no pixel is touched.  Read: the header, the logical screen descriptor (section 18),
    the global colour table and the background index (19), the NETSCAPE2.0 application extension (loop), and per frame the graphic
    control extension (23: the delay as an exact Fraction of a second, the transparent index or None, the disposal bits), the image
    descriptor (20: left, top, width, height, interlace flag, local colour table 21), the LZW minimum code size and the image data
    with its sub-blocks joined.  Comment, plain-text and other application extensions are skipped; a file without trailer is taken
    when it holds at least one complete frame, as Pillow takes it.
    Resolved here, as Pillow's GifImagePlugin resolves them: the EFFECTIVE disposal of a frame is sticky - the most recent non-zero
    disposal bits among frames 0 .. k (bits 4 .. 7 count as 3), so a frame with bits 0 or without a control extension inherits -; the
    index a disposal 2 fills with is the frame's transparent index, else the background index looked up in the FRAME's table; the row of
    `tables` and the entry count of the table the frame reads.  A background index at or beyond the table it is looked up in has no
    single rule in Pillow - frame 0 is disposed as a palette image and turns black, later frames go through `_rgb`, which takes entry
    0 (both pinned by the host tests) - so a file in which such a fill would be carried out is refused by name; where it is never
    carried out (the frame has a transparent index, another disposal, or is the last) the file is taken and `fill` is 0.
    ValueError, naming what the file has, for: a frame with no colour table, neither global nor local (Pillow's mode L path); a frame
    that reaches outside the logical screen (Pillow grows the canvas); an LZW minimum code size outside 2 .. 8; a transparent index
    at or beyond its frame's table; a disposal to a background index its frame's table does not hold; a zero-sized frame or screen; a file with no image; a sub-block, table or block that runs past
    the end of the file; a block that is no extension, image or trailer."""
    data = bytes(data)
    if data[:6] not in GIF_SIGNATURES:
        raise ValueError("not a GIF file: neither a GIF87a nor a GIF89a header")
    if len(data) < 13:
        raise ValueError("the logical screen descriptor runs past the end of the file")
    width, height, flags, background, _ = struct.unpack_from("<HHBBB", data, 6)
    if not width or not height:
        raise ValueError(f"a zero-sized logical screen ({width} x {height})")
    pos, tables, global_entries = 13, [], 0

    def table(pos, bits, what):
        k = 2 << bits
        if pos + 3 * k > len(data):
            raise ValueError(f"{what} of {k} entries runs past the end of the file")
        t = np.zeros((256, 3), np.uint8)
        t[:k] = np.frombuffer(data, np.uint8, 3 * k, pos).reshape(k, 3)
        tables.append(t)
        return pos + 3 * k, k

    def sub_blocks(pos, what):
        parts = []
        while True:
            if pos >= len(data):
                raise ValueError(f"a sub-block of {what} runs past the end of the file: no block terminator")
            size = data[pos]
            pos += 1
            if size == 0:
                return b"".join(parts), pos
            if pos + size > len(data):
                raise ValueError(f"a sub-block of {what} runs past the end of the file")
            parts.append(data[pos:pos + size])
            pos += size

    if flags & 0x80:
        pos, global_entries = table(pos, flags & 7, "the global colour table")
    else:
        background = 0
    frames, loop, trailer, sticky = [], None, False, 0
    delay, transparent, bits = Fraction(0), None, 0                              # of the graphic control extension in front of the next image
    while pos < len(data):
        kind = data[pos]
        pos += 1
        if kind == 0x3B:
            trailer = True
            break
        if kind == 0x21:
            if pos >= len(data):
                raise ValueError("an extension block runs past the end of the file")
            label = data[pos]
            if label == 0xFF and data[pos + 1:pos + 2] == b"\x0b" and data[pos + 2:pos + 13] == b"NETSCAPE2.0":
                body, pos = sub_blocks(pos + 13, "the NETSCAPE2.0 extension")
                if loop is None and len(body) >= 3 and body[0] == 1:
                    loop = struct.unpack_from("<H", body, 1)[0]
                continue
            body, pos = sub_blocks(pos + 1, f"extension {label:#04x}")
            if label == 0xF9 and len(body) >= 4:
                packed, cs, index = struct.unpack_from("<BHB", body)
                delay, transparent, bits = Fraction(cs, 100), (index if packed & 1 else None), (packed >> 2) & 7
                if bits:
                    sticky = min(bits, 3)
        elif kind == 0x2C:
            if pos + 9 > len(data):
                raise ValueError("an image descriptor runs past the end of the file")
            left, top, w, h, packed = struct.unpack_from("<HHHHB", data, pos)
            pos += 9
            k = len(frames)
            if not w or not h:
                raise ValueError(f"frame {k} is zero-sized ({w} x {h})")
            if left + w > width or top + h > height:
                raise ValueError(f"frame {k} ({w} x {h} at ({left}, {top})) reaches outside the logical screen of {width} x {height}: {_GIF_ONLY}")
            if packed & 0x80:
                pos, entries = table(pos, packed & 7, f"the local colour table of frame {k}")
                row = len(tables) - 1
            elif global_entries:
                row, entries = 0, global_entries
            else:
                raise ValueError(f"frame {k} has no colour table, neither a global nor a local one: {_GIF_ONLY}")
            if pos >= len(data):
                raise ValueError(f"the image data of frame {k} runs past the end of the file")
            code_size = data[pos]
            if not 2 <= code_size <= 8:
                raise ValueError(f"frame {k} has an LZW minimum code size of {code_size}: {_GIF_ONLY}")
            body, pos = sub_blocks(pos + 1, f"the image data of frame {k}")
            if transparent is not None and transparent >= entries:
                raise ValueError(f"frame {k} has the transparent index {transparent} and a colour table of {entries} entries")
            fill = transparent if transparent is not None else (background if background < entries else 0)
            frames.append(GifFrame(left, top, w, h, bool(packed & 0x40), transparent, delay, bits, sticky, fill, row, entries, code_size, body))
            delay, transparent, bits = Fraction(0), None, 0
        else:
            raise ValueError(f"block {kind:#04x} at byte {pos - 1} is no extension, image descriptor or trailer")
    if not frames:
        raise ValueError("the file holds no image")
    for k, f in enumerate(frames[:-1]):                                          # the last frame's disposal is never carried out
        if f.disposal == 2 and f.transparent is None and background >= f.table_entries:
            raise ValueError(f"frame {k} is disposed to the background index {background}, which its colour table of {f.table_entries} entries "
                             "does not hold (Pillow has no single colour for that)")
    return ParsedGif(data[:6], width, height, background, global_entries, np.stack(tables), tuple(frames), loop, trailer)


def gif_fps(delays):
    """the rate of a GIF's delays (Fractions of a second, whole centiseconds): 100 n / the sum of the centiseconds when every delay is
    positive and the largest and the smallest differ by at most one centisecond - the spread gif_delays gives a constant rate -, else
    None"""
    cs = [d * 100 for d in delays]
    if not cs or min(cs) <= 0 or max(cs) - min(cs) > 1:
        return None
    return Fraction(100 * len(cs)) / sum(cs)


def gif_descriptors(frames, slot) -> np.ndarray:
    """GifFrames in file order from frame 0 on, slot: {frame index: output slot} -> int32 (n, ops.GIF_FRAME_INTS), what emo_gif_compose
    reads per frame: left, top, w, h, the transparent index or -1, the effective disposal, the fill index, the interlace flag, the table
    row, the table's entries, the output slot or -1.  Nothing lies under frame 0, so a disposal 3 there becomes what Pillow does: a
    fill with the frame's transparent index, or nothing."""
    desc = np.zeros((len(frames), ops.GIF_FRAME_INTS), np.int32)
    for k, f in enumerate(frames):
        disposal, fill = f.disposal, f.fill
        if k == 0 and disposal == 3:
            disposal, fill = (2, f.transparent) if f.transparent is not None else (1, fill)
        desc[k] = (f.left, f.top, f.width, f.height, -1 if f.transparent is None else f.transparent, disposal, fill, int(f.interlace),
                   f.table_row, f.table_entries, slot.get(k, -1))
    return desc


def _decode_parsed_gif(p: ParsedGif, picked, device, who: str) -> torch.Tensor:
    """the frames `picked` (indices into p.frames, each at most once) -> uint8 (len(picked), H, W, 3) on the device, in that order: ONE
    upload (offsets, code sizes, descriptors, tables, streams), emo_gif_lzw_decode and emo_gif_compose over the frames up to the last
    picked one, ONE small read (both statuses and the counts)"""
    n = max(picked) + 1
    fr = p.frames[:n]
    slot = {k: i for i, k in enumerate(picked)}
    offsets = np.concatenate([[0], np.cumsum([len(f.data) for f in fr])]).astype(np.int64)
    out_offsets = np.concatenate([[0], np.cumsum([f.width * f.height for f in fr])]).astype(np.int64)
    code_size = np.array([f.code_size for f in fr], np.int32)
    desc = gif_descriptors(fr, slot)
    pad = -int(offsets[-1]) % 4 or (4 if offsets[-1] == 0 else 0)
    total = ops.gif_layout_check(offsets, code_size, out_offsets, int(offsets[-1]) + pad)      # before any launch
    parts = [offsets.view(np.uint8), out_offsets.view(np.uint8), code_size.view(np.uint8), desc.reshape(-1).view(np.uint8),
             np.ascontiguousarray(p.tables).reshape(-1)] + [np.frombuffer(f.data, np.uint8) for f in fr] + [np.zeros(pad, np.uint8)]
    dev = torch.from_numpy(np.concatenate(parts)).to(device)                      # the one copy
    at = np.cumsum([0] + [len(a) for a in parts[:5]])
    d_offsets, d_out = dev[at[0]:at[1]].view(torch.int64), dev[at[1]:at[2]].view(torch.int64)
    d_code, d_desc = dev[at[2]:at[3]].view(torch.int32), dev[at[3]:at[4]].view(torch.int32).view(n, ops.GIF_FRAME_INTS)
    d_tables = dev[at[4]:at[5]].view(-1, 256, 3)
    indices, produced, decoded = ops.gif_lzw_decode(dev[at[5]:], d_offsets, d_code, d_out, total)
    rgb, composed = ops.gif_compose(indices, d_out, d_desc, d_tables, len(picked), p.height, p.width)
    back = torch.cat([decoded, composed, produced]).cpu().numpy()                 # the one read
    for k, f in enumerate(fr):
        for entry, st in (("emo_gif_lzw_decode", int(back[k])), ("emo_gif_compose", int(back[n + k]))):
            if st:
                got = f" after {int(back[2 * n + k])} of {f.width * f.height} colour indices" if entry == "emo_gif_lzw_decode" else ""
                raise ValueError(f"{who}: frame {k} does not decode: {ops.gif_status_words(st)}{got} ({entry} status {st})")
    return rgb


def _gif_device(device, who):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ops._lib.EmoHipError(f"{who} decodes on the HIP device, got device {device} (there is no host decoder here)")
    return device


def decode_gif(data, device=None, select=None):
    """A GIF file's bytes -> (uint8 frames (n, H, W, 3) on the device at the size of the logical screen, the delays as exact Fractions of
    a second, loop: the NETSCAPE2.0 count, 0 forever, None without the extension).  Frame k is, byte for byte, what Pillow's
    `im.seek(k); im.convert("RGB")` gives (at its default LoadingStrategy.RGB_AFTER_FIRST): the canvas after frame k, with the
    transparency, the disposal of the frames before, sub-rectangles, local tables and interlace applied.  The host walks the blocks
    only (parse_gif); the LZW data, descriptors and tables of all frames go up in ONE copy and through two launches -
    emo_gif_lzw_decode, one wavefront per frame, and emo_gif_compose - followed by one small read of the statuses.  select= (a slice)
    picks the frames returned; every frame up to the last selected one is still decoded and composited, because the canvas depends
    on them, later ones are not.  ValueError for a file parse_gif refuses, and - naming the frame, the status in words and how far
    it got - for image data that does not decode or a colour index beyond its table.  There is no host decoder behind this."""
    device = _gif_device(device, "decode_gif")
    try:
        p = parse_gif(data)
    except ValueError as e:
        raise ValueError(f"decode_gif: {e}") from None
    picked = list(range(len(p.frames)))
    if select is not None:
        picked = picked[select]
        if not picked:
            raise ValueError(f"decode_gif: the file holds {len(p.frames)} frames; {select} selects none")
    return _decode_parsed_gif(p, picked, device, "decode_gif"), [p.frames[k].delay for k in picked], p.loop


def _read_gif_clip(path, step, length, start, who):
    """read_video for a `.gif` -> (RGB frames on the device, fps or None)"""
    path = os.fspath(path)
    with open(path, "rb") as f:
        data = f.read()
    try:
        p = parse_gif(data)
    except ValueError as e:
        raise ValueError(f"{who}: {path!r}: {e}") from None
    picked = list(range(len(p.frames)))[start::step][:length]
    if not picked:
        raise ValueError(f"{who}: {path!r} holds {len(p.frames)} frames; [{start}::{step}][:{length}] selects none")
    return _decode_parsed_gif(p, picked, _gif_device(None, who), f"{who}: {path!r}"), gif_fps(p.delays)


def save_images_grid(images: torch.Tensor, path: str, quality: int = 90):
    """magicanimate/utils/util.py:35-41: (b, c, 1, h, w) in [0, 1] -> one image file of the grid `torchvision.utils.make_grid(images)`
    lays out with its defaults (8 per row, 2 pixels of padding; make_grid_u8), `* 255` truncated to uint8 as :39 does.  `.png` is written
    lossless (encode_png), `.jpg` / `.jpeg` as one baseline JPEG frame at `quality` (the frame encode_mjpeg makes).  The file is
    encoded on the HIP device: images held on the host are uploaded."""
    path = _path_with(path, "save_images_grid", (".png", ".jpg", ".jpeg"), "one image, lossless as PNG or as a baseline JPEG")
    if not torch.is_tensor(images) or images.dim() != 5 or images.shape[2] != 1:
        raise ValueError(f"save_images_grid takes a float (b, c, 1, h, w) tensor, got {tuple(getattr(images, 'shape', ()))}")
    _check_quality(quality)
    if not images.is_cuda:
        images = images.to("cuda")
    grid = make_grid_u8(images, n_rows=8)                                        # (1, Hg, Wg, 3)
    if path.lower().endswith(".png"):
        data = encode_png(grid)[0]
    else:
        out, starts, bits = encode_streams(grid, quality)
        data = jpeg_header(int(grid.shape[1]), int(grid.shape[2]), int(quality)) + finish_scan(out.cpu().numpy()[int(starts[0]):], int(bits[0]))
    _write_file(path, data)


# ---------------------------------------------------------------------------------------------------------------------- reference surface
def encode_avi(frames_u8: torch.Tensor, fps, quality: int = 90, restart_interval=None, audio=None) -> bytes:
    """(n, H, W, 3) uint8 device frames -> a Motion-JPEG `.avi` file as bytes: encode_mjpeg (with its restart_interval) + avi_container"""
    jpegs = encode_mjpeg(frames_u8, quality, restart_interval)                   # (checks the arguments)
    return avi_container(jpegs, int(frames_u8.shape[-2]), int(frames_u8.shape[-3]), fps, audio=audio)


def _avi_check(quality=90, restart_interval=None, prefix=""):
    _check_quality(quality)
    restart_mcus(restart_interval, 16)


@dataclasses.dataclass(frozen=True)
class OutputFormat:
    """One file format of the writers.  FORMATS holds them all, and what a writer or the pipeline's save_path= decides per format is
    read from it: the path it takes, the keywords it takes and whose the others are, whether fps= and audio= mean anything to it."""
    format: object      # the format= of write_video, save_videos_grid and images2video that selects it; save_path= goes by ext
    ext: str
    noun: str           # what the refusals call it
    options: tuple      # the keywords it owns
    check: object       # (**options, prefix=): refuses a bad value of one, before any launch
    encode: object      # (frames_u8, fps, **options) -> the file's bytes; stills, which write_png numbers: no fps, one file per frame
    plays: bool = True  # it has a frame rate, so fps= is needed
    rate: object = None     # (fps, n_frames): refuses a rate such a file cannot hold, where there is one
    sound: bool = False     # it holds audio=


FORMATS = {
    "avi": OutputFormat(None, ".avi", "a Motion-JPEG `.avi` file", ("quality", "restart_interval"), _avi_check, encode_avi, sound=True),
    "gif": OutputFormat("gif", ".gif", "an animated GIF", GIF_OPTIONS, _gif_check, encode_gif, rate=gif_delays),
    "apng": OutputFormat("apng", ".apng", "an animated PNG", PNG_OPTIONS, _png_check, encode_apng, rate=lambda fps, n: apng_delay(fps)),
    "png": OutputFormat("png", ".png", "numbered PNG stills", PNG_OPTIONS[:2], _png_check, encode_png, plays=False),
}
# option -> the keyword of the pipeline call that carries it
SAVE_KEYWORDS = {"quality": "save_quality", "restart_interval": "save_restart_interval", "palette": "save_palette", "dither": "save_dither",
                 "dither_strength": "save_dither_strength", "loop": "save_loop", "filter": "save_png_filter"}


def _listed(words, last="and") -> str:
    words = list(words)
    return words[0] if len(words) == 1 else f"{', '.join(words[:-1])} {last} {words[-1]}"


def _path_with(path, who, exts, hint):
    """path as a str where it ends in one of exts, in either case; the refusal says what `who` writes - hint - and names exts"""
    path = os.fspath(path)
    if os.path.splitext(path)[1].lower() not in exts:
        raise ValueError(f"{who} writes {hint}: name the file {_listed((f'`{e}`' for e in exts), 'or')}, got {path!r}")
    return path


def _write_file(path, data) -> None:
    d = os.path.dirname(os.fspath(path))
    if d:
        os.makedirs(d, exist_ok=True)            # util.py:32
    with open(path, "wb") as fh:
        fh.write(data)


def _given(options) -> dict:
    """the options that were set: not None, and not the quality the writers have as their default"""
    return {k: v for k, v in options.items() if v is not None and (k != "quality" or v != 90)}


def _own_options(record, options, who, save=False) -> None:
    """Refuses the options `record` does not own, before anything runs, and says which format owns them.  save: the caller is the
    pipeline call, which spells the options as SAVE_KEYWORDS does, knows no others, and selects a format by save_path's extension."""
    def names(options):
        return _listed([f"{SAVE_KEYWORDS[k]}=" for k in options if k in SAVE_KEYWORDS] if save else [f"{k}=" for k in options])
    foreign = sorted(set(options) - set(record.options))
    if foreign:
        owners = dict.fromkeys(next((r for r in FORMATS.values() if k in r.options), None) for k in foreign)      # the first that owns it
        how = (lambda r: f"`{r.ext}` save_path") if save else (lambda r: f"format=\"{r.format}\", `{r.ext}` path" if r.format else f"`{r.ext}` path, no format=")
        raise ValueError(f"{who}: unknown option{'s' if len(foreign) > 1 else ''} {names(foreign)} for {record.noun}, which takes {names(record.options)}"
                         + "".join(f"; {names(r.options)} belong to {r.noun} ({how(r)})" for r in owners if r is not None))


def _write_clip(who, frames, path, fps, record, audio, options, hint=None) -> None:
    """The one sequence behind every writer of a clip: the path has the format's extension, the options are the format's own, audio=
    comes only where the format holds sound - all before frames() is asked for the frames, so before anything is uploaded or
    launched; then encode, which checks the frames and the options' values before its first launch, and write."""
    path = _path_with(path, who, (record.ext,), hint or record.noun)
    _own_options(record, options, who)
    if audio is not None and not record.sound:
        raise ValueError(f"{who}: {record.noun} holds no sound: audio= has no place in one; write an `.avi` file for audio=")
    _write_file(path, record.encode(frames(), fps, **options, **({} if audio is None else {"audio": audio})))


def _write_video(who, frames, path, fps, quality, audio, restart_interval, format, options) -> None:
    """write_video, for it and for the two entries of the reference surface, which hand over frames() they make only once nothing is refused"""
    named = {r.format: r for r in FORMATS.values() if r.plays}
    if not isinstance(format, (str, type(None))) or format not in named:
        raise ValueError(f"{who}: format= takes {_listed((f'{f!r} for {r.noun}' for f, r in named.items()), 'or')}, got {format!r}")
    hint = None if format is not None else named[None].noun + " (" + ", ".join(
        f"format=\"{f}\" with a `{r.ext}` path writes {r.noun}" for f, r in named.items() if f) + "; mp4 needs an encoder that is not part of this build)"
    _write_clip(who if format is None else f"{who} with format=\"{format}\"", frames, path, fps, named[format], audio,
                {**_given(dict(quality=quality, restart_interval=restart_interval)), **options}, hint)


def write_video(frames_u8: torch.Tensor, path, fps, quality: int = 90, audio=None, restart_interval=None, format=None, **options) -> None:
    """(n, H, W, 3) uint8 device frames -> an `.avi` file: encode_mjpeg (with its restart_interval) + avi_container.  With format="gif"
    and a `.gif` path: an animated GIF instead (encode_gif; its options - loop, colors, palette, dither, dither_strength, strip_rows -
    as keywords).  With format="apng" and an `.apng` path: a lossless animated PNG (encode_apng; its options are filter, strip_rows
    and loop).  FORMATS says which keywords a format owns; another format's are refused by its name, and so is audio= where the format
    holds no sound."""
    _write_video("write_video", lambda: frames_u8, path, fps, quality, audio, restart_interval, format, options)


@dataclasses.dataclass(frozen=True)
class SavePlan:
    """What save_path= of the pipeline call writes once the frames exist (save_plan): the file's format, its path, the rate it plays at
    (None: stills) and the options that were set."""
    record: OutputFormat
    path: str
    rate: object
    options: dict

    def write(self, frames_u8, audio=None):
        if not self.record.plays:
            return write_png(frames_u8, self.path, **self.options)
        _write_clip("save_path=", lambda: frames_u8, self.path, self.rate, self.record, audio, self.options)


def save_plan(save_path, n_frames: int, fps, interpolation_factor: int, options: dict) -> SavePlan:
    """Everything save_path= of the pipeline call can be refused for before the denoising loop, in one place: the extension names a
    format of FORMATS; `options` - the call's save_* keywords by the option they carry (SAVE_KEYWORDS), None where not given - are
    that format's own and hold values it takes; n_frames stills have a numbered name; the rate, fps * interpolation_factor, is one
    the file can hold.  fps=None leaves the rate open, which only stills may (SavePlan.rate stays None)."""
    path = _path_with(save_path, "save_path=", tuple(r.ext for r in FORMATS.values()), _listed((r.noun for r in FORMATS.values()), "or"))
    record = next(r for r in FORMATS.values() if r.ext == os.path.splitext(path)[1].lower())
    options = _given(options)
    _own_options(record, options, "save_path=", save=True)
    record.check(**options, prefix="save_")
    if not record.plays and not _png_pattern(path, "save_path=")[1] and n_frames > 1:
        raise ValueError(f"save_path={path!r} names one `.png` file for {n_frames} frames: put a field for the frame's number "
                         "into the name, as in `frames/f_%04d.png`, or name the file `.apng` for an animated PNG")
    rate = None
    if record.plays and fps is not None:
        rate = fps_fraction(fps * int(interpolation_factor))
        if record.rate is not None:
            record.rate(rate, n_frames)
    return SavePlan(record, path, rate, options)


def make_grid_u8(videos: torch.Tensor, rescale=False, n_rows=6) -> torch.Tensor:
    """(b, c, t, h, w) float in [0, 1] ([-1, 1] with rescale) -> (t, Hg, Wg, 3) uint8, the frames save_videos_grid hands to its writer:
    torchvision.utils.make_grid(x, nrow=n_rows) with its defaults per time step (b == 1: the frame itself; otherwise xmaps = min(n_rows, b)
    cells of (h + 2, w + 2) across a zero canvas of (h + 2) * ymaps + 2 by (w + 2) * xmaps + 2, image k at (y * (h + 2) + 2,
    x * (w + 2) + 2)), then (x * 255) truncated to uint8 (values outside [0, 1] are clamped rather than wrapped).  Torch copies on the
    videos' device."""
    if not torch.is_tensor(videos) or videos.dim() != 5 or videos.shape[1] not in (1, 3) or not videos.is_floating_point():
        raise ValueError(f"save_videos_grid takes a float (b, c, t, h, w) tensor with c = 1 or 3, got {tuple(getattr(videos, 'shape', ()))}")
    b, c, t, h, w = videos.shape
    x = videos.permute(2, 0, 3, 4, 1)                                            # t b h w c
    if c == 1:
        x = x.expand(t, b, h, w, 3)                                              # make_grid repeats a single channel
    if b == 1:
        grid = x[:, 0]
    else:
        xmaps = min(int(n_rows), b)
        ymaps = -(-b // xmaps)
        grid = torch.zeros(t, (h + 2) * ymaps + 2, (w + 2) * xmaps + 2, 3, device=videos.device, dtype=videos.dtype)
        for k in range(b):
            y0, x0 = (k // xmaps) * (h + 2) + 2, (k % xmaps) * (w + 2) + 2
            grid[:, y0:y0 + h, x0:x0 + w] = x[:, k]
    if rescale:
        grid = (grid + 1.0) / 2.0                                                # util.py:28
    return (grid * 255).clamp(0, 255).to(torch.uint8).contiguous()               # util.py:29


def save_videos_grid(videos: torch.Tensor, path: str, rescale=False, n_rows=6, fps=25, quality: int = 90, restart_interval=None, format=None,
                     **options):
    """magicanimate/utils/util.py:21-33 with a Motion-JPEG `.avi` in place of imageio.mimsave.  The frames are encoded on the HIP device:
    videos held on the host are uploaded.  restart_interval as in encode_mjpeg.  format="gif" with a `.gif` path writes the animated GIF
    mimsave would, format="apng" with an `.apng` path a lossless animated PNG (write_video)."""
    frames = lambda: make_grid_u8(videos if not torch.is_tensor(videos) or videos.is_cuda else videos.to("cuda"), rescale, n_rows)
    _write_video("save_videos_grid", frames, path, fps, quality, None, restart_interval, format, options)


def images2video(video, path, fps=8, quality: int = 90, restart_interval=None, format=None, **options):
    """util.py:111-113: a sequence of (H, W, 3) uint8 frames (arrays, or one (t, H, W, 3) array / tensor) -> an `.avi` file.
    restart_interval as in encode_mjpeg.  format="gif" with a `.gif` path writes an animated GIF, format="apng" with an `.apng` path a
    lossless animated PNG (write_video)."""
    frames = lambda: (video if torch.is_tensor(video) else torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f) for f in video])))).to("cuda")
    _write_video("images2video", frames, path, fps, quality, None, restart_interval, format, options)


def decode_jpeg(data: bytes) -> np.ndarray:
    """one JPEG file -> (H, W, 3) uint8 RGB (Pillow's decoder)"""
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def video2images(path, step=4, length=16, start=0):
    """util.py:102-108: the frames [start::step][:length] of an `.avi` file this module wrote, as (H, W, 3) uint8 arrays; of an `.apng` /
    `.png` / `.gif` file or a numbered `.png` pattern (read_video, decoded on the device) the same frames, copied to the host"""
    if not os.fspath(path).lower().endswith(".avi"):
        return list(read_video(path, step, length, start)[0].cpu().numpy())
    jpegs, _, _ = read_avi(path)
    return [decode_jpeg(j) for j in jpegs[start::step][:length]]


def read_image(path_or_bytes, size=None, resample="bicubic", progressive: bool = False) -> torch.Tensor:
    """One baseline JPEG file (a path, or the file's bytes) -> (H, W, 3) uint8 ON THE DEVICE, decoded by decode_mjpeg: what
    `np.array(Image.open(path).convert("RGB"))` gives, byte for byte, without the pixels passing through a host decoder.
    size=(width, height) resizes the frame as `.resize(size)` does (resize_frames with `resample`), still on the device.  ValueError
    from parse_jpeg for a file it refuses (progressive, arithmetic-coded, 4:1:1, RGB, ...): Pillow reads those.
    progressive=True also decodes a Huffman-coded progressive file (SOF2) with a complete progression on the device, scan by scan
    (decode_mjpeg(progressive=True)): the same bytes, since libjpeg reads such a file to the coefficients of the baseline one; a
    progression that stops early, which libjpeg smooths, stays refused.
    A PNG file (recognised by its signature; what parse_png takes: 8 bits, grey, grey + alpha, RGB or RGBA, no interlace) is decoded by
    decode_png and brought to RGB as `.convert("RGB")` does - grey in all three channels, alpha dropped - by indexing on the device.
    A GIF file (recognised by its signature, `GIF87a` or `GIF89a`; what parse_gif takes) gives its first frame, decoded by decode_gif:
    what `Image.open(path).convert("RGB")` gives."""
    if size is not None:
        size, resample = _resize_size(size, "read_image"), _resize_filter(resample)
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    try:
        if data[:8] == PNG_SIGNATURE:
            parse_png(data)
        elif data[:6] in GIF_SIGNATURES:
            parse_gif(data)
        else:
            parse_jpeg(data, restart=True, layouts=True, progressive=progressive)
    except ValueError as e:
        raise ValueError(f"read_image: {e}") from None
    if data[:6] in GIF_SIGNATURES:
        frames = decode_gif(data, select=slice(0, 1))[0]
    else:
        frames = _png_rgb(decode_png([data])) if data[:8] == PNG_SIGNATURE else decode_mjpeg([data], progressive=progressive)
    if size is not None and (int(frames.shape[2]), int(frames.shape[1])) != size:
        frames = resize_frames(frames, size, resample)
    return frames[0]


def read_video(path, step=1, length=None, start=0, size=None, resample="bicubic", progressive: bool = False):
    """An `.avi` file this module wrote -> (uint8 frames (n, H, W, 3) ON THE DEVICE, fps Fraction, audio as read_avi returns it): the
    frames [start::step][:length], decoded by decode_mjpeg.  What `VideoReader(path).read()` gives magicanimate/pipelines/animation.py:174-185,
    without the frames passing through a host decoder.  size=(width, height) resizes the decoded frames as animation.py:177 does
    (resize_frames with `resample`), still on the device; None returns them as stored.  progressive=True takes progressive frames
    too, mixed with baseline ones (decode_mjpeg(progressive=True)).
    An `.apng` file, an animated (or still) `.png` file and a numbered pattern as write_png takes it (`frames/f_%04d.png`: consecutive
    numbers from the first file that exists, 0 or 1) are read too, inflated and unfiltered on the device (decode_png, decode_apng) and
    brought to RGB as read_image does; only the selected frames are decoded.  fps is then 1 / delay where all the file's delays are
    equal, else None - None for stills -, and audio is None.
    A `.gif` file is read too (decode_gif: LZW decoding and the compositing of the frames on the device; every frame up to the last
    selected one is decoded, since a GIF frame is a patch on the canvas the frames before it left).  fps is then 100 n / the sum of the
    file's n delays in centiseconds when every delay is positive and the largest and the smallest differ by at most one centisecond
    (what gif_delays writes for a constant rate: 30 fps comes back as 30), else None; audio is None."""
    if size is not None:
        size, resample = _resize_size(size, "read_video"), _resize_filter(resample)
    if os.fspath(path).lower().endswith(".gif"):
        frames, fps = _read_gif_clip(path, step, length, start, "read_video")
        if size is not None and (int(frames.shape[2]), int(frames.shape[1])) != size:
            frames = resize_frames(frames, size, resample)
        return frames, fps, None
    if os.fspath(path).lower().endswith((".png", ".apng")):
        frames, fps = _read_png_clip(path, step, length, start, "read_video")
        if size is not None and (int(frames.shape[2]), int(frames.shape[1])) != size:
            frames = resize_frames(frames, size, resample)
        return frames, fps, None
    jpegs, fps, audio = read_avi(path)
    picked = jpegs[start::step][:length]
    if not picked:
        raise ValueError(f"read_video: {os.fspath(path)!r} holds {len(jpegs)} frames; [{start}::{step}][:{length}] selects none")
    frames = decode_mjpeg(picked, progressive=progressive)
    if size is not None and (int(frames.shape[2]), int(frames.shape[1])) != size:
        frames = resize_frames(frames, size, resample)
    return frames, fps, audio


def load_control_clip(path, size, window, offset=0, max_length=None, resample="bicubic", progressive: bool = False):
    """magicanimate/pipelines/animation.py:174-194 for a Motion-JPEG `.avi` file (or an `.apng`, `.png` or `.gif` clip, as read_video takes them) -> (control frames uint8 (t, height, width, 3) on the
    device, original_length): every frame is read (:175), resized to size=(width, height) when the clip has another size (:176-177; the
    reference compares the height alone, having square frames on both sides), cut to [offset : offset + max_length] when max_length is
    given (:178-179) and, when what is left is no multiple of `window` (config.L, the context length), followed by copies of its last
    frame up to the next multiple (:192-194, np.pad mode="edge").  original_length is the frame count in front of that padding: the
    length comparison_videos cuts the result back to.  Nothing leaves the device.  progressive= as in read_video."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"load_control_clip: window= is the context length, a positive int, got {window!r}")
    if isinstance(offset, bool) or not isinstance(offset, (int, np.integer)) or offset < 0:
        raise ValueError(f"load_control_clip: offset= is a frame index >= 0, got {offset!r}")
    if max_length is not None and (isinstance(max_length, bool) or not isinstance(max_length, (int, np.integer)) or max_length < 1):
        raise ValueError(f"load_control_clip: max_length= is None or a positive int, got {max_length!r}")
    # existing host tests replace read_video by a stand-in without the keyword: it is handed over only when set
    frames, _, _ = read_video(path, size=_resize_size(size, "load_control_clip"), resample=resample, **(dict(progressive=True) if progressive else {}))
    total = int(frames.shape[0])
    if max_length is not None:
        frames = frames[int(offset):int(offset) + int(max_length)]
    original_length = int(frames.shape[0])
    if original_length < 1:
        raise ValueError(f"load_control_clip: {os.fspath(path)!r} holds {total} frames; [{offset}:{offset}+{max_length}] selects none")
    if original_length % window:
        frames = torch.cat([frames, frames[-1:].expand(window - original_length % window, *frames.shape[1:])])
    return frames, original_length


def comparison_videos(source_u8, control_u8, sample, original_length) -> torch.Tensor:
    """magicanimate/pipelines/animation.py:217-228: the three clips every reference run lays side by side - the source image repeated,
    the control frames / 255 and the sample, each cut to original_length frames - as one float32 (3, c, t, h, w) tensor on the sample's
    device, ready for save_videos_grid.  source_u8: uint8 (h, w, 3); control_u8: uint8 (>= t, h, w, 3) (load_control_clip's frames);
    sample: float (1, c, >= t, h, w) in [0, 1] (the pipeline's `.videos`).  The 256 quotients x / 255 are taken on the host in doubles,
    as the reference takes them, and gathered."""
    if not torch.is_tensor(sample) or sample.dim() != 5 or sample.shape[0] != 1 or not sample.is_floating_point():
        raise ValueError(f"comparison_videos: sample is the pipeline's float (1, c, t, h, w) videos, got {tuple(getattr(sample, 'shape', ()))}")
    t = int(original_length)
    _, c, f, h, w = sample.shape
    as_u8 = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(sample.device)
    source_u8, control_u8 = as_u8(source_u8), as_u8(control_u8)
    if source_u8.dtype != torch.uint8 or tuple(source_u8.shape) != (h, w, c):
        raise ValueError(f"comparison_videos: source_u8 is one uint8 ({h}, {w}, {c}) frame at the sample's size, got {source_u8.dtype} {tuple(source_u8.shape)}")
    if control_u8.dtype != torch.uint8 or control_u8.dim() != 4 or tuple(control_u8.shape[1:]) != (h, w, c):
        raise ValueError(f"comparison_videos: control_u8 is uint8 (t, {h}, {w}, {c}) at the sample's size, got {control_u8.dtype} {tuple(control_u8.shape)}")
    if not 1 <= t <= min(f, int(control_u8.shape[0])):
        raise ValueError(f"comparison_videos: original_length {original_length!r} with {control_u8.shape[0]} control frames and a sample of {f}")
    unit = torch.from_numpy((np.arange(256) / 255.0).astype(np.float32)).to(sample.device)
    source = unit[source_u8.long()].permute(2, 0, 1)[None, :, None].expand(1, c, t, h, w)             # :217-218
    control = unit[control_u8[:t].long()].permute(3, 0, 1, 2)[None]                                   # :221-224
    return torch.cat([source, control, sample[:, :, :t].float()])                                     # :226-228
