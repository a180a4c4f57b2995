"""The signal path in front of the wav2vec2 encoder (Net.py:627-640): what `sf.read`, `librosa.resample`,
`waveform.mean(axis=1)` and the processor's utterance normalisation do between a file and `input_values`.

  read_wav          a RIFF/WAVE parser (PCM 8 / 16 / 24 / 32, IEEE float 32 / 64, WAVE_FORMAT_EXTENSIBLE around those) - file IO, host
  resample_taps     the resampling filter, designed in float64 (a DESIGN CHOICE, DESIGN.md section 1 row (f)4: the reference calls
                    librosa.resample, whose default filter is a third-party table; this is scipy.signal.resample_poly's
                    Kaiser(5.0)-windowed sinc, reproduced to 4.4e-16)
  phase_table       the same taps, rounded once to f32, one row per output phase - the layout emo_audio_resample reads
  prepare_waveform  upload -> emo_audio_resample (channel downmix + rational polyphase resampling) -> emo_waveform_normalize: the
                    (1, n) f32 `input_values` on the device

Demuxing a video container (Net.py:683-692 goes through moviepy) is not built: extract_features_from_mp4 reads the .wav beside the video.
"""
from __future__ import annotations

import functools
import math
import os
import struct

import numpy as np
import torch

from . import ops

TARGET_RATE = 16000                  # Wav2Vec2FeatureExtractor.sampling_rate of wav2vec2-base-960h (Net.py:630)
MAX_RATE_FACTOR = 65536              # max(up, down) past this is a table of > 1.3 M taps (a rate pair such as 96001 -> 16000)
KAISER_BETA = 5.0

WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE


# ----------------------------------------------------------------------------------------------------------------- file reading
def read_wav(path):
    """A .wav file -> (frames float32 (n, channels), sample_rate).  Integer PCM is scaled like soundfile's float read: 8-bit unsigned
    (v - 128) / 128, 16 / 24 / 32-bit signed v / 2^(bits - 1); IEEE float 32 / 64 is taken as it is (64 rounded to f32).  Unknown chunks
    are skipped (with their odd-size pad byte); a `data` size of 0 or 0xFFFFFFFF (a streamed file) means "to the end of the file"."""
    with open(os.fspath(path), "rb") as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise ValueError(f"read_wav: {path!r} is not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        body = pos + 8
        if cid == b"data":
            end = len(raw) if size in (0, 0xFFFFFFFF) else min(body + size, len(raw))
            data = raw[body:end]
            break
        if cid == b"fmt ":
            if size < 16 or body + size > len(raw):
                raise ValueError("read_wav: truncated fmt chunk")
            fmt = raw[body:body + size]
        pos = body + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError("read_wav: no fmt chunk before the data chunk" if fmt is None else "read_wav: no data chunk")
    tag, channels, rate, _, block_align, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == WAVE_FORMAT_EXTENSIBLE:
        if len(fmt) < 40:
            raise ValueError("read_wav: WAVE_FORMAT_EXTENSIBLE with a short fmt chunk")
        tag = struct.unpack_from("<H", fmt, 24)[0]           # the first two bytes of the SubFormat GUID are the format tag
    if channels < 1 or rate < 1:
        raise ValueError(f"read_wav: {channels} channels at {rate} Hz")
    if (tag, bits) not in ((WAVE_FORMAT_PCM, 8), (WAVE_FORMAT_PCM, 16), (WAVE_FORMAT_PCM, 24), (WAVE_FORMAT_PCM, 32),
                           (WAVE_FORMAT_IEEE_FLOAT, 32), (WAVE_FORMAT_IEEE_FLOAT, 64)):
        raise ValueError(f"read_wav: format tag {tag} (0x{tag:04X}) with {bits} bits per sample is not read: PCM 8 / 16 / 24 / 32 and "
                         "IEEE float 32 / 64 are")
    width = bits // 8
    n = len(data) // (width * channels)
    data = data[:n * width * channels]
    if tag == WAVE_FORMAT_IEEE_FLOAT:
        x = np.frombuffer(data, dtype="<f4" if bits == 32 else "<f8").astype(np.float32)
    elif bits == 8:
        x = (np.frombuffer(data, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif bits == 24:
        b = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = ((v ^ 0x800000) - 0x800000).astype(np.float64) / float(1 << 23)           # sign-extend
    else:
        x = np.frombuffer(data, dtype="<i2" if bits == 16 else "<i4").astype(np.float64) / float(1 << (bits - 1))
    return np.ascontiguousarray(x.astype(np.float32).reshape(n, channels)), int(rate)


# ----------------------------------------------------------------------------------------------------------------- filter design
def rate_ratio(in_rate: int, out_rate: int):
    """(up, down, half) of a rate pair: up / down = out_rate / in_rate in lowest terms, half = 10 * max(up, down)."""
    in_rate, out_rate = int(in_rate), int(out_rate)
    if in_rate < 1 or out_rate < 1:
        raise ValueError(f"sample rates must be positive, got {in_rate} -> {out_rate}")
    g = math.gcd(in_rate, out_rate)
    up, down = out_rate // g, in_rate // g
    if max(up, down) > MAX_RATE_FACTOR:
        raise ValueError(f"resampling {in_rate} -> {out_rate} Hz is the ratio {up}/{down}: a filter of {20 * max(up, down) + 1} taps; "
                         f"ratios up to {MAX_RATE_FACTOR} are served (resample to a standard rate first)")
    return up, down, 10 * max(up, down)


@functools.lru_cache(maxsize=32)
def resample_taps(in_rate: int, out_rate: int = TARGET_RATE):
    """The float64 filter of the rate pair: h[k + half] for k = -half .. half =
    fc * sinc(fc * k) * kaiser(2 * half + 1, 5.0)[k + half], fc = 1 / max(up, down), scaled so that sum(h) == up (read-only array;
    cached per pair).  sinc is taken as exactly 0 at the non-zero multiples of max(up, down), where sin(pi x) / (pi x) in floating point
    leaves 4e-17 - so that a pair with up == down == 1 is the identity."""
    up, down, half = rate_ratio(in_rate, out_rate)
    m = max(up, down)
    k = np.arange(-half, half + 1, dtype=np.int64)
    s = np.sinc(k.astype(np.float64) / m)
    s[(k % m == 0) & (k != 0)] = 0.0
    h = s / m * np.kaiser(2 * half + 1, KAISER_BETA)
    h *= up / h.sum()
    h.setflags(write=False)
    return h


def taps_per_phase(up: int, half: int) -> int:
    return -(-half // up) + half // up + 1


@functools.lru_cache(maxsize=32)
def _phase_table(in_rate: int, out_rate: int):
    up, down, half = rate_ratio(in_rate, out_rate)
    h = resample_taps(in_rate, out_rate).astype(np.float32)           # rounded once
    i0, tpp = -(-half // up), taps_per_phase(up, half)
    k = np.arange(up, dtype=np.int64)[:, None] + up * (np.arange(tpp, dtype=np.int64)[None, :] - i0)
    ok = np.abs(k) <= half
    tab = np.where(ok, h[np.clip(k + half, 0, 2 * half)], np.float32(0))
    return torch.from_numpy(np.ascontiguousarray(tab, dtype=np.float32))


def phase_table(in_rate: int, out_rate: int = TARGET_RATE) -> torch.Tensor:
    """The f32 taps in emo_audio_resample's layout, (up, taps_per_phase): entry [p][c] = h[p + up * (c - ceil(half / up))], 0 outside
    +-half.  Output n = (T0 * up + p) / down reads row p against frames T0 + ceil(half / up) - c."""
    return _phase_table(int(in_rate), int(out_rate))


# ----------------------------------------------------------------------------------------------------------------- device path
def prepare_waveform(audio, sample_rate: int, device="cuda") -> torch.Tensor:
    """(n,) or (n, channels) samples at `sample_rate` -> the encoder's `input_values`, (1, n_16k) f32 on the device: channel mean and
    resampling to 16 kHz in one emo_audio_resample launch (at 16 kHz: a one-tap table, a plain downmix), then emo_waveform_normalize."""
    x = torch.as_tensor(audio).detach()
    if x.dim() == 1:
        x = x[:, None]
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"prepare_waveform: expected (n,) or (n, channels) samples, got {tuple(x.shape)}")
    up, down, half = rate_ratio(sample_rate, TARGET_RATE)
    if up == down:
        taps, half = torch.ones(1, 1), 0
    else:
        taps = phase_table(sample_rate, TARGET_RATE)
    dev = torch.device(device)
    frames = x.to(dev, torch.float32).contiguous()
    y = ops.audio_resample(frames, taps.to(dev), up, down, half)
    return ops.waveform_normalize(y).reshape(1, -1)
