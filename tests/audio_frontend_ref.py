"""Float64 restatements of the audio front-end's definitions (emote_hack_amd/audio_io.py, emo_audio_resample, emo_waveform_normalize)
and a WAV writer, shared by tests/test_audio_io_host.py and tests/test_gpu_audio_frontend.py.  Nothing here imports the package: these
are the definitions the product is compared against, written out on their own.

  resampling   g = gcd(in_rate, out_rate), up = out_rate / g, down = in_rate / g, half = 10 * max(up, down), fc = 1 / max(up, down)
               h[k] = fc * sinc(fc * k) * kaiser(2 * half + 1, 5.0)[k + half] for k = -half .. half, scaled so that sum(h) == up
               y[n] = sum_j h[n * down - j * up] * x[j] over |n * down - j * up| <= half, x[j] = mean over channels, 0 outside the utterance
               len(y) = ceil(n_in * up / down)
  normalising  (x - mean) / sqrt(var + 1e-7), population variance
  fps table    video frame i -> wav2vec2 frame floor((audio_start + i / fps) * 16000 / prod(conv_stride))
"""
import math
import struct
from fractions import Fraction

import numpy as np

RATES = (44100, 48000, 22050, 11025, 8000)


def ratio(in_rate, out_rate):
    g = math.gcd(in_rate, out_rate)
    up, down = out_rate // g, in_rate // g
    return up, down, 10 * max(up, down)


def taps_f64(in_rate, out_rate):
    up, down, half = ratio(in_rate, out_rate)
    fc = 1.0 / max(up, down)
    k = np.arange(-half, half + 1)
    h = fc * np.sinc(fc * k) * np.kaiser(2 * half + 1, 5.0)
    return h * (up / h.sum())


def downmix_f64(frames):
    f = np.asarray(frames, dtype=np.float64)
    return f if f.ndim == 1 else f.sum(axis=1) / f.shape[1]


def out_len(n_in, up, down):
    return -(-n_in * up // down)


def resample_def(x, h, up, down, half, n0=0, n_out=None, j0=0):
    """y[n0 .. n0 + n_out) of the definition, float64.  x holds the mono samples of GLOBAL frames j0 .. j0 + len(x) - 1 (zero elsewhere);
    h has 2 * half + 1 taps.  Python integers for n * down: no overflow."""
    x = np.asarray(x, dtype=np.float64)
    if n_out is None:
        n_out = out_len(len(x), up, down)
    y = np.zeros(n_out)
    for i in range(n_out):
        t = (n0 + i) * down
        j = np.arange(-((half - t) // up), (t + half) // up + 1)          # ceil((t - half) / up) .. floor((t + half) / up)
        loc = j - j0
        ok = (loc >= 0) & (loc < len(x))
        y[i] = np.sum(h[(t - j[ok] * up) + half] * x[loc[ok]])
    return y


def normalize_def(x):
    x = np.asarray(x, dtype=np.float64)
    return (x - x.mean()) / np.sqrt(x.var() + 1e-7)


def normalize_tol(x):
    """64 * 2^-24 * (1 + |mean| / sqrt(var + 1e-7)) * max(1, max |y_ref|) from the input's float64 statistics: 64 f32 roundoffs of
    headroom on a result whose conditioning is the offset over the spread."""
    x = np.asarray(x, dtype=np.float64)
    s = np.sqrt(x.var() + 1e-7)
    return 64 * 2.0 ** -24 * (1 + abs(x.mean()) / s) * max(1.0, float(np.abs(normalize_def(x)).max()))


def fps_indices(n_frames, fps, audio_start, samples_per_frame=320, rate=16000):
    fps, t0 = Fraction(*fps) if isinstance(fps, tuple) else Fraction(fps), Fraction(audio_start)
    return [math.floor((t0 + Fraction(i) / fps) * Fraction(rate, samples_per_frame)) for i in range(n_frames)]


# ---------------------------------------------------------------------------------------------------------------------- WAV writer
PCM, FLOAT, EXTENSIBLE = 1, 3, 0xFFFE
_GUID_TAIL = bytes.fromhex("000000001000800000AA00389B71")


def encode_samples(values, tag, bits):
    """values (n, channels): integers for PCM (8-bit: 0 .. 255 unsigned), floats for IEEE float -> little-endian interleaved bytes."""
    v = np.asarray(values)
    if tag == FLOAT:
        return v.astype("<f4" if bits == 32 else "<f8").tobytes()
    if bits == 8:
        return v.astype(np.uint8).tobytes()
    if bits == 24:
        return b"".join(struct.pack("<i", int(s))[:3] for s in v.reshape(-1))
    return v.astype("<i2" if bits == 16 else "<i4").tobytes()


def write_wav(path, values, rate, tag, bits, extensible=False, chunks_before_data=(), data_size=None):
    """A RIFF/WAVE file written with struct.  chunks_before_data: (id, payload) pairs put between fmt and data (an odd payload gets its pad
    byte); data_size overrides the data chunk's size field (0xFFFFFFFF or 0: a streamed file)."""
    v = np.asarray(values)
    channels = 1 if v.ndim == 1 else v.shape[1]
    data = encode_samples(v.reshape(-1, channels), tag, bits)
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", EXTENSIBLE if extensible else tag, channels, rate, rate * align, align, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, (1 << channels) - 1) + struct.pack("<H", tag) + _GUID_TAIL
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for cid, payload in chunks_before_data:
        body += cid + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path
