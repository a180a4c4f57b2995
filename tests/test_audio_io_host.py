"""Host-side checks of the audio front-end in front of wav2vec2 (no GPU): the WAV reader against files written with struct, the
resampling filter design against its float64 definition and scipy's resample_poly, the fps -> wav2vec2-frame index table against Fraction
arithmetic, and the argument checks of `__call__(head_rotation_speeds=)` with stubs."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from emote_hack_amd import audio_io
from emote_hack_amd.conditioning import audio_context_tokens, audio_frame_indices
from tests import audio_frontend_ref as R

FORMATS = [(R.PCM, 8), (R.PCM, 16), (R.PCM, 24), (R.PCM, 32), (R.FLOAT, 32), (R.FLOAT, 64)]


def _samples(tag, bits, n, channels, seed):
    """(values as written, the float32 frames the scaling rule gives)"""
    rng = np.random.default_rng(seed)
    if tag == R.FLOAT:
        v = rng.uniform(-1.5, 1.5, (n, channels)).astype(np.float32)           # float files may leave [-1, 1]
        return (v if bits == 32 else v.astype(np.float64)), v
    if bits == 8:
        v = rng.integers(0, 256, (n, channels))
        v[0, 0], v[1, 0] = 0, 255
        return v, ((v.astype(np.float64) - 128) / 128).astype(np.float32)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = rng.integers(lo, hi + 1, (n, channels))
    v[0, 0], v[1, 0], v[2, 0] = lo, hi, -1                                     # the extremes and a sign-extended -1
    return v, (v.astype(np.float64) / float(1 << (bits - 1))).astype(np.float32)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("tag,bits", FORMATS)
def test_read_wav_round_trip(tmp_path, tag, bits, channels):
    v, want = _samples(tag, bits, 37, channels, bits + channels)
    for ext in (False, True):
        got, rate = audio_io.read_wav(R.write_wav(tmp_path / f"a{int(ext)}.wav", v, 44100, tag, bits, extensible=ext))
        assert rate == 44100 and got.dtype == np.float32 and got.shape == (37, channels)
        assert np.array_equal(got, want)


def test_read_wav_chunk_walk_and_refusals(tmp_path):
    v, want = _samples(R.PCM, 16, 50, 2, 3)
    # a LIST chunk of odd size (pad byte) and an unknown chunk before data
    p = R.write_wav(tmp_path / "list.wav", v, 48000, R.PCM, 16, chunks_before_data=[(b"LIST", b"INFOISFT\x03\x00\x00\x00ab\x00"), (b"junk", b"1234567")])
    got, rate = audio_io.read_wav(p)
    assert rate == 48000 and np.array_equal(got, want)
    for size in (0xFFFFFFFF, 0):                                               # a streamed file: data runs to the end of the file
        got, _ = audio_io.read_wav(R.write_wav(tmp_path / "stream.wav", v, 48000, R.PCM, 16, data_size=size))
        assert np.array_equal(got, want)
    got, _ = audio_io.read_wav(str(R.write_wav(tmp_path / "str.wav", v[:, 0], 8000, R.PCM, 16)))      # a str path, mono
    assert got.shape == (50, 1) and np.array_equal(got[:, 0], want[:, 0])
    with pytest.raises(ValueError, match=r"format tag 2\b"):                   # MS ADPCM
        audio_io.read_wav(R.write_wav(tmp_path / "adpcm.wav", v, 8000, 2, 16))
    with pytest.raises(ValueError, match="format tag 1 .* 12 bits"):
        audio_io.read_wav(R.write_wav(tmp_path / "odd.wav", v, 8000, R.PCM, 12))
    (tmp_path / "not.wav").write_bytes(b"OggS" + bytes(40))
    with pytest.raises(ValueError, match="RIFF"):
        audio_io.read_wav(tmp_path / "not.wav")


@pytest.mark.parametrize("rate", R.RATES + (16000,))
def test_resample_taps_definition(rate):
    up, down, half = R.ratio(rate, 16000)
    assert audio_io.rate_ratio(rate, 16000) == (up, down, half)
    h = audio_io.resample_taps(rate, 16000)
    assert h.dtype == np.float64 and h.shape == (2 * half + 1,)
    assert abs(h.sum() - up) < 1e-12
    assert np.array_equal(h, h[::-1])
    np.testing.assert_allclose(h, R.taps_f64(rate, 16000), rtol=0, atol=1e-15)
    assert audio_io.resample_taps(rate, 16000) is h                            # cached per pair
    # the f32 phase table holds every tap once, in the kernel's layout
    tab = audio_io.phase_table(rate, 16000).numpy()
    i0 = -(-half // up)
    assert tab.shape == (up, i0 + half // up + 1) and tab.dtype == np.float32
    from emote_hack_amd import _lib
    assert _lib.load().emo_audio_resample_taps_per_phase(up, half) == tab.shape[1] == audio_io.taps_per_phase(up, half)      # the C entry sizes it alike
    h32 = h.astype(np.float32)
    seen = np.zeros(2 * half + 1, bool)
    for p in range(up):
        for c in range(tab.shape[1]):
            k = p + up * (c - i0)
            if abs(k) <= half:
                assert tab[p, c] == h32[k + half]
                seen[k + half] = True
            else:
                assert tab[p, c] == 0
    assert seen.all()
    if rate == 16000:
        assert np.array_equal(h, np.eye(1, 21, 10)[0])                         # the identity


@pytest.mark.parametrize("rate", R.RATES + (16000,))
def test_definition_equals_scipy_resample_poly(rate):
    signal = pytest.importorskip("scipy.signal")
    up, down, half = R.ratio(rate, 16000)
    h = R.taps_f64(rate, 16000)
    for n_in in (1, 7, 700):
        x = np.random.default_rng(n_in + rate).uniform(-1, 1, n_in)
        want = signal.resample_poly(x, up, down, window=("kaiser", 5.0), padtype="constant")
        got = R.resample_def(x, h, up, down, half)
        assert got.shape == want.shape == (math.ceil(n_in * up / down),)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_rate_pairs_past_the_table_limit_are_refused():
    with pytest.raises(ValueError, match="96001"):                             # coprime with 16000: down = 96001
        audio_io.resample_taps(96001, 16000)
    with pytest.raises(ValueError):
        audio_io.rate_ratio(16000, 65537)
    assert audio_io.rate_ratio(65536, 1)[:2] == (1, 65536)                     # the limit itself is served
    with pytest.raises(ValueError, match="positive"):
        audio_io.rate_ratio(0, 16000)


@pytest.mark.parametrize("fps", [25, 30, (30000, 1001)])
@pytest.mark.parametrize("start", [0, 0.37])
def test_fps_index_table(fps, start):
    F = 40
    want = R.fps_indices(F, fps, start)
    assert audio_frame_indices(F, fps, start) == want
    if not isinstance(fps, tuple):
        assert audio_frame_indices(F, Fraction(fps), Fraction(start)) == want
    # the table selects rows of the windows; a clip that outlasts the audio is refused, one that just fits is not
    Ta = want[-1] + 1
    win = torch.arange(Ta, dtype=torch.float32)[:, None].expand(Ta, 6).contiguous()
    tok = audio_context_tokens(win, F, 3, fps=fps, audio_start=start)
    assert tok.shape == (F, 2, 3) and tok[:, 0, 0].tolist() == [float(i) for i in want]
    with pytest.raises(ValueError, match="audio ends"):
        audio_context_tokens(win[:-1], F, 3, fps=fps, audio_start=start)
    with pytest.raises(ValueError, match="audio ends"):
        audio_frame_indices(F, fps, start, num_audio_frames=want[-1])
    # without fps the stretch rule is untouched
    assert audio_context_tokens(win, 4, 3)[:, 0, 0].tolist() == [float(i * Ta // 4) for i in range(4)]


def test_fps_table_is_exact_where_floats_are_not():
    """(i / fps) * 50 in floats lands below an integer for some i (e.g. fps = 30000 / 1001); the table is rational arithmetic."""
    fps = (30000, 1001)
    want = R.fps_indices(3001, fps, 0)
    assert audio_frame_indices(3001, fps, 0) == want
    assert want[3000] == 5005 and want[600] == 1001                            # i * 1001 / 600 at multiples of 600: exact integers


# ---------------------------------------------------------------- __call__(head_rotation_speeds=) with stubs
class _Stop(Exception):
    pass


def _pipe(monkeypatch, seen):
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests.test_clip_vision_host import _pipe as stub_pipe

    def fake_denoise(self, lat, ref, text, **kw):
        seen.update(kw)
        raise _Stop

    monkeypatch.setattr(EMOAnimationPipeline, "denoise", fake_denoise)
    p = stub_pipe()
    p.unet = SimpleNamespace(config=SimpleNamespace(sample_size=2, block_out_channels=(8, 16)), device=torch.device("cpu"), in_channels=4)
    p.controlnet, p.vae, p.vae_scale_factor = None, None, 8
    p.scheduler = SimpleNamespace(init_noise_sigma=1.0)
    return p


class StubSpeedEncoder:
    def __init__(self, dim):
        self.speed_embedding_dim = dim
        self.seen = []

    def __call__(self, v):
        self.seen.append(v)
        return v[:, None] * torch.ones(1, self.speed_embedding_dim)


def test_call_head_rotation_speeds_argument_checks(monkeypatch):
    seen = {}
    p = _pipe(monkeypatch, seen)
    kw = dict(appearance_encoder=object(), ref_image_latents=torch.zeros(1, 4, 2, 2), latents=torch.zeros(1, 4, 2, 2, 2),
              text_embeddings=torch.zeros(2, 1, 5))
    with pytest.raises(ValueError, match="speed_encoder"):                     # (the stub pipeline is built without __init__)
        p("", 2, head_rotation_speeds=0.3, **kw)
    p.speed_encoder = None
    with pytest.raises(ValueError, match="speed_encoder"):
        p("", 2, head_rotation_speeds=0.3, **kw)
    p.speed_encoder = StubSpeedEncoder(64)
    with pytest.raises(ValueError, match=r"SpeedEncoder\(9, 32\)"):            # the UNet's time embedding is 4 * 8 wide
        p("", 2, head_rotation_speeds=0.3, **kw)
    p.speed_encoder = StubSpeedEncoder(32)
    with pytest.raises(ValueError, match="ONE speed per clip"):
        p("", 2, head_rotation_speeds=torch.tensor([0.1, 0.2]), **kw)
    with pytest.raises(ValueError, match="ONE speed per clip"):
        p("", 2, head_rotation_speeds=[0.1, 0.2, 0.3], **kw)
    for v in (0.3, torch.tensor([0.3]), torch.tensor(0.3)):
        seen.clear()
        with pytest.raises(_Stop):
            p("", 2, head_rotation_speeds=v, **kw)
        arg = p.speed_encoder.seen[-1]
        assert arg.dtype == torch.float32 and arg.shape == (1,) and float(arg) == float(torch.tensor(0.3))
        assert seen["speed_embeddings"].shape == (1, 32)
    # an explicit speed_embeddings= takes precedence: the encoder is not called
    n = len(p.speed_encoder.seen)
    given = torch.full((1, 32), 7.0)
    with pytest.raises(_Stop):
        p("", 2, head_rotation_speeds=0.3, speed_embeddings=given, **kw)
    assert len(p.speed_encoder.seen) == n and seen["speed_embeddings"] is given


def test_ctor_takes_a_speed_encoder():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    unet = SimpleNamespace(device=torch.device("cpu"))
    assert EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler()).speed_encoder is None
    enc = StubSpeedEncoder(32)
    assert EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler(), speed_encoder=enc).speed_encoder is enc


def test_call_audio_argument_forms(monkeypatch, tmp_path):
    """audio= as a path, a (samples, rate) pair and a bare waveform reach the extractor as the issue states; no extractor, a rate beside a
    path and a disagreeing rate are ValueErrors."""
    seen = {}
    p = _pipe(monkeypatch, seen)

    class StubExtractor:
        sampling_rate = 16000
        model = SimpleNamespace(config=SimpleNamespace(hidden_size=3, conv_stride=(5, 2, 2, 2, 2, 2, 2)))

        def __init__(self):
            self.calls = []

        def extract_features(self, audio, m=2, n=2, sample_rate=None):
            self.calls.append(("array", sample_rate))
            return torch.arange(20, dtype=torch.float32)[:, None].expand(20, 15).contiguous()

        def extract_features_from_wav(self, path, m=2, n=2):
            self.calls.append(("wav", path))
            return self.extract_features(None)

        def extract_features_from_mp4(self, path, m=2, n=2):
            self.calls.append(("mp4", path))
            return self.extract_features(None)

    fx = StubExtractor()
    kw = dict(appearance_encoder=object(), ref_image_latents=torch.zeros(1, 4, 2, 2), latents=torch.zeros(1, 4, 2, 2, 2),
              text_embeddings=torch.zeros(2, 1, 5), feature_extractor=fx)
    wave = np.zeros(100, np.float32)

    def run(**extra):
        fx.calls.clear()
        with pytest.raises(_Stop):
            p("", 2, **dict(kw, **extra))
        return list(fx.calls), seen["audio_features"]

    assert run(audio=wave)[0] == [("array", None)]                             # bare: 16 kHz, the host path as before
    assert run(audio=wave, audio_sample_rate=44100)[0] == [("array", 44100)]
    assert run(audio=(wave, 48000))[0] == [("array", 48000)]
    assert run(audio=(wave, np.int64(16000)))[0] == [("array", 16000)]
    assert run(audio=str(tmp_path / "a.WAV"))[0][0] == ("wav", str(tmp_path / "a.WAV"))
    assert run(audio=tmp_path / "a.wav")[0][0] == ("wav", str(tmp_path / "a.wav"))
    assert run(audio=str(tmp_path / "clip.mp4"))[0][0] == ("mp4", str(tmp_path / "clip.mp4"))
    calls, feats = run(audio=wave, fps=25, audio_start=0.1)                    # frames 5, 7 of 20 at 50 Hz
    assert feats.shape == (2, 5, 3) and feats[:, 0, 0].tolist() == [5.0, 7.0]
    assert run(audio=wave)[1][:, 0, 0].tolist() == [0.0, 10.0]                 # without fps: stretched over the clip
    with pytest.raises(ValueError, match="audio ends"):
        p("", 2, audio=wave, fps=2, audio_start=0.1, **kw)
    with pytest.raises(ValueError, match="carries its own"):
        p("", 2, audio="a.wav", audio_sample_rate=16000, **kw)
    with pytest.raises(ValueError, match="disagree"):
        p("", 2, audio=(wave, 48000), audio_sample_rate=16000, **kw)
    with pytest.raises(ValueError, match="feature_extractor"):
        p("", 2, audio=wave, **{k: v for k, v in kw.items() if k != "feature_extractor"})


def test_extract_features_from_mp4_needs_the_wav_beside_it(tmp_path):
    from emote_hack_amd.wav2vec2 import Wav2VecFeatureExtractor
    fx = Wav2VecFeatureExtractor(model=None, device="cpu")
    with pytest.raises(ValueError, match="demuxing"):
        fx.extract_features_from_mp4(str(tmp_path / "clip.mp4"))
    seen = []
    fx.extract_features = lambda audio, m, n, sample_rate=None: seen.append((audio.shape, sample_rate)) or "features"
    R.write_wav(tmp_path / "clip.wav", np.zeros((30, 2), np.int16), 22050, R.PCM, 16)
    assert fx.extract_features_from_mp4(tmp_path / "clip.mp4") == "features" and seen == [((30, 2), 22050)]
    assert fx.extract_features_from_wav(tmp_path / "clip.wav", 1, 1) == "features" and seen[-1] == ((30, 2), 22050)
