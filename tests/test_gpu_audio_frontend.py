"""GPU checks of the signal path in front of wav2vec2 (Net.py:627-640): emo_audio_resample and emo_waveform_normalize against their
float64 definitions (tests/audio_frontend_ref.py), the feature extractor's file / any-rate entry points, and the pipeline's `audio=` path /
`fps=` / `head_rotation_speeds=` inputs against the same call fed with explicit features / embeddings.

Tolerances (from the arithmetic, not from the code under test):
  resampler   atol 1e-5, rtol 0: at most 62 taps per output, f32 unit roundoff 2^-24, per-phase sum |h| <= 2.3, inputs in [-1, 1]:
              62 * 2^-24 * 2.3 = 8.5e-6 (a sequential f32 emulation errs by 2.6e-7).
              Observed on MI355X, max |y - y_def| over n_in {1, 7, 1500} x channels {1, 2, 3}: 44100 Hz 2.1e-7, 48000 Hz 3.4e-7,
              22050 Hz 2.5e-7, 11025 Hz 3.4e-7, 8000 Hz 2.9e-7; the 64-bit index case 2.0e-7.
  normaliser  64 * 2^-24 * (1 + |mean| / sqrt(var + 1e-7)) * max(1, max |y_ref|) from the input's float64 statistics.
              Observed on MI355X (error / bound): n = 2 7.3e-8 / 5.6e-6, n = 255 2.5e-7 / 9.9e-6, n = 256 3.0e-7 / 1.3e-5,
              n = 257 2.3e-7 / 1.2e-5, n = 100003 3.9e-7 / 1.8e-5, the DC case (mean 0.9, sigma 0.001) 1.9e-5 / 1.4e-2.
"""
import numpy as np
import pytest
import torch

from emote_hack_amd.synth import seeded_randn
from tests import audio_frontend_ref as R
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _frames(n, channels, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, channels)).astype(np.float32)


def _resample(frames, rate, **kw):
    from emote_hack_amd import audio_io, ops
    up, down, half = audio_io.rate_ratio(rate, 16000)
    return ops.audio_resample(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV), audio_io.phase_table(rate, 16000).to(DEV), up, down, half, **kw)


def _h32(rate):
    return R.taps_f64(rate, 16000).astype(np.float32).astype(np.float64)          # the definition's taps: float64 design, rounded once to f32


# ------------------------------------------------------------------------------------------------------------------ the resampler
@pytest.mark.parametrize("rate", R.RATES)
def test_resampler_vs_float64_definition(rate):
    up, down, half = R.ratio(rate, 16000)
    h, worst = _h32(rate), 0.0
    for n_in in (1, 7, 1500):                                                      # 1 and 7 are shorter than the filter
        for channels in (1, 2, 3):
            f = _frames(n_in, channels, rate + 10 * n_in + channels)
            y = _resample(f, rate).cpu().numpy()
            assert y.shape == (-(-n_in * up // down),) and y.dtype == np.float32
            err = float(np.abs(y - R.resample_def(R.downmix_f64(f), h, up, down, half)).max())
            print(f"resample {rate} -> 16000 n_in={n_in} channels={channels}: max err {err:.3e}")
            worst = max(worst, err)
    print(f"resample {rate} -> 16000: worst {worst:.3e}")
    assert worst <= 1e-5


def test_resampler_at_16k_is_the_channel_mean_bit_for_bit():
    from emote_hack_amd import audio_io, ops
    f = _frames(1500, 2, 5)
    want = (f[:, 0] + f[:, 1]) / np.float32(2)
    assert np.array_equal(_resample(f, 16000).cpu().numpy(), want)                # the designed 21-tap filter of 16000 -> 16000
    one_tap = ops.audio_resample(torch.from_numpy(f).to(DEV), torch.ones(1, 1, device=DEV), 1, 1, 0)    # what prepare_waveform launches
    assert np.array_equal(one_tap.cpu().numpy(), want)
    got = audio_io.prepare_waveform(f, 16000, DEV)
    assert got.shape == (1, 1500) and torch.equal(got[0], ops.waveform_normalize(torch.from_numpy(want).to(DEV)))
    f3 = _frames(300, 3, 6)
    want3 = ((f3[:, 0] + f3[:, 1]) + f3[:, 2]) / np.float32(3)                     # summed in channel order, one division
    assert np.array_equal(_resample(f3, 16000).cpu().numpy(), want3)


def test_resampler_in_pieces_is_bit_identical():
    """The 1500-frame 44.1 kHz case as three unequal output ranges, each from the input slice that covers its taps (plus margin)."""
    rate, f = 44100, _frames(1500, 2, 44100 + 15000 + 2)
    up, down, half = R.ratio(rate, 16000)
    whole = _resample(f, rate)
    n_out = whole.numel()
    parts = []
    for a, b in ((0, 100), (100, 133), (133, n_out)):
        lo = max((a * down - half) // up - 3, 0)
        hi = min(((b - 1) * down + half) // up + 4, len(f))
        parts.append(_resample(f[lo:hi], rate, in_start=lo, out_start=a, n_out=b - a))
    assert torch.equal(torch.cat(parts), whole)
    # a slice that starts exactly at the first tap and ends exactly at the last one
    a, b = 200, 260
    lo, hi = -((half - a * down) // up), ((b - 1) * down + half) // up + 1
    assert torch.equal(_resample(f[lo:hi], rate, in_start=lo, out_start=a, n_out=b - a), whole[a:b])


def test_resampler_indices_past_2_31():
    """64 outputs from n = 2^31 // 441 + 17 on (n * down > 2^31: five minutes into a 44.1 kHz recording) from a 400-frame slice at the
    matching global index, against the definition evaluated at those global indices.  32-bit index arithmetic fails this."""
    rate = 44100
    up, down, half = R.ratio(rate, 16000)
    n0 = 2 ** 31 // 441 + 17
    assert n0 * down > 2 ** 31 and (up, down) == (160, 441)
    j0 = -((half - n0 * down) // up) - 20                                          # 20 frames before the first tap of output n0
    assert ((n0 + 63) * down + half) // up < j0 + 400
    f = _frames(400, 2, 31)
    y = _resample(f, rate, in_start=j0, out_start=n0, n_out=64).cpu().numpy()
    ref = R.resample_def(R.downmix_f64(f), _h32(rate), up, down, half, n0=n0, n_out=64, j0=j0)
    err = float(np.abs(y - ref).max())
    print(f"resample at n0 = {n0}: max err {err:.3e}, max |y| {float(np.abs(ref).max()):.3f}")
    assert np.abs(ref).max() > 0.1 and err <= 1e-5


def test_resampler_refuses_a_table_of_the_wrong_size():
    from emote_hack_amd import ops
    from emote_hack_amd._lib import EmoHipError
    f = torch.zeros(10, 1, device=DEV)
    with pytest.raises(EmoHipError, match="phase table"):
        ops.audio_resample(f, torch.ones(160, 55, device=DEV), 160, 441, 4410)    # 160 x 56 is the table of 44100 -> 16000


# ------------------------------------------------------------------------------------------------------------------ the normaliser
NORM_CASES = [(2, 0.0, 0.1), (255, 0.0, 0.1), (256, 0.0, 0.1), (257, 0.0, 0.1), (100003, 0.0, 0.1), (100003, 0.9, 0.001)]


@pytest.mark.parametrize("n,mean,sigma", NORM_CASES)
def test_normaliser_vs_float64(n, mean, sigma):
    from emote_hack_amd import ops
    x = (mean + sigma * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    y = ops.waveform_normalize(xd)
    ref, tol = R.normalize_def(x), R.normalize_tol(x)
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print(f"normalise n={n} mean={mean} sigma={sigma}: max err {err:.3e}, bound {tol:.3e}")
    assert y.shape == xd.shape and y.dtype == torch.float32 and err <= tol
    assert torch.equal(ops.waveform_normalize(xd), y)                              # a fixed reduction order: the same bits every run


def test_normaliser_refuses_a_short_workspace():
    from emote_hack_amd import _lib, ops
    from emote_hack_amd._lib import EmoHipError
    n = 100003
    need = _lib.load().emo_waveform_normalize_workspace_bytes(n)
    assert need >= 8 and need % 4 == 0
    x = torch.zeros(n, device=DEV)
    ops.waveform_normalize(x, workspace=torch.empty(need // 4, device=DEV))        # exactly enough
    with pytest.raises(EmoHipError, match="workspace"):
        ops.waveform_normalize(x, workspace=torch.empty(need // 4 - 1, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ the front-end
def _model(cfg, dtype=torch.float32):
    from emote_hack_amd.wav2vec2 import Wav2Vec2Model, wav2vec2_synth_state_dict
    m = Wav2Vec2Model(cfg)
    m.load_state_dict(wav2vec2_synth_state_dict(cfg))
    return m.to(DEV, dtype)


@pytest.fixture(scope="module")
def fx():
    from emote_hack_amd.wav2vec2 import Wav2VecFeatureExtractor
    return Wav2VecFeatureExtractor(_model(cases.WAV2VEC2_TINY), DEV)


def _pcm16(n, channels, seed):
    """16-bit samples and the float frames a reader gives for them"""
    v = np.random.default_rng(seed).integers(-20000, 20000, (n, channels))
    return v, (v / 32768.0).astype(np.float32)


def test_extract_features_at_a_rate_runs_the_device_front_end(fx, tmp_path):
    from emote_hack_amd import audio_io
    from emote_hack_amd.conditioning import audio_windows
    v, frames = _pcm16(11025, 2, 7)                                                 # 0.25 s of stereo 44.1 kHz -> 4000 samples
    feats = fx.extract_features(frames, m=2, n=2, sample_rate=44100)
    iv = audio_io.prepare_waveform(frames, 44100, DEV)
    assert iv.shape == (1, 4000) and feats.shape == (12, 5 * 64)
    assert torch.equal(feats, audio_windows(fx.model(iv).last_hidden_state, 2, 2))
    assert abs(float(iv.mean())) < 1e-5 and abs(float(iv.var(unbiased=False)) - 1) < 1e-3
    path = R.write_wav(tmp_path / "a.wav", v, 44100, R.PCM, 16)
    decoded, rate = audio_io.read_wav(path)
    assert rate == 44100 and np.array_equal(decoded, frames)
    assert torch.equal(fx.extract_features_from_wav(path), feats)
    assert torch.equal(fx.extract_features_from_wav(str(path), m=2, n=2), fx.extract_features_from_wav(decoded, sample_rate=rate))
    assert torch.equal(fx.extract_features_from_mp4(tmp_path / "a.mp4"), feats)     # the .wav beside the video
    # a rate of 16000 also takes the device path: the normalisation kernel instead of the host statement, the same features to rounding
    w = 0.5 * seeded_randn((4000,), 501)
    torch.testing.assert_close(fx.extract_features(w, sample_rate=16000), fx.extract_features(w), rtol=1e-3, atol=1e-4)


def test_extract_features_without_a_rate_is_the_old_path(fx):
    """No sample_rate: the host statements of the parent commit, bit for bit (restated here), and through the committed goldens."""
    import os

    from safetensors.torch import load_file

    from emote_hack_amd.conditioning import audio_windows
    from emote_hack_amd.wav2vec2 import Wav2VecFeatureExtractor, normalize_waveform
    w = 0.5 * seeded_randn((4000,), 501)
    old = audio_windows(fx.model(normalize_waveform(w).to(DEV)).last_hidden_state, 2, 2)
    assert torch.equal(fx.extract_features(w), old) and torch.equal(fx.extract_features_from_wav(w, 2, 2), old)
    st = torch.stack([w * 1.5, w * 0.5], 1)
    assert torch.equal(fx.extract_features(st), audio_windows(fx.model(normalize_waveform(st.mean(dim=1)).to(DEV)).last_hidden_state, 2, 2))
    gold = load_file(os.path.join(cases.GOLDEN_DIR, "wav2vec2.safetensors"))
    wave = 0.1 * seeded_randn((16000,), 502) + 0.05 * torch.sin(torch.arange(16000) * 0.05)
    base = Wav2VecFeatureExtractor(_model({}), DEV)
    torch.testing.assert_close(base.extract_features(wave, m=2, n=2).float().cpu(), gold["base/features"], rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def pipe_kw():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.appearance_encoder import AppearanceEncoderModel
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests.test_gpu_unet import build
    unet = build(dict(cases.TINY_MOTION, cross_attention_dim=64), torch.float32)
    ref = build(dict(cases.TINY, cross_attention_dim=64), torch.float32, cases.REF_PREFIX, cls=AppearanceEncoderModel, has_out=False)
    pipe = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler())
    kw = dict(video_length=4, height=128, width=128, num_inference_steps=2, guidance_scale=7.5, context_frames=4, context_stride=1,
              context_overlap=0, output_type="latent", appearance_encoder=ref, text_embeddings=seeded_randn((2, 5, 64), 2),
              ref_image_latents=seeded_randn((1, 4, 16, 16), 3), latents=seeded_randn((1, 4, 4, 16, 16), 1).to(DEV), seed=0)
    return pipe, kw


def test_pipeline_call_takes_an_audio_file_and_fps(fx, pipe_kw, tmp_path):
    """pipe(audio=path, fps=25) == pipe(audio_features=) with the features built from the public pieces: read_wav -> prepare_waveform ->
    model -> audio_windows -> the fps index table."""
    from emote_hack_amd import audio_io
    from emote_hack_amd.conditioning import audio_frame_indices, audio_windows
    pipe, kw = pipe_kw
    v, frames = _pcm16(11025, 2, 8)
    path = str(R.write_wav(tmp_path / "speech.wav", v, 44100, R.PCM, 16))
    a = pipe("", audio=path, fps=25, feature_extractor=fx, **kw).videos
    samples, rate = audio_io.read_wav(path)
    windows = audio_windows(fx.model(audio_io.prepare_waveform(samples, rate, DEV)).last_hidden_state, 2, 2)
    idx = audio_frame_indices(4, 25, 0, windows.shape[0])
    assert idx == [0, 2, 4, 6] and windows.shape[0] == 12
    feats = windows[torch.tensor(idx, device=windows.device)].reshape(4, 5, 64)
    b = pipe("", audio_features=feats, **kw).videos
    assert torch.equal(a, b)
    assert torch.equal(pipe("", audio=(frames, 44100), fps=25, feature_extractor=fx, **kw).videos, a)      # the (samples, rate) pair
    c = pipe("", audio=path, fps=(30000, 1001), audio_start=0.1, feature_extractor=fx, **kw).videos       # other frames: other latents
    assert float((a - c).abs().max()) > 1e-4
    with pytest.raises(ValueError, match="audio ends"):
        pipe("", audio=path, fps=25, audio_start=0.2, feature_extractor=fx, **kw)


def test_pipeline_call_takes_head_rotation_speeds(pipe_kw):
    from emote_hack_amd.conditioning import SpeedEncoder
    from tests.test_gpu_conditioning import mk
    pipe, kw = pipe_kw
    enc = mk(SpeedEncoder, "speed_encoder.", 9, 4 * cases.TINY["block_out_channels"][0])
    with pytest.raises(ValueError, match="speed_encoder"):
        pipe("", head_rotation_speeds=0.3, **kw)
    pipe.speed_encoder = enc
    try:
        a = pipe("", head_rotation_speeds=0.3, **kw).videos
        b = pipe("", speed_embeddings=enc(torch.tensor([0.3])), **kw).videos
        assert torch.equal(a, b)
        assert torch.equal(pipe("", head_rotation_speeds=torch.tensor([0.3]), **kw).videos, a)
        assert float((a - pipe("", **kw).videos).abs().max()) > 1e-4           # the speed embedding is live
    finally:
        pipe.speed_encoder = None
