"""GPU sweeps of the small front-end kernels over what raw inputs can be - audio of any length, images of any size:
emo_channelnorm (csrc/frontend.hip) over its chunk split, the caps of both passes, fewer rows than row lanes, ragged channel slabs and
padded leading dimensions; emo_audio_windows up to the second trip of its grid; the wav2vec2 encoder at utterance lengths that leave
one frame, two, an odd remainder at every layer; emo_image_preprocess (csrc/vision.hip) at strong shrinks, frames below the filter
support, extreme aspect ratios and other crop sizes; emo_vision_embed up to its last register slot.  The case tables are
tests/frontend_sweep_cases.py.  The C entries are called directly where the ops wrapper offers no leading dimensions.

References are f64 evaluations on inputs already quantised to the compute dtype; tolerances are the tables of tests/test_gpu_kernels.py
(TOL), tests/test_gpu_clip_text.py (its TOL, as test_vision_embed uses) and tests/test_gpu_clip_vision.py (RTOL / ATOL); the parity
groups print the largest error as a fraction of the tolerance before they assert it (pytest -s shows the figures).  The exact groups
(the +-1 statistics probe, run-to-run identity, the index kernels, batches) compare bits."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from emote_hack_amd.synth import seeded_randn
from tests import cases
from tests import frontend_sweep_cases as S
from tests.test_gpu_clip_text import TOL as TOL_CLIP
from tests.test_gpu_clip_vision import ATOL, RTOL, definition_pixels
from tests.test_gpu_gemm_sweeps import DEV, IDS, bits, sentinel, untouched
from tests.test_gpu_kernels import TOL, ops

pytestmark = pytest.mark.gpu

EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))       # the value the entries receive (float eps)
EMO_ERR_UNSUPPORTED = -3


def dti(dtype):
    return {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    from emote_hack_amd import _lib
    return _lib.load()


def nan_cols(t, ld):
    """t (rows, w) on the device as a column view of a (rows, ld) buffer whose padding is NaN"""
    buf = torch.full((t.shape[0], ld), float("nan"), device=DEV, dtype=t.dtype)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def sentinel_cols(rows, w, ld, dtype, rows_behind=2):
    """a (rows, w) output view of a sentinel-filled (rows + rows_behind, ld) buffer and the mask of what must keep its bits"""
    buf = sentinel((rows + rows_behind, ld), dtype)
    keep = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    keep[:rows, :w] = False
    return buf, buf[:rows, :w], keep


def within(label, got, ref64, tol):
    """the assert_close condition |got - ref| <= atol + rtol * |ref|, as the largest error over its tolerance"""
    g = got.double()
    assert g.shape == ref64.shape and bool(torch.isfinite(g).all()), (label, "shape / not finite")
    f = float(((g - ref64).abs() / (tol["atol"] + tol["rtol"] * ref64.abs())).max())
    print(f"frontend-sweep {label} | {f:.4f} of tolerance")
    assert f <= 1.0, (label, f)


# ------------------------------------------------------------------------------------------------------------------ emo_channelnorm
def channelnorm(x, gamma, beta, y, act, S_, C_, dtype, ws=None):
    L = lib()
    n = L.emo_channelnorm_workspace_bytes(S_, C_) // 4
    assert n == S.cn_chunks(S_)[0] * C_ * 2
    if ws is None:
        ws = torch.full((n + 64,), float("nan"), device=DEV, dtype=torch.float32)       # a partial nobody wrote shows
    rc = L.emo_channelnorm(x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), y.stride(0), S_, C_, EPS, int(act),
                           ws.data_ptr(), dti(dtype), stream())
    assert rc == 0, rc
    return ws


def cn_rows(S_, C_, dtype, seed):
    return (seeded_randn((S_, C_), seed) * 2 + 0.3).to(dtype)


@pytest.mark.parametrize("S_", S.CN_S)
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_channelnorm_rows_channels_and_leading_dimensions(dtype, S_):
    """S x C in {1, 63, 64, 65, 130} x GELU on / off, ldx = C + 3 with NaN padding, ldy = C + 5 with sentinel padding that must survive,
    against (x - mean) / sqrt(var + eps) * gamma + beta (biased variance) written out in f64; S = 1 gives beta.
    (S = 2, C = 63 in f32 is the case that found sum(x^2) / S - mean^2 on the raw values losing a small variance - two rows 0.01 apart:
    16.5 x the tolerance; the kernel now sums x - x[0, c].)"""
    for C_ in S.CN_C:
        xq = cn_rows(S_, C_, dtype, 100 + C_)
        gamma, beta = 1 + 0.1 * seeded_randn((C_,), 8), 0.1 * seeded_randn((C_,), 9)
        x64 = xq.double()
        mean, var = x64.mean(0), x64.var(0, unbiased=False)
        ref = (x64 - mean) / torch.sqrt(var + EPS32) * gamma.double() + beta.double()
        if S_ == 1:
            assert torch.equal(ref, beta.double()[None])
        x = nan_cols(xq, C_ + S.CN_PAD[0])
        for gelu in (False, True):
            buf, y, keep = sentinel_cols(S_, C_, C_ + S.CN_PAD[1], dtype)
            channelnorm(x, gamma.to(DEV), beta.to(DEV), y, gelu, S_, C_, dtype)
            assert untouched(buf, keep), (S_, C_, gelu, "wrote outside the S x C view")
            want = 0.5 * ref * (1 + torch.erf(ref / math.sqrt(2.0))) if gelu else ref
            within(f"channelnorm S={S_} C={C_} gelu={int(gelu)} {IDS[dtype]}", y.float().cpu(), want, TOL[dtype])


@pytest.mark.parametrize("S_", S.CN_PROBE_S)
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_channelnorm_exact_statistics_probe(dtype, S_):
    """x = +1 on a seeded half of the rows of each channel, -1 on the rest: every partial sum is an exact integer, the mean is 0 and
    the variance 1, so y = beta +- f32(f32(1 / sqrt(1 + eps)) * gamma), rounded once more for the 2-byte types - BIT FOR BIT.  One
    row or chunk dropped or counted twice moves the mean and the bits; the bf16 tolerance would hide a lost chunk of 33000 rows."""
    n, per, nb = S.cn_chunks(S_)
    assert S_ % 2 == 0 and (n - 1) * per < S_
    rstd = torch.tensor(1.0 / math.sqrt(1.0 + EPS32), dtype=torch.float64).float()
    for C_ in S.CN_C:
        g = torch.Generator().manual_seed(S_ + C_)
        sign = torch.stack([torch.randperm(S_, generator=g) for _ in range(C_)], 1) < S_ // 2      # (S, C): half of each column
        xq = (sign.float() * 2 - 1).to(dtype)
        assert bool((xq.float().sum(0) == 0).all())
        gamma, beta = 1 + 0.1 * seeded_randn((C_,), 18), 0.1 * seeded_randn((C_,), 19)
        k = rstd * gamma                                                              # one f32 product
        want = (beta[None] + xq.float() * k[None]).to(dtype)                          # +-1 * k is exact: one f32 sum, one rounding to dtype
        buf, y, keep = sentinel_cols(S_, C_, C_ + S.CN_PAD[1], dtype)
        channelnorm(nan_cols(xq, C_ + S.CN_PAD[0]), gamma.to(DEV), beta.to(DEV), y, False, S_, C_, dtype)
        assert untouched(buf, keep), (S_, C_)
        bad = bits(y.cpu().contiguous()) != bits(want)
        assert not bool(bad.any()), (f"S={S_} C={C_} {IDS[dtype]} ({n} chunks of {per}, {nb} apply blocks): {int(bad.sum())} of {bad.numel()} "
                                     f"elements differ, first at {bad.nonzero()[0].tolist()}: got {y.cpu()[bad][0].item()} want {want[bad][0].item()}")


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_channelnorm_same_bits_from_run_to_run(dtype):
    """the partials are re-reduced in chunk order by every apply block (include/emo_hip.h): two calls on the same rows, the second on
    a workspace that still holds the first call's partials, return the same bits"""
    for S_, C_ in ((33000, 130), (513, 65)):
        x = cn_rows(S_, C_, dtype, 31).to(DEV)
        gamma, beta = (1 + 0.1 * seeded_randn((C_,), 8)).to(DEV), (0.1 * seeded_randn((C_,), 9)).to(DEV)
        y1, y2 = sentinel((S_, C_), dtype), sentinel((S_, C_), dtype)
        ws = channelnorm(x, gamma, beta, y1, True, S_, C_, dtype)
        channelnorm(x, gamma, beta, y2, True, S_, C_, dtype, ws=ws)
        assert torch.equal(bits(y1), bits(y2)), (S_, C_)
        assert torch.equal(bits(ops().channel_norm(x, gamma, beta, EPS, gelu=True)), bits(y1))      # and the wrapper's contiguous call


# ------------------------------------------------------------------------------------------------------------------ emo_audio_windows
@pytest.mark.parametrize("D", S.AW_D)
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_audio_windows_index_restatement(dtype, D):
    """out[t, j] = feats[t - m + j] inside the utterance, else 0, bit for bit; T = 200 x D = 768 is past the grid cap: the grid-stride
    loop takes a second trip"""
    assert max(S.AW_T) * 5 * max(S.AW_D) > S.AW_GRID_THREADS
    for T in S.AW_T:
        feats = seeded_randn((T, D), 70 + T).to(dtype)
        dev = feats.to(DEV)
        for m, n in S.AW_MN:
            src = torch.arange(T)[:, None] - m + torch.arange(m + n + 1)[None, :]                 # (T, m + n + 1)
            ok = (src >= 0) & (src < T)
            want = torch.where(ok[:, :, None], feats[src.clamp(0, T - 1)], torch.zeros((), dtype=dtype))
            got = ops().audio_windows(dev, m, n).cpu()
            assert got.shape == (T, m + n + 1, D) and got.dtype == dtype
            assert torch.equal(bits(got), bits(want.contiguous())), (T, D, m, n)


# ------------------------------------------------------------------------------------------------------------------ the encoder
@pytest.fixture(scope="module")
def tiny_encoder():
    from emote_hack_amd.wav2vec2 import Wav2Vec2Model, wav2vec2_synth_state_dict
    sd = wav2vec2_synth_state_dict(cases.WAV2VEC2_TINY)
    m = Wav2Vec2Model(cases.WAV2VEC2_TINY)
    m.load_state_dict(sd)
    return m.to(DEV, torch.float32), sd


@pytest.mark.parametrize("n_samples", S.ENC_SAMPLES)
def test_wav2vec2_tiny_at_real_lengths(tiny_encoder, n_samples):
    """400 samples leave one output frame, 719 still one, 720 two, 4001 an odd remainder at every layer, 48000 are 3 s of audio: the
    window GEMMs at M = 1, the positional conv at T = 1, against the oracle restatement (tests/test_oracle_golden.py pins that to
    transformers) at the tolerance of test_wav2vec2_tiny_f32"""
    from oracle import wav2vec2_ref as W
    model, sd = tiny_encoder
    T = n_samples
    for k, s in zip(model.config.conv_kernel, model.config.conv_stride):
        T = (T - k) // s + 1
    x = 0.5 * seeded_randn((1, n_samples), 600 + n_samples)
    got = model(x).last_hidden_state.cpu()
    want = W.wav2vec2_forward(sd, cases.WAV2VEC2_TINY, x)
    assert got.shape == want.shape == (1, T, 64)
    within(f"wav2vec2 tiny n={n_samples} T={T}", got, want.double(), TOL[torch.float32])


@pytest.mark.parametrize("n_samples", S.ENC_TOO_SHORT)
def test_wav2vec2_refuses_a_length_it_cannot_serve_before_any_launch(tiny_encoder, n_samples, monkeypatch):
    """399 samples run dry at the last layer (one frame in front of a kernel of 2): a ValueError, raised before the first kernel"""
    from emote_hack_amd import ops as o
    model, _sd = tiny_encoder

    def launched(*a, **kw):
        raise AssertionError("a kernel was launched for an utterance the model cannot serve")

    for name in ("gemm", "convert", "channel_norm", "act", "layer_norm"):
        monkeypatch.setattr(o, name, launched)
    with pytest.raises(ValueError):
        model(torch.zeros(1, n_samples))


# ------------------------------------------------------------------------------------------------------------------ emo_image_preprocess
def noise_frame(H, W, seed=0):
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(H * 7 + W + seed), dtype=torch.uint8)


def processor(S_):
    from emote_hack_amd.clip_vision import CLIPImageProcessor
    return CLIPImageProcessor(size={"shortest_edge": S_}, crop_size=S_, device=DEV)


@pytest.mark.parametrize("H,W,S_", S.IP_CASES)
def test_preprocess_geometries_vs_torch_definition(H, W, S_):
    """uniform-noise frames (every tap matters) through CLIPImageProcessor(size={"shortest_edge": S}, crop_size=S) against
    F.interpolate(bicubic, antialias) + crop + clamp + rescale + normalise: 95 taps per axis over a 1500-column span, frames smaller
    than the filter support, crop offsets in the thousands, one partial tile, crops of 32 .. 336"""
    from emote_hack_amd.clip_vision import resize_crop_taps
    t = resize_crop_taps(H, W, S_, S_)
    assert t["span_max"] * 12 <= 64 * 1024
    img = noise_frame(H, W)
    got = processor(S_)(img).pixel_values
    assert got.shape == (1, 3, S_, S_) and got.dtype == torch.float32
    ref = definition_pixels(img, S_, S_)
    print(f"preprocess {H}x{W}->{S_}: taps {t['yw'].shape[1]} x {t['xw'].shape[1]}, span {t['span_max']}, "
          f"max |hip - definition| {float((got[0].cpu() - ref).abs().max()):.3e}")
    within(f"preprocess {H}x{W}->{S_}", got[0].cpu(), ref.double(), dict(rtol=RTOL, atol=ATOL))


def test_preprocess_batch_equals_single_calls():
    H, W, S_ = S.IP_BATCH
    frames = [noise_frame(H, W, seed=i) for i in range(3)]
    assert not torch.equal(frames[0], frames[1]) and not torch.equal(frames[1], frames[2])
    proc = processor(S_)
    batch = proc(torch.stack(frames)).pixel_values
    assert batch.shape == (3, 3, S_, S_)
    for i, f in enumerate(frames):
        assert torch.equal(batch[i], proc(f).pixel_values[0]), i


def test_preprocess_refuses_a_span_beyond_the_lds_before_the_launch():
    """span_max = 5462 columns x 3 channels x 4 bytes is 8 bytes past 64 KB: EMO_ERR_UNSUPPORTED from the entry's checks, the output untouched"""
    S_, k = 8, 4
    img = torch.zeros(1, 1, 6000, 3, dtype=torch.uint8, device=DEV)
    out = sentinel((1, 3, S_, S_), torch.float32)
    tap = torch.zeros(S_, 2, dtype=torch.int32, device=DEV)
    wt = torch.zeros(S_, k, dtype=torch.float32, device=DEV)
    mean, std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.5, 0.5, 0.5)
    call = lambda span: lib().emo_image_preprocess(img.data_ptr(), out.data_ptr(), 1, 1, 6000, S_, tap.data_ptr(), wt.data_ptr(), k, tap.data_ptr(),
                                                   wt.data_ptr(), k, span, 1 / 255, mean, std, stream())
    assert call(5462) == EMO_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert untouched(out, torch.ones(out.shape, dtype=torch.bool, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ emo_vision_embed
def vision_embed(patch, cls, pos, gamma, beta, y, B, Np, C_, dtype):
    return lib().emo_vision_embed(patch.data_ptr(), patch.stride(0), cls.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                  y.stride(0), B, Np, C_, EPS, dti(dtype), stream())


@pytest.mark.parametrize("Np", S.VE_NP)
@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_vision_embed_register_slots_and_leading_dimensions(dtype, Np):
    """C in {V, 1280, 64 * 5 * V} (one vector; slot 4 partly in f32; all five slots full), B = 2, ldp = C + V with NaN padding, ldy =
    C + 2 V with sentinel padding, against LayerNorm([class | patch rows] + position) in f64 at test_vision_embed's tolerance"""
    B, V = S.VE_B, S.vec(dtype)
    for C_ in S.ve_widths(dtype):
        q = lambda t: t.to(dtype)
        patch, cls, pos = q(seeded_randn((B * Np, C_), 41)), q(seeded_randn((C_,), 42)), q(seeded_randn((Np + 1, C_), 43))
        g, b = 1 + 0.1 * seeded_randn((C_,), 44), 0.1 * seeded_randn((C_,), 45)
        tok = torch.cat([cls.double().expand(B, 1, C_), patch.double().view(B, Np, C_)], 1) + pos.double()[None]
        ref = F.layer_norm(tok, (C_,), g.double(), b.double(), EPS32).reshape(-1, C_)
        buf, y, keep = sentinel_cols(B * (Np + 1), C_, C_ + 2 * V, dtype)
        rc = vision_embed(nan_cols(patch, C_ + V), cls.to(DEV), pos.to(DEV), g.to(DEV), b.to(DEV), y, B, Np, C_, dtype)
        assert rc == 0, (C_, rc)
        assert untouched(buf, keep), (C_, "wrote outside the view")
        within(f"vision_embed C={C_} Np={Np} {IDS[dtype]}", y.float().cpu(), ref, TOL_CLIP[dtype])


@pytest.mark.parametrize("dtype", S.DTYPES, ids=IDS.get)
def test_vision_embed_refuses_a_row_beyond_its_registers(dtype):
    B, Np, V = S.VE_B, 1, S.vec(dtype)
    C_ = 64 * S.VE_MAXV * V + V
    patch, cls, pos = (torch.zeros(s, device=DEV, dtype=dtype) for s in ((B * Np, C_), (C_,), (Np + 1, C_)))
    g, b = torch.ones(C_, device=DEV), torch.zeros(C_, device=DEV)
    y = sentinel((B * (Np + 1), C_), dtype)
    assert vision_embed(patch, cls, pos, g, b, y, B, Np, C_, dtype) == EMO_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert untouched(y, torch.ones(y.shape, dtype=torch.bool, device=DEV))
