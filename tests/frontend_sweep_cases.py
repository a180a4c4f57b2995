"""Case tables of the audio / image front-end sweeps, shared by tests/test_gpu_frontend_gemm_sweeps.py and
tests/test_gpu_frontend_sweeps.py (which launch them) and the CPU coverage tests in tests/test_host_logic.py (which ask emo_gemm_plan
what each window GEMM would launch and check the exact probes' arithmetic).  Plain data and CPU tensors, no device needed.

A window GEMM is a 1-D convolution run as emo_gemm on an overlapping row view of its (time, channel) input: row m of A is the k*C
contiguous elements from row m*s of x on, lda = s*C < K = k*C (emote_hack_amd/wav2vec2.py).  V = elements per 16 bytes, BK = k-values
per 128-byte ring stage."""
import torch
import torch.nn.functional as F

from tests.gemm_sweep_cases import ALL_HINTS, DTYPES, bk, ld_of, vec

# ---- A. window GEMMs ---------------------------------------------------------------------------------------------------------------
WIN_KS = ((3, 2), (3, 1), (2, 2), (10, 5))       # (kernel, stride); (2, 2) is the boundary lda == K
WIN_M = (1, 300)                                 # 300: ragged against every tile height
WIN_N = 72
WIN_SPLITS = (1, None, 3)                        # single pass | the planner's (what Wav2Vec2Model.forward runs) | pinned


def win_channels(dtype):
    """K = k*C of one ragged stage | one full stage and a ragged one | several whole stages (the phase main loop takes those)"""
    V, BK = vec(dtype), bk(dtype)
    return (V, BK // 2 + V, 2 * BK)


def win_case(dtype, k, s, C, M, tile=0, split_k=1, bias=False):
    return dict(dtype=dtype, k=k, s=s, C=C, M=M, N=WIN_N, K=k * C, lda=s * C, T=(M - 1) * s + k, tile=tile, split_k=split_k, bias=bias)


def win_cases(dtype, k, s):
    return [win_case(dtype, k, s, C, M, tile, split, bias)
            for C in win_channels(dtype) for M in WIN_M for tile in ALL_HINTS for split in WIN_SPLITS for bias in (False, True)]


def win_geometry(c):
    """the output is N columns from column c0 of a (M + 3, ldc) buffer"""
    c0 = 2 * vec(c["dtype"])
    return dict(c0=c0, ldc=ld_of("q8", c0 + c["N"]))


def win_plan(c):
    from emote_hack_amd import ops
    return ops.gemm_plan(dtype=c["dtype"], M=c["M"], N=c["N"], K=c["K"], lda=c["lda"], ldc=win_geometry(c)["ldc"], bias=c["bias"],
                         tile=c["tile"], split_k=c["split_k"])


def grid16(shape, gen, lim16):
    """multiples of 1/16 in [-lim16 / 16, lim16 / 16]"""
    return torch.randint(-lim16, lim16 + 1, shape, generator=gen).float() / 16.0


def assert_exact(y64, what):
    """every value of the f64 result is a multiple of 1/16 below 16 in magnitude: representable in f32, f16 and bf16 (8 significant
    bits reach 1/16 steps up to 16), so are all partial sums (same bound) - whatever order or split the kernel sums in"""
    assert float(y64.abs().max()) < 16.0 and bool((y64 * 16 == (y64 * 16).round()).all()), what
    for dt_ in DTYPES:
        assert torch.equal(y64.to(dt_).double(), y64), (what, dt_)


def win_operands(dtype, k, s, C, M, mode):
    """CPU operands of one window GEMM and its f64 results: x (T, C), w (N, k*C) - both already quantised to dtype, as f32 -, bias (N,)
    f32, y0 / y0_bias (M, N) f64.
    mode "probe": x[t, c] = 1 where c == t % C else 0, w and bias multiples of 1/16 ([-2, 2], [-1, 1] for k = 10; [-1, 1]), so that
    out[m, n] = bias[n] + sum_j w[n, j*C + (m*s + j) % C] exactly - asserted here.  mode "random": against F.conv1d in f64."""
    N, K, T = WIN_N, k * C, (M - 1) * s + k
    g = torch.Generator(device="cpu").manual_seed(4000 + 131 * k + 17 * s + C + M)
    if mode == "probe":
        x = torch.zeros(T, C)
        x[torch.arange(T), torch.arange(T) % C] = 1.0
        w = grid16((N, K), g, 32 if k <= 3 else 16)
        bias = grid16((N,), g, 16)
        idx = torch.arange(k)[None, :] * C + (torch.arange(M)[:, None] * s + torch.arange(k)[None, :]) % C      # (M, k)
        y0 = w.double()[:, idx].sum(-1).t().contiguous()                                                      # (M, N)
        assert_exact(y0, (k, s, C, M))
        assert_exact(y0 + bias.double(), (k, s, C, M, "bias"))
    else:
        x = torch.randn(T, C, generator=g).to(dtype).float()
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype).float()
        bias = 0.1 * torch.randn(N, generator=g)
        y0 = F.conv1d(x.double().t()[None], w.double().view(N, k, C).permute(0, 2, 1), stride=s)[0].t().contiguous()
    assert y0.shape == (M, N)
    return dict(x=x, w=w, bias=bias, y0=y0, y0_bias=y0 + bias.double())


def win_keys(dtype):
    return [(k, s, C, M) for k, s in WIN_KS for C in win_channels(dtype) for M in WIN_M]


# ---- A'. the grouped form: the positional convolution -------------------------------------------------------------------------------
POS_KP = (16, 15, 128)       # even kernels yield T + 1 steps of which T are kept, odd ones T: the last window ends on xp's last element
POS_G = 3
POS_T = (1, 49, 130)
POS_SPLITS = (None, 1)


def pos_widths(dtype):
    return (vec(dtype), 48)


def pos_case(dtype, kp, cg, T, split_k=None):
    return dict(dtype=dtype, kp=kp, cg=cg, T=T, G=POS_G, M=T, N=cg, K=kp * cg, lda=cg, split_k=split_k, tile=0, bias=True)


def pos_cases(dtype):
    return [pos_case(dtype, kp, cg, T, split) for kp in POS_KP for cg in pos_widths(dtype) for T in POS_T for split in POS_SPLITS]


def pos_plan(c):
    from emote_hack_amd import ops
    return ops.gemm_plan(dtype=c["dtype"], M=c["M"], N=c["N"], K=c["K"], lda=c["lda"], ldc=c["G"] * c["cg"], bias=True, tile=c["tile"],
                         split_k=c["split_k"])


def pos_operands(dtype, kp, cg, T, mode):
    """CPU operands of the grouped positional conv: h (T, G*cg), w (G, cg, kp*cg) with w[g][n][j*cg + c] the tap j / input channel c
    weight of output channel n of group g, bias (G*cg,), y (T, G*cg) f64 = F.conv1d(groups=G, padding=kp // 2)[..., :T].
    mode "probe": a one-hot h (every time step for the short kernels, one step in 16 for kp = 128: at most 16 / 15 / 8 terms of at
    most 1/2 / 1/2 / 1 per sum) and 1/16 grids - every sum exact, asserted here."""
    G, H = POS_G, POS_G * cg
    g = torch.Generator(device="cpu").manual_seed(7000 + 13 * kp + cg + T)
    if mode == "probe":
        every = 16 if kp == 128 else 1
        h = torch.zeros(T, H)
        t = torch.arange(0, T, every)
        for gi in range(G):
            h[t, gi * cg + (t // every + gi) % cg] = 1.0
        w = grid16((G, cg, kp * cg), g, 16 if kp == 128 else 8)
        bias = grid16((H,), g, 16)
    else:
        h = torch.randn(T, H, generator=g).to(dtype).float()
        w = (torch.randn(G, cg, kp * cg, generator=g) / (kp * cg) ** 0.5).to(dtype).float()
        bias = 0.1 * torch.randn(H, generator=g)
    wt = w.view(G * cg, kp, cg).permute(0, 2, 1).double()                         # conv1d's (out, in / groups, k)
    y = F.conv1d(h.double().t()[None], wt, bias.double(), padding=kp // 2, groups=G)[0, :, :T].t().contiguous()
    if mode == "probe":
        assert_exact(y, (kp, cg, T))
    return dict(h=h, w=w, bias=bias, y=y)


def pos_keys(dtype):
    return [(kp, cg, T) for kp in POS_KP for cg in pos_widths(dtype) for T in POS_T]


def win_tables():
    """(section, cases, planner) of every window GEMM the GPU module launches - the coverage test walks this"""
    out = []
    for dt_ in DTYPES:
        for k, s in WIN_KS:
            out.append(("win", win_cases(dt_, k, s), win_plan))
        out.append(("pos", pos_cases(dt_), pos_plan))
    return out


# wav2vec2-base (emote_hack_amd/wav2vec2.py BASE_CONFIG) at 1 s and 10 s of 16 kHz audio: the GEMMs of the feature encoder and of the
# positional convolution as (M, N, K, lda)
def base_model_gemms(n_samples):
    from emote_hack_amd.wav2vec2 import BASE_CONFIG as B
    out, T, C = [], n_samples, 1
    for i, (k, s, co) in enumerate(zip(B["conv_kernel"], B["conv_stride"], B["conv_dim"])):
        T = (T - k) // s + 1
        K = (k + 7) // 8 * 8 if i == 0 else k * C           # layer 0: the window matrix is materialised, its rows padded to 16 bytes
        out.append((T, co, K, K if i == 0 else s * C))
        C = co
    cg = B["hidden_size"] // B["num_conv_pos_embedding_groups"]
    out.append((T, cg, B["num_conv_pos_embeddings"] * cg, cg))
    return out


# ---- B. emo_channelnorm --------------------------------------------------------------------------------------------------------------
CN_S = (1, 2, 3, 4, 5, 255, 256, 257, 513, 16385, 33000)    # 16385: the first S past the 64-chunk cap; 33000: past the 512 apply blocks
CN_C = (1, 63, 64, 65, 130)
CN_PROBE_S = (2, 4, 256, 514, 16386, 33000)                 # even: one chunk, three chunks of 172, the chunk cap, the apply cap
CN_PAD = (3, 5)                                             # ldx = C + 3 (NaN padding), ldy = C + 5 (sentinel padding)


def cn_chunks(S):
    """emo_channelnorm's split: (chunks, rows per chunk, apply blocks)"""
    n = min(64, max(1, -(-S // 256)))
    return n, -(-S // n), min(512, max(1, -(-S // 16)))


# ---- C. emo_audio_windows and the encoder ------------------------------------------------------------------------------------------
AW_T = (1, 2, 4, 200)
AW_MN = ((2, 2), (0, 3), (5, 0), (7, 7))
AW_D = (1, 7, 768)
AW_GRID_THREADS = 256 * 8 * 256                             # frontend.hip fgrid: at most 2048 blocks of 256
ENC_SAMPLES = (400, 719, 720, 4001, 48000)                  # one output frame | still one | two | an odd remainder at every layer | 3 s
ENC_TOO_SHORT = (9, 399)                                    # below the first kernel | no frame left at the last layer

# ---- D. emo_image_preprocess ---------------------------------------------------------------------------------------------------------
IP_CASES = ((1080, 1920, 224), (1500, 1500, 64), (2, 2, 224), (1, 1, 224), (3, 500, 224), (500, 3, 224), (224, 4000, 224),
            (4000, 224, 224), (64, 64, 32), (50, 70, 40), (720, 1280, 336), (37, 53, 336))       # (H, W, S)
IP_BATCH = (50, 70, 40)


# ---- E. emo_vision_embed ---------------------------------------------------------------------------------------------------------------
VE_MAXV = 5                                                 # vision.hip: register slots of 64 lanes x 16 bytes per row
VE_NP = (1, 4)
VE_B = 2


def ve_widths(dtype):
    """one vector | 1280 (f32: slot 4 partly, 2-byte types: slot 2) | all five slots full"""
    V = vec(dtype)
    return (V, 1280, 64 * VE_MAXV * V)
