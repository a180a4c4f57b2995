"""Thin host wrappers: torch tensors (device memory, streams = plumbing) -> raw pointers -> C ABI.

Every function launches hand-written HIP kernels from libemo_hip.so on torch's current stream.
Nothing here computes with torch; tensors are only allocated (`torch.empty`) and addressed.
Activations are 2-D "rows x channels" tensors (NHWC rows), possibly views with a leading
dimension (`.stride(0)`) larger than their width.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import EMO_BF16, EMO_F16, EMO_F32, AttentionParams, GemmParams, check

_DT = {torch.float32: EMO_F32, torch.bfloat16: EMO_BF16, torch.float16: EMO_F16}


def dt(t_or_dtype) -> int:
    d = t_or_dtype if isinstance(t_or_dtype, torch.dtype) else t_or_dtype.dtype
    try:
        return _DT[d]
    except KeyError:
        raise _lib.EmoHipError(f"unsupported compute dtype {d} (float32 | bfloat16 | float16)")


def vec(dtype) -> int:
    return 4 if dtype == torch.float32 else 8


class KernelProfiler:
    """Live per-kernel timing with HIP events on the launch stream (bench.py `roofline`).  Each profiled
    launch is bracketed by two events recorded on the stream the kernel is launched on; durations and
    the launch's ALGORITHMIC flops / bytes are summed per kernel class after a synchronise."""

    def __init__(self):
        self.records = []   # (name, flops, bytes, ev0, ev1)

    def launch(self, name, flops, nbytes, fn, tag=""):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self.records.append((name, flops, nbytes, e0, e1, tag))

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, fl, nb, e0, e1, _tag in self.records:
            d = out.setdefault(name, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += nb
        return out

    def by_shape(self):
        torch.cuda.synchronize()
        out = {}
        for name, fl, nb, e0, e1, tag in self.records:
            d = out.setdefault((name, tag), dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += nb
        return out


PROFILER = None  # set to a KernelProfiler to time launches


def _launch(name, flops, nbytes, fn, tag=""):
    if PROFILER is None:
        fn()
    else:
        PROFILER.launch(name, flops, nbytes, fn, tag)


def _stream():
    if not torch.cuda.is_available():
        raise _lib.EmoHipError("no HIP device: emote_hack_amd ops launch gfx950 kernels (there is no CPU fallback)")
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.EmoHipError("emote_hack_amd ops need device tensors (no CPU fallback on the product path)")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _rows(t):
    """(ptr, ld) of a 2-D row-major view."""
    assert t.dim() == 2 and t.stride(1) == 1, (t.shape, t.stride())
    return _ptr(t), t.stride(0)


# ----------------------------------------------------------------------------- layout / elementwise
def ncfhw_to_rows(x5d: torch.Tensor, dtype, cpad=None) -> torch.Tensor:
    _need_cuda(x5d)
    B, Cc, F, H, W = x5d.shape
    x5d = x5d.contiguous().float()
    cpad = cpad or Cc
    y = torch.empty(B * F * H * W, cpad, device=x5d.device, dtype=dtype)
    check(_lib.load().emo_ncfhw_to_rows(_ptr(x5d), _ptr(y), B, Cc, F, H, W, cpad, cpad, dt(dtype), _stream()), "emo_ncfhw_to_rows")
    return y


def rows_to_ncfhw(x: torch.Tensor, B, Cc, F, H, W) -> torch.Tensor:
    _need_cuda(x)
    p, ld = _rows(x)
    y = torch.empty(B, Cc, F, H, W, device=x.device, dtype=torch.float32)
    check(_lib.load().emo_rows_to_ncfhw(p, _ptr(y), B, Cc, F, H, W, ld, dt(x), _stream()), "emo_rows_to_ncfhw")
    return y


def copy_cols(x: torch.Tensor, y: torch.Tensor, coff: int):
    px, ldx = _rows(x)
    py, ldy = _rows(y)
    check(_lib.load().emo_copy_cols(px, ldx, py, ldy, coff, x.shape[0], x.shape[1], dt(x), _stream()), "emo_copy_cols")


def concat_cols(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], dim=channels) (unet_3d_blocks.py:629,731) as two strided row copies."""
    y = torch.empty(a.shape[0], a.shape[1] + b.shape[1], device=a.device, dtype=a.dtype)
    copy_cols(a, y, 0)
    copy_cols(b, y, a.shape[1])
    return y


def add(a: torch.Tensor, b: torch.Tensor, alpha=1.0, out=None) -> torch.Tensor:
    out = torch.empty_like(a) if out is None else out
    pa, lda = _rows(a)
    pb, ldb = _rows(b)
    po, ldo = _rows(out)
    check(_lib.load().emo_add(pa, lda, pb, ldb, float(alpha), po, ldo, a.shape[0], a.shape[1], dt(a), _stream()), "emo_add")
    return out


def add_periodic(x: torch.Tensor, f: torch.Tensor, out=None) -> torch.Tensor:
    """y[m, :] = x[m, :] + f[m % P, :] over rows views (emo_add_periodic): the face-region map added behind conv_in to every frame of
    every batch row (Net.py:509-516).  out=None runs IN PLACE on x - the zero-copy skip slot keeps its address."""
    _need_cuda(x, f, out)
    out = x if out is None else out
    assert f.dtype == x.dtype == out.dtype and f.shape[1] == x.shape[1] and tuple(out.shape) == tuple(x.shape), (x.shape, f.shape, out.shape)
    px, ldx = _rows(x)
    pf, ldf = _rows(f)
    po, ldo = _rows(out)
    _launch("add_periodic", 0.0, x.element_size() * (2.0 * x.shape[0] + f.shape[0]) * x.shape[1],
            lambda: check(_lib.load().emo_add_periodic(px, ldx, pf, ldf, po, ldo, x.shape[0], x.shape[1], f.shape[0], dt(x), _stream()),
                          "emo_add_periodic"), tag=f"M={x.shape[0]} C={x.shape[1]} P={f.shape[0]}")
    return out


def mask_pool(mask: torch.Tensor, dtype, threshold=None) -> torch.Tensor:
    """f32 (Hp, Wp) map -> (Hp/8 * Wp/8, 8) rows in `dtype`: channel 0 the 8x8 area mean, channels 1..7 zero - the cpad=8 rows
    FaceRegionController consumes (emo_mask_pool).  threshold=t pools (x > t ? 1 : 0) instead: FaceLocator logits take t = 0."""
    _need_cuda(mask)
    assert mask.dtype == torch.float32 and mask.dim() == 2 and mask.is_contiguous(), (mask.dtype, mask.shape)
    Hp, Wp = mask.shape
    out = torch.empty(max(Hp // 8, 0) * max(Wp // 8, 0), 8, device=mask.device, dtype=dtype)
    check(_lib.load().emo_mask_pool(_ptr(mask), _ptr(out), Hp, Wp, int(threshold is not None), float(threshold or 0.0), dt(dtype), _stream()),
          "emo_mask_pool")
    return out


def convert(src: torch.Tensor, dtype, fp16_round=False) -> torch.Tensor:
    _need_cuda(src)
    src = src.contiguous()
    dst = torch.empty(src.shape, device=src.device, dtype=dtype)
    check(_lib.load().emo_convert(_ptr(src), dt(src), _ptr(dst), dt(dtype), src.numel(), int(fp16_round), _stream()), "emo_convert")
    return dst


def silu(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.load().emo_silu(_ptr(x), _ptr(y), x.numel(), dt(x), _stream()), "emo_silu")
    return y


def timestep_embedding(timesteps: torch.Tensor, freqs: torch.Tensor, dim: int, flip: bool, dtype) -> torch.Tensor:
    """int64 timesteps -> emo_timestep_embedding; float32 ones (fractional tables) -> emo_timestep_embedding_f32"""
    _need_cuda(timesteps, freqs)
    assert timesteps.dtype in (torch.int64, torch.float32) and freqs.dtype == torch.float32
    B = timesteps.shape[0]
    out = torch.empty(B, dim, device=timesteps.device, dtype=dtype)
    name = "emo_timestep_embedding" if timesteps.dtype == torch.int64 else "emo_timestep_embedding_f32"
    check(getattr(_lib.load(), name)(_ptr(timesteps), _ptr(freqs), _ptr(out), B, dim, int(flip), dt(dtype), _stream()), name)
    return out


# ----------------------------------------------------------------------------- norms
GN_ONE_LAUNCH = True   # A/B hook (bench.py --gn-two-launch): False keeps every GroupNorm on the stats + apply pair


def _mod_rows(mod, n_inst, Cc):
    """(ptr, ld) of a scale-shift modulation operand: f32 (n_inst, 2C) = (scale | shift), possibly a column view of a wider buffer"""
    assert mod.dtype == torch.float32 and tuple(mod.shape) == (n_inst, 2 * Cc) and mod.stride(1) == 1, (mod.shape, mod.dtype, mod.stride())
    return _ptr(mod), mod.stride(0)


def _mod_per_rows(mod, M, S, mod_rows, Cc):
    """(ptr, ld) of a PER-FRAME modulation operand: f32 (M / mod_rows, 2C), one (scale | shift) row per mod_rows consecutive rows of x;
    an instance of S rows holds whole frames"""
    assert mod_rows > 0 and S % mod_rows == 0, (S, mod_rows)
    return _mod_rows(mod, M // mod_rows, Cc)


def group_norm(x: torch.Tensor, gamma, beta, n_inst: int, groups: int, eps: float, silu_: bool, out=None, mod=None, mod_rows=0) -> torch.Tensor:
    """GroupNorm over NHWC rows; x (n_inst*S, C).  n_inst=B -> joint 5-D statistics (resnet.py:180),
    n_inst=B*F -> per frame (attention.py:124).
    mod = f32 (n_inst, 2C) rows (scale | shift): the scale-shift form y = act(GN(x) * (1 + scale) + shift) (resnet.py:191-197) in the
    same launches - emo_hip.h emo_groupnorm_apply_mod / emo_groupnorm_mod.
    mod_rows = r > 0: mod is (M / r, 2C) instead - one row per r consecutive rows of x (per FRAME under joint statistics: the per-frame
    speed embedding, resnet.py:188-195) - emo_groupnorm_apply_mod_rows / emo_groupnorm_mod_rows."""
    _need_cuda(x, mod)
    lib = _lib.load()
    M, Cc = x.shape
    S = M // n_inst
    px, ldx = _rows(x)
    y = torch.empty(M, Cc, device=x.device, dtype=x.dtype) if out is None else out
    py, ldy = _rows(y)
    if mod is not None and mod_rows:
        pm, ldm = _mod_per_rows(mod, M, S, mod_rows, Cc)
        tag = f"M={M} C={Cc}{' silu' if silu_ else ''} mod/{mod_rows}"
        if GN_ONE_LAUNCH and lib.emo_groupnorm_one_launch_ok(n_inst, S, Cc, groups, dt(x)):
            _launch("groupnorm", 0.0, x.element_size() * 2.0 * M * Cc,
                    lambda: check(lib.emo_groupnorm_mod_rows(px, ldx, _ptr(gamma), _ptr(beta), pm, ldm, int(mod_rows), py, ldy, n_inst, S, Cc, groups,
                                                             float(eps), int(silu_), dt(x), _stream()), "emo_groupnorm_mod_rows"), tag=tag + " 1L")
            return y
        part = torch.empty(max(lib.emo_groupnorm_workspace_bytes(n_inst, S, Cc, groups) // 4, 1), device=x.device, dtype=torch.float32)

        def run_mod_rows():
            check(lib.emo_groupnorm_stats(px, ldx, _ptr(part), n_inst, S, Cc, groups, dt(x), _stream()), "emo_groupnorm_stats")
            check(lib.emo_groupnorm_apply_mod_rows(px, ldx, _ptr(part), _ptr(gamma), _ptr(beta), pm, ldm, int(mod_rows), py, ldy, n_inst, S, Cc,
                                                   groups, float(eps), int(silu_), dt(x), _stream()), "emo_groupnorm_apply_mod_rows")
        _launch("groupnorm", 0.0, x.element_size() * 2.0 * M * Cc, run_mod_rows, tag=tag)
        return y
    if mod is not None:
        pm, ldm = _mod_rows(mod, n_inst, Cc)
        tag = f"M={M} C={Cc}{' silu' if silu_ else ''} mod"
        if GN_ONE_LAUNCH and lib.emo_groupnorm_one_launch_ok(n_inst, S, Cc, groups, dt(x)):
            _launch("groupnorm", 0.0, x.element_size() * 2.0 * M * Cc,
                    lambda: check(lib.emo_groupnorm_mod(px, ldx, _ptr(gamma), _ptr(beta), pm, ldm, py, ldy, n_inst, S, Cc, groups, float(eps),
                                                        int(silu_), dt(x), _stream()), "emo_groupnorm_mod"), tag=tag + " 1L")
            return y
        part = torch.empty(max(lib.emo_groupnorm_workspace_bytes(n_inst, S, Cc, groups) // 4, 1), device=x.device, dtype=torch.float32)

        def run_mod():
            check(lib.emo_groupnorm_stats(px, ldx, _ptr(part), n_inst, S, Cc, groups, dt(x), _stream()), "emo_groupnorm_stats")
            check(lib.emo_groupnorm_apply_mod(px, ldx, _ptr(part), _ptr(gamma), _ptr(beta), pm, ldm, py, ldy, n_inst, S, Cc, groups,
                                              float(eps), int(silu_), dt(x), _stream()), "emo_groupnorm_apply_mod")
        _launch("groupnorm", 0.0, x.element_size() * 2.0 * M * Cc, run_mod, tag=tag)
        return y
    if GN_ONE_LAUNCH and lib.emo_groupnorm_one_launch_ok(n_inst, S, Cc, groups, dt(x)):   # small instances: one launch, one read
        _launch("groupnorm", 0.0, x.element_size() * 2.0 * M * Cc,
                lambda: check(lib.emo_groupnorm(px, ldx, _ptr(gamma), _ptr(beta), py, ldy, n_inst, S, Cc, groups, float(eps), int(silu_),
                                                dt(x), _stream()), "emo_groupnorm"), tag=f"M={M} C={Cc}{' silu' if silu_ else ''} 1L")
        return y
    ws = lib.emo_groupnorm_workspace_bytes(n_inst, S, Cc, groups)
    part = torch.empty(max(ws // 4, 1), device=x.device, dtype=torch.float32)

    def run():
        check(lib.emo_groupnorm_stats(px, ldx, _ptr(part), n_inst, S, Cc, groups, dt(x), _stream()), "emo_groupnorm_stats")
        check(lib.emo_groupnorm_apply(px, ldx, _ptr(part), _ptr(gamma), _ptr(beta), py, ldy, n_inst, S, Cc, groups, float(eps),
                                      int(silu_), dt(x), _stream()), "emo_groupnorm_apply")
    _launch("groupnorm", 0.0, x.element_size() * 2.0 * M * Cc, run, tag=f"M={M} C={Cc}{' silu' if silu_ else ''}")   # algorithmic: one read + one write
    return y


def group_norm_coeffs(x: torch.Tensor, gamma, beta, n_inst: int, groups: int, eps: float, mod=None, mod_rows=0) -> torch.Tensor:
    """The statistics half of a GroupNorm whose normalisation runs inside its consumer (conv3x3(gn=...)): one read-only pass over x,
    then the per-(instance, channel) factors (n_inst, 2C) f32, channel pairs interleaved (scale, scale, shift, shift) - emo_hip.h
    emo_groupnorm_coeffs.  The normalised tensor is never materialised.
    mod = f32 (n_inst, 2C) rows (scale | shift): the factors carry the scale-shift modulation (emo_groupnorm_coeffs_mod).
    mod_rows = r > 0: mod is (M / r, 2C), one row per r consecutive rows of x, and the table has one row per mod row, (M / r, 2C):
    the consumer reads it with ONE image per table row (emo_groupnorm_coeffs_mod_rows)."""
    _need_cuda(x, mod)
    lib = _lib.load()
    M, Cc = x.shape
    S = M // n_inst
    px, ldx = _rows(x)
    part = torch.empty(max(lib.emo_groupnorm_workspace_bytes(n_inst, S, Cc, groups) // 4, 1), device=x.device, dtype=torch.float32)
    per_rows = mod is not None and mod_rows
    coef = torch.empty(M // mod_rows if per_rows else n_inst, 2 * Cc, device=x.device, dtype=torch.float32)

    def run():
        check(lib.emo_groupnorm_stats(px, ldx, _ptr(part), n_inst, S, Cc, groups, dt(x), _stream()), "emo_groupnorm_stats")
        if per_rows:
            pm, ldm = _mod_per_rows(mod, M, S, mod_rows, Cc)
            check(lib.emo_groupnorm_coeffs_mod_rows(_ptr(part), _ptr(gamma), _ptr(beta), pm, ldm, int(mod_rows), _ptr(coef), n_inst, S, Cc, groups,
                                                    float(eps), dt(x), _stream()), "emo_groupnorm_coeffs_mod_rows")
            return
        if mod is not None:
            pm, ldm = _mod_rows(mod, n_inst, Cc)
            check(lib.emo_groupnorm_coeffs_mod(_ptr(part), _ptr(gamma), _ptr(beta), pm, ldm, _ptr(coef), n_inst, S, Cc, groups, float(eps), dt(x),
                                               _stream()), "emo_groupnorm_coeffs_mod")
            return
        check(lib.emo_groupnorm_coeffs(_ptr(part), _ptr(gamma), _ptr(beta), _ptr(coef), n_inst, S, Cc, groups, float(eps), dt(x), _stream()),
              "emo_groupnorm_coeffs")
    _launch("groupnorm_stats", 0.0, x.element_size() * 1.0 * M * Cc, run, tag=f"M={M} C={Cc}")   # algorithmic: one read
    return coef


def group_norm_fold_linear(x: torch.Tensor, gamma, beta, n_inst: int, groups: int, eps: float, w: torch.Tensor, bias):
    """GroupNorm (no activation) folded into the Linear / 1x1 conv behind it (emo_hip.h emo_groupnorm_fold_linear): one
    statistics pass over x, then per-instance weights (n_inst, Cout, C) and a per-instance bias (n_inst, Cout) f32 for
    gemm(x, w_n, bias_n, w_slab_rows=S) - the normalised tensor is never materialised."""
    _need_cuda(x, w)
    lib = _lib.load()
    M, Cc = x.shape
    S = M // n_inst
    Cout = w.shape[0]
    assert w.shape == (Cout, Cc) and w.is_contiguous() and w.dtype == x.dtype
    px, ldx = _rows(x)
    part = torch.empty(max(lib.emo_groupnorm_workspace_bytes(n_inst, S, Cc, groups) // 4, 1), device=x.device, dtype=torch.float32)
    wn = torch.empty(n_inst, Cout, Cc, device=x.device, dtype=x.dtype)
    rb = torch.empty(n_inst, Cout, device=x.device, dtype=torch.float32)

    def run():
        check(lib.emo_groupnorm_stats(px, ldx, _ptr(part), n_inst, S, Cc, groups, dt(x), _stream()), "emo_groupnorm_stats")
        check(lib.emo_groupnorm_fold_linear(_ptr(part), _ptr(gamma), _ptr(beta), _ptr(w), _ptr(bias), _ptr(wn), _ptr(rb), n_inst, S, Cc, groups,
                                            Cout, float(eps), dt(x), _stream()), "emo_groupnorm_fold_linear")
    _launch("groupnorm_fold", 0.0, x.element_size() * 1.0 * M * Cc, run, tag=f"M={M} C={Cc}")   # algorithmic: one read
    return wn, rb


def layer_norm(x: torch.Tensor, gamma, beta, eps=1e-5, pe=None, rows_per_frame=0, frames=0) -> torch.Tensor:
    _need_cuda(x)
    M, Cc = x.shape
    px, ldx = _rows(x)
    y = torch.empty(M, Cc, device=x.device, dtype=x.dtype)
    _launch("layernorm", 0.0, x.element_size() * 2.0 * M * Cc,
            lambda: check(_lib.load().emo_layernorm(px, ldx, _ptr(gamma), _ptr(beta), _ptr(y), Cc, M, Cc, float(eps), _ptr(pe),
                                                    rows_per_frame, frames, dt(x), _stream()), "emo_layernorm"))
    return y


def layer_norm_act(x: torch.Tensor, gamma, beta, eps=1e-5, gelu=True, out=None) -> torch.Tensor:
    """act(LayerNorm(x)) over the last dim in one pass, act = erf-GELU or none (emo_layernorm_act).  out: a rows view to write into."""
    _need_cuda(x, out)
    M, Cc = x.shape
    px, ldx = _rows(x)
    y = torch.empty(M, Cc, device=x.device, dtype=x.dtype) if out is None else out
    assert y.shape == x.shape and y.dtype == x.dtype, (y.shape, y.dtype)
    py, ldy = _rows(y)
    _launch("layernorm_act", 0.0, x.element_size() * 2.0 * M * Cc,
            lambda: check(_lib.load().emo_layernorm_act(px, ldx, _ptr(gamma), _ptr(beta), py, ldy, M, Cc, float(eps), int(bool(gelu)), dt(x),
                                                        _stream()), "emo_layernorm_act"))
    return y


def layer_norm_stats(x: torch.Tensor, eps=1e-5) -> torch.Tensor:
    """(mean, rstd) per row, f32 (M, 2): the statistics pass of a LayerNorm folded into the consumer GEMM (gemm(ln=...))."""
    _need_cuda(x)
    M, Cc = x.shape
    px, ldx = _rows(x)
    st = torch.empty(M, 2, device=x.device, dtype=torch.float32)
    _launch("layernorm_stats", 0.0, x.element_size() * 1.0 * M * Cc,
            lambda: check(_lib.load().emo_layernorm_stats(px, ldx, _ptr(st), M, Cc, float(eps), dt(x), _stream()), "emo_layernorm_stats"))
    return st


# ----------------------------------------------------------------------------- GEMM / conv
_VT_VERDICT = {}   # (M, w shape, vt geometry, dtype, tile hint) -> emo_gemm_vt_ok's answer: unsupported levels go straight to two launches
GEMM_TILE = 0   # tuning hook for tools/bench: pins emo_gemm_params.tile of every dense GEMM that does not pass tile=


def gemm(a: torch.Tensor, w: torch.Tensor, bias=None, *, rowbias=None, rows_per_batch=0, residual=None, geglu=False,
         out_scale=1.0, out=None, transpose_rows=0, transpose_ld=0, conv=None, split_k=None, ln=None, tile=None,
         w_slab_rows=0, gn=None, vt_cols=0, vt_rows=0, vt_ld=0, workspace=None, vt_out=None):
    """out = epilogue(a @ w.T).  a (M, K) rows view; w (N, K) contiguous in the compute dtype.
    ln = (colsum f32 (N,), stats f32 (M, 2) from layer_norm_stats(a)): LayerNorm over K folded into the GEMM - a holds the RAW
    rows, w / bias carry the folded affine (emo_hip.h emo_gemm_params.ln_colsum).
    conv = dict(H, W, Cin, stride, upsample2x, Ho, Wo) selects the implicit 3x3 conv loader (then a is
    the (B*F*H*W, >=Cin) NHWC input and M = B*F*Ho*Wo).
    transpose_rows=L stores V^T per batch of L rows: out (M/L, N, transpose_ld).
    gn = (coef from group_norm_coeffs(a), images per instance, silu): GroupNorm (+ SiLU) of the conv's input applied inside the
    halo-reuse 3x3 conv - a holds the RAW rows (emo_hip.h emo_gemm_params.gn_coef; conv_gn_fusable says which convs qualify).
    vt_cols = n: the LAST n output columns are stored transposed per batch of vt_rows rows (V^T (M / vt_rows, n, vt_ld)), the first N - n
    row-major: returns (out (M, N - n), vt) - or None when this GEMM is not served that way (emo_hip.h emo_gemm_params.vt; the caller
    then runs two launches).
    vt_out = the (M / vt_rows, vt_cols, vt_ld) tensor to store V^T into instead of a fresh allocation.
    workspace = an f32 tensor to hold the split-K partials (at least split_k * M * N elements) instead of a fresh allocation."""
    _need_cuda(a, w)
    if vt_cols and _VT_VERDICT.get((a.shape[0], tuple(w.shape), vt_cols, vt_rows, vt_ld, a.dtype, tile, GEMM_TILE)) is False:
        return None     # asked before (emo_gemm_vt_ok below): not served - no throw-away allocations, no ctypes call
    p = GemmParams()
    pa, lda = _rows(a)
    if w_slab_rows:     # per-instance weights (n_inst, N, K) and bias (n_inst, N): rows [i * w_slab_rows, ...) use slab i (group_norm_fold_linear)
        assert w.dim() == 3 and conv is None and ln is None and a.shape[0] == w.shape[0] * w_slab_rows, (w.shape, a.shape, w_slab_rows)
        assert bias is None or (bias.shape == w.shape[:2] and bias.is_contiguous()), bias.shape
        p.w_slab_rows, p.w_slab_stride = w_slab_rows, w.stride(0)
        split_k = 1
    N, K = w.shape[-2:]
    assert w.is_contiguous() and w.dtype == a.dtype, (w.dtype, a.dtype)
    if conv is None:
        M = a.shape[0]
        assert a.shape[1] == K, (a.shape, w.shape)
    else:
        M = (a.shape[0] // (conv["H"] * conv["W"])) * conv["Ho"] * conv["Wo"]
    n_out = N // 2 if geglu else N
    if transpose_rows:
        nb = M // transpose_rows
        if out is None:
            out = torch.empty(nb, n_out, transpose_ld, device=a.device, dtype=a.dtype)   # pad columns [L, ld) are cleaned by the attention loader
        p.transpose_out, p.t_rows, p.t_ld, p.t_batch_stride = 1, transpose_rows, transpose_ld, n_out * transpose_ld
        p.C, p.ldc = out.data_ptr(), 0
    else:
        if out is None:
            out = torch.empty(M, n_out - vt_cols, device=a.device, dtype=a.dtype)
        pc, ldc = _rows(out)
        p.C, p.ldc = pc.value, ldc
    p.A, p.lda, p.W = pa.value, lda, w.data_ptr()
    p.bias = bias.data_ptr() if bias is not None else None
    if rowbias is not None:
        assert rowbias.dtype == torch.float32 and rowbias.stride(1) == 1
        p.rowbias, p.rows_per_batch, p.ld_rowbias = rowbias.data_ptr(), rows_per_batch, rowbias.stride(0)
    if residual is not None:
        pr, ldr = _rows(residual)
        p.residual, p.ldr = pr.value, ldr
    p.M, p.N, p.K = M, N, K
    p.geglu, p.out_scale = int(geglu), float(out_scale)
    if conv is not None:
        p.conv_taps, p.H, p.W_, p.Cin = 9, conv["H"], conv["W"], conv["Cin"]
        p.stride, p.upsample2x, p.Ho, p.Wo = conv["stride"], int(conv["upsample2x"]), conv["Ho"], conv["Wo"]
        p.conv_asym = int(conv.get("asym", 0))
        p.up_h, p.up_w = conv.get("up", (0, 0))
    p.dtype = dt(a)
    vt = None
    if vt_cols:
        assert conv is None and not geglu and residual is None and not transpose_rows and tuple(out.shape) == (M, N - vt_cols)
        vt = vt_out if vt_out is not None else torch.empty(M // vt_rows, vt_cols, vt_ld, device=a.device, dtype=a.dtype)
        assert tuple(vt.shape) == (M // vt_rows, vt_cols, vt_ld) and vt.is_contiguous() and vt.dtype == a.dtype
        p.vt, p.vt_col0, p.t_rows, p.t_ld, p.t_batch_stride = vt.data_ptr(), N - vt_cols, vt_rows, vt_ld, vt_cols * vt_ld
    if gn is not None:
        coef, imgs_per_inst, gn_silu = gn
        assert conv is not None and coef.dtype == torch.float32 and coef.is_contiguous() and coef.shape[1] == 2 * conv["Cin"], coef.shape
        p.gn_coef, p.gn_imgs_per_inst, p.gn_silu = coef.data_ptr(), int(imgs_per_inst), int(bool(gn_silu))
        split_k = 1
    p.tile = int(tile if tile is not None else (GEMM_TILE if conv is None else 0))
    if ln is not None:
        colsum, stats = ln
        assert conv is None and colsum.dtype == torch.float32 and colsum.numel() == N
        assert stats.dtype == torch.float32 and stats.shape == (M, 2) and stats.is_contiguous()
        p.ln_colsum, p.ln_stats = colsum.data_ptr(), stats.data_ptr()
        split_k = 1   # the correction rides in the accumulator init of ONE pass over K
    lib = _lib.load()
    if vt_cols:
        split_k = 1
        ok = bool(lib.emo_gemm_vt_ok(C.byref(p)))
        if out.data_ptr() % 16 == 0 and vt.data_ptr() % 16 == 0 and out.stride(0) == N - vt_cols:   # (the verdict of a plain geometry only)
            _VT_VERDICT[(a.shape[0], tuple(w.shape), vt_cols, vt_rows, vt_ld, a.dtype, tile, GEMM_TILE)] = ok
        if not ok:
            return None
    sk = lib.emo_gemm_suggest_split_k(M, N, K, p.dtype, int(bool(geglu)), int(bool(transpose_rows))) if split_k is None else split_k
    ws = None
    if sk > 1:
        if workspace is not None:
            assert workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() * 4 >= lib.emo_gemm_workspace_bytes(M, N, sk)
        ws = workspace if workspace is not None else torch.empty(lib.emo_gemm_workspace_bytes(M, N, sk) // 4, device=a.device, dtype=torch.float32)
        p.split_k, p.workspace = sk, ws.data_ptr()
    esz = a.element_size()
    _launch("gemm_conv3x3" if conv is not None else "gemm_dense", 2.0 * M * N * K,
            esz * (float(M) * (K if conv is None else conv["Cin"]) + float(N) * K + float(M) * n_out),
            lambda: check(_lib.load().emo_gemm(C.byref(p), _stream()), "emo_gemm"),
            tag=f"M={M} N={N} K={K}" + (" geglu" if geglu else "") + (" T" if transpose_rows else "") +
                (f" s{conv['stride']}{'u' if conv['upsample2x'] else ''}" if conv is not None else "") + (f" sk{sk}" if sk > 1 else "") +
                (" ln" if ln is not None else "") + (" slab" if w_slab_rows else "") + (" rowbias" if rowbias is not None else "") +
                (" gn" if gn is not None else "") + (f" vt{vt_cols}" if vt_cols else ""))
    return (out, vt) if vt_cols else out


GEMM_STORE_PATHS = ("lds", "vec_row", "scalar_row", "vt_quad", "vt_scalar", "splitk_ws")   # emo_hip.h emo_gemm_plan, plan[5]


def gemm_plan(*, dtype, M, N, K, lda=None, ldc=None, bias=False, rowbias=False, rows_per_batch=0, ld_rowbias=None, residual=False, ldr=None,
              geglu=False, out_scale=1.0, transpose_rows=0, transpose_ld=0, t_batch_stride=None, conv=None, split_k=None, workspace=True,
              ln=False, ln_colsum=None, ln_stats=None, tile=0, w_slab_rows=0, w_slab_stride=None, vt_cols=0, vt_rows=0, vt_ld=0,
              misalign=None):
    """What ops.gemm / emo_gemm launches for this parameter block, asked of the library on the host (emo_hip.h emo_gemm_plan; no GPU
    needed): (family, tile after fallbacks, phase loop, flags [1 conv | 2 V^T kernel | 4 LayerNorm fold | 8 vt split store], split_k,
    store path - an index into GEMM_STORE_PATHS -, bias in the accumulators, row bias in the accumulators).
    Operands are described, not passed: bias / rowbias / residual / ln say whether the pointer is set; lda / ldc / ldr / ld_rowbias
    default to the contiguous widths; split_k=None asks the planner as ops.gemm does, workspace=False withholds the split-K workspace;
    ln_colsum / ln_stats override ln for one pointer each; misalign = dict(A= / W= / C= / residual= / bias= / ln_colsum= / ln_stats= /
    vt= bytes) offsets that pointer from 256-byte alignment.  Raises EmoHipError where emo_gemm would refuse the call."""
    mis = dict(misalign or {})
    fake = lambda name, on=True: (256 + mis.get(name, 0)) if on else None    # non-NULL, never dereferenced
    p = GemmParams()
    n_out = N // 2 if geglu else N
    p.A, p.lda, p.W = fake("A"), (K if conv is None else conv["Cin"]) if lda is None else lda, fake("W")
    p.bias = fake("bias", bias)
    if rowbias:
        p.rowbias, p.rows_per_batch, p.ld_rowbias = fake("rowbias"), rows_per_batch, N if ld_rowbias is None else ld_rowbias
    if residual:
        p.residual, p.ldr = fake("residual"), n_out if ldr is None else ldr
    p.C = fake("C")
    if transpose_rows:
        p.transpose_out, p.t_rows, p.t_ld = 1, transpose_rows, transpose_ld
        p.t_batch_stride = n_out * transpose_ld if t_batch_stride is None else t_batch_stride
    else:
        p.ldc = (n_out - vt_cols) if ldc is None else ldc
    p.M, p.N, p.K = M, N, K
    p.geglu, p.out_scale = int(geglu), float(out_scale)
    if conv is not None:
        p.conv_taps, p.H, p.W_, p.Cin = 9, conv["H"], conv["W"], conv["Cin"]
        p.stride, p.upsample2x, p.Ho, p.Wo = conv["stride"], int(conv.get("upsample2x", 0)), conv["Ho"], conv["Wo"]
        p.conv_asym = int(conv.get("asym", 0))
        p.up_h, p.up_w = conv.get("up", (0, 0))
    p.dtype = dt(dtype)
    if vt_cols:
        p.vt, p.vt_col0, p.t_rows, p.t_ld, p.t_batch_stride = fake("vt"), N - vt_cols, vt_rows, vt_ld, vt_cols * vt_ld
    if w_slab_rows:
        p.w_slab_rows, p.w_slab_stride = w_slab_rows, N * K if w_slab_stride is None else w_slab_stride
    p.tile = int(tile)
    p.ln_colsum = fake("ln_colsum", ln if ln_colsum is None else ln_colsum)
    p.ln_stats = fake("ln_stats", ln if ln_stats is None else ln_stats)
    lib = _lib.load()
    if split_k is None:     # what ops.gemm does
        split_k = 1 if (ln or vt_cols or w_slab_rows) else lib.emo_gemm_suggest_split_k(M, N, K, p.dtype, int(bool(geglu)), int(bool(transpose_rows)))
    if split_k > 1:
        p.split_k, p.workspace = split_k, fake("workspace", workspace)
    plan = (C.c_int * 8)()
    check(lib.emo_gemm_plan(C.byref(p), plan), "emo_gemm_plan")
    return tuple(plan)


def conv_halo_plan(*, dtype, n_img, H, W, Cin, N, upsample2x=False, lda=None, ldc=None, bias=False, rowbias=False, rows_per_batch=0,
                   ld_rowbias=None, residual=False, ldr=None, inplace=False, out_scale=1.0, gn=False, imgs_per_inst=1, silu=True, tile=0):
    """What the stride-1 3x3 conv of n_img frames of H x W (x Cin) to N channels launches on the halo-reuse kernel, asked of the library
    on the host (emo_hip.h emo_conv3x3_halo_plan; no GPU needed): (served, patch height, block width / tiles / grid of the main launch,
    block width / tiles / grid of the tail launch; 0s for a launch that does not exist or a conv the kernel does not serve).
    Operands are described, not passed, as in gemm_plan; the output and the residual get DISJOINT fake address ranges unless
    inplace=True says the residual is the output (then ldr = ldc).  Raises EmoHipError where emo_gemm would refuse the call."""
    He, We = (2 * H, 2 * W) if upsample2x else (H, W)
    p = GemmParams()
    p.A, p.lda, p.W = 256, Cin if lda is None else lda, 256
    p.bias = 256 if bias else None
    if rowbias:
        p.rowbias, p.rows_per_batch, p.ld_rowbias = 256, rows_per_batch, N if ld_rowbias is None else ld_rowbias
    p.C, p.ldc = 1 << 40, N if ldc is None else ldc
    if residual or inplace:
        p.residual, p.ldr = (p.C, p.ldc) if inplace else (1 << 41, N if ldr is None else ldr)
    p.M, p.N, p.K, p.out_scale = n_img * He * We, N, 9 * Cin, float(out_scale)
    p.conv_taps, p.H, p.W_, p.Cin, p.stride, p.upsample2x, p.Ho, p.Wo = 9, H, W, Cin, 1, int(upsample2x), He, We
    p.dtype, p.tile, p.split_k = dt(dtype), int(tile), 1
    if gn:
        p.gn_coef, p.gn_imgs_per_inst, p.gn_silu = 256, int(imgs_per_inst), int(bool(silu))
    plan = (C.c_int * 8)()
    check(_lib.load().emo_conv3x3_halo_plan(C.byref(p), plan), "emo_conv3x3_halo_plan")
    return tuple(plan)


def conv_gn_fusable(x: torch.Tensor, w: torch.Tensor, n_img: int, H: int, W: int, rowbias=None, rows_per_batch=0) -> bool:
    """Whether the stride-1 3x3 conv of x (n_img*H*W, >= Cin) with the re-laid weight w runs on the halo-reuse kernel, i.e. may take
    its GroupNorm (+ SiLU) along as conv3x3(gn=...) (emo_hip.h emo_conv3x3_gn_fusable)."""
    p = GemmParams()
    _, lda = _rows(x)
    p.lda, p.M, p.N, p.K = lda, n_img * H * W, w.shape[0], w.shape[1]
    p.conv_taps, p.H, p.W_, p.Cin, p.stride, p.Ho, p.Wo = 9, H, W, w.shape[1] // 9, 1, H, W
    p.dtype = dt(x)
    if rowbias is not None:
        p.rowbias, p.rows_per_batch, p.ld_rowbias = rowbias.data_ptr(), rows_per_batch, rowbias.stride(0)
    return bool(_lib.load().emo_conv3x3_gn_fusable(C.byref(p)))


def conv3x3(x: torch.Tensor, w: torch.Tensor, bias, n_img: int, H: int, W: int, *, stride=1, upsample2x=False, pad=1, upsample_to=None, **kw):
    """Per-frame 3x3 conv, pad 1 (resnet.py:30-38), as an implicit GEMM over NHWC rows.
    w is the re-laid (Cout, 9*Cin_pad) weight.  pad=0 means the asymmetric (0, 1, 0, 1) padding of the VAE encoder's downsampler."""
    cin = w.shape[1] // 9
    if upsample_to is not None and tuple(upsample_to) == (2 * H, 2 * W):
        upsample2x, upsample_to = True, None        # the x2 fast path (a shift instead of a division per tap)
    He, We = (2 * H, 2 * W) if upsample2x else (tuple(upsample_to) if upsample_to is not None else (H, W))
    tot = 2 if pad == 1 else 1
    Ho, Wo = (He + tot - 3) // stride + 1, (We + tot - 3) // stride + 1
    assert x.shape[0] == n_img * H * W and pad in (0, 1)
    return gemm(x, w, bias, conv=dict(H=H, W=W, Cin=cin, stride=stride, upsample2x=upsample2x, Ho=Ho, Wo=Wo, asym=int(pad == 0),
                                      up=(He, We) if upsample_to is not None else (0, 0)), **kw), Ho, Wo


# ----------------------------------------------------------------------------- attention
def attention(q, k0, v0t, Lk0, *, B, Lq, heads, d, scale, seg0_div=1, k1=None, v1t=None, Lk1=0, seg1_div=1,
              seg1_first_batch=0, seg1_skip=0, seg1_row=None, causal=False, out=None) -> torch.Tensor:
    """q (B*Lq, >=heads*d) rows view; k0 rows view; v0t (Bk, heads*d, ld) V^T tensors.
    seg1_row: device int32 tensor holding the bank row every batch >= seg1_first_batch reads (see emo_hip.h).
    causal: query row i sees keys j <= i only (one KV segment, Lq == Lk0 - emo_hip.h emo_attention_params.causal).
    out: optional (B*Lq, >=heads*d) rows view to write into (its stride(0) is ldo); allocated when None."""
    _need_cuda(q, k0, v0t, out)
    p = AttentionParams()
    pq, ldq = _rows(q)
    pk, ldk = _rows(k0)
    if out is None:
        out = torch.empty(B * Lq, heads * d, device=q.device, dtype=q.dtype)
    assert out.dtype == q.dtype and out.shape[0] == B * Lq and out.shape[1] >= heads * d, (out.shape, out.dtype)
    po, ldo = _rows(out)
    p.q, p.ldq = pq.value, ldq
    p.k0, p.ldk0, p.v0t, p.ldv0t, p.Lk0 = pk.value, ldk, v0t.data_ptr(), v0t.stride(1), Lk0
    p.seg0_div = seg0_div
    if k1 is not None:
        pk1, ldk1 = _rows(k1)
        p.k1, p.ldk1, p.v1t, p.ldv1t, p.Lk1 = pk1.value, ldk1, v1t.data_ptr(), v1t.stride(1), Lk1
        p.seg1_div, p.seg1_first_batch, p.seg1_skip = seg1_div, seg1_first_batch, seg1_skip
        if seg1_row is not None:
            assert seg1_row.dtype == torch.int32 and seg1_row.is_cuda
            p.seg1_row = seg1_row.data_ptr()
    else:
        p.seg1_div = 1
    p.out, p.ldo = po.value, ldo
    p.B, p.Lq, p.heads, p.d, p.scale, p.dtype = B, Lq, heads, d, float(scale), dt(q)
    p.causal = int(bool(causal))
    esz = q.element_size()
    # (only the batch rows from seg1_first_batch on read the second segment - under CFG the uncond half does not)
    b1 = max(B - seg1_first_batch, 0) if k1 is not None else 0
    _launch("attention", 4.0 * heads * Lq * d * (B * Lk0 + b1 * Lk1), esz * heads * d * (2.0 * B * Lq + 2.0 * (B * Lk0 + b1 * Lk1)),
            lambda: check(_lib.load().emo_attention(C.byref(p), _stream()), "emo_attention"),
            tag=f"B={B} Lq={Lq} Lk={Lk0}+{Lk1} h={heads} d={d}" + (" causal" if causal else ""))
    return out


def attention_plan(*, dtype, B, Lq, Lk0, heads, d, Lk1=0, causal=False):
    """What ops.attention launches for this shape, asked of the library on the host (emo_hip.h emo_attention_plan; no GPU needed):
    (head-dim class in 16-byte chunks, loader rounds, ring depth, q tiles per block - > 1 = the resident walk -, causal).
    Lk1 > 0 = a second KV segment is present.  Contiguous operands; raises EmoHipError where emo_attention would refuse the shape."""
    p = AttentionParams()
    fake, Cc = 256, heads * d   # non-NULL, never dereferenced
    ld0, ld1 = (Lk0 + 7) // 8 * 8, (Lk1 + 7) // 8 * 8
    p.q, p.ldq, p.k0, p.ldk0, p.v0t, p.ldv0t, p.Lk0 = fake, Cc, fake, Cc, fake, ld0, Lk0
    p.seg0_div = p.seg1_div = 1
    if Lk1:
        p.k1, p.ldk1, p.v1t, p.ldv1t, p.Lk1 = fake, Cc, fake, ld1, Lk1
    p.out, p.ldo = fake, Cc
    p.B, p.Lq, p.heads, p.d, p.scale, p.dtype = B, Lq, heads, d, 1.0, dt(dtype)
    p.causal = int(bool(causal))
    plan = (C.c_int * 5)()
    check(_lib.load().emo_attention_plan(C.byref(p), plan), "emo_attention_plan")
    return tuple(plan)


def temporal_attention(qkv: torch.Tensor, B, F, HW, heads, d, scale, out=None) -> torch.Tensor:
    """out: optional (B*F*HW, >=heads*d) rows view to write into (its stride(0) is ldo); allocated when None."""
    _need_cuda(qkv, out)
    pq, ld = _rows(qkv)
    if out is None:
        out = torch.empty(B * F * HW, heads * d, device=qkv.device, dtype=qkv.dtype)
    assert out.dtype == qkv.dtype and out.shape[0] == B * F * HW and out.shape[1] >= heads * d, (out.shape, out.dtype)
    po, ldo = _rows(out)
    _launch("temporal_attention", 4.0 * B * HW * heads * F * F * d, qkv.element_size() * 4.0 * B * F * HW * heads * d,
            lambda: check(_lib.load().emo_temporal_attention(pq, ld, po, ldo, B, F, HW, heads, d, float(scale),
                                                             dt(qkv), _stream()), "emo_temporal_attention"),
            tag=f"B={B} F={F} HW={HW} h={heads} d={d}")
    return out


# ----------------------------------------------------------------------------- sampler
def sched_step(noise_pred, counter, latents, history, lat_in, *, C_, F, HW, guidance_scale, a, b, c_x, c, slot, c_noise, s_next,
               seed, step, eps_out=None):
    """One scheduler step (emo_sched_step): c / slot are 4-tuples (slot -1 = no ring entry)."""
    _need_cuda(noise_pred, counter, latents, history, lat_in, eps_out)
    assert noise_pred.dtype == counter.dtype == latents.dtype == torch.float32
    n = C_ * F * HW
    assert latents.numel() == n and noise_pred.numel() >= n and (lat_in is None or lat_in.numel() == n)
    assert all(s_ < 0 for s_ in slot) or (history is not None and history.numel() >= (max(slot) + 1) * n)
    p = _lib.SchedStepParams(guidance_scale=float(guidance_scale), a=float(a), b=float(b), c_x=float(c_x),
                             c=(C.c_float * 4)(*map(float, c)), slot=(C.c_int * 4)(*map(int, slot)), c_noise=float(c_noise),
                             s_next=float(s_next), seed=int(seed) & 0xFFFFFFFF, step=int(step) & 0xFFFFFFFF, scale_only=0)
    check(_lib.load().emo_sched_step(_ptr(noise_pred), _ptr(counter), _ptr(latents), _ptr(history), _ptr(lat_in), _ptr(eps_out),
                                     C_, F, HW, C.byref(p), _stream()), "emo_sched_step")


def sched_scale(latents, lat_in, *, C_, F, HW, s):
    """lat_in = s * latents (emo_sched_step, scale_only): the model input of the first step that runs"""
    _need_cuda(latents, lat_in)
    assert latents.numel() == lat_in.numel() == C_ * F * HW
    p = _lib.SchedStepParams(s_next=float(s), slot=(C.c_int * 4)(-1, -1, -1, -1), scale_only=1)
    check(_lib.load().emo_sched_step(None, None, _ptr(latents), None, _ptr(lat_in), None, C_, F, HW, C.byref(p), _stream()),
          "emo_sched_step")


def accumulate_window(pred_rows, noise_pred_branch, counter, frames_i32, *, C_, F, HW, add_counter):
    pp, ld = _rows(pred_rows)
    check(_lib.load().emo_accumulate_window(pp, ld, _ptr(noise_pred_branch), _ptr(counter), _ptr(frames_i32), frames_i32.numel(),
                                            C_, F, HW, int(add_counter), dt(pred_rows), _stream()), "emo_accumulate_window")


# ----------------------------------------------------------------------------- EMO conditioning ops (A17/A18)
_ACT = {"silu": 0, "relu": 1, "tanh": 2, "gelu": 3, "quick_gelu": 4}


def act(x: torch.Tensor, kind: str) -> torch.Tensor:
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.load().emo_act(_ptr(x), _ptr(y), x.numel(), _ACT[kind], dt(x), _stream()), "emo_act")
    return y


def speed_encode(v: torch.Tensor, centers: torch.Tensor, radii: torch.Tensor, dtype) -> torch.Tensor:
    _need_cuda(v, centers, radii)
    out = torch.empty(v.shape[0], centers.shape[0], device=v.device, dtype=dtype)
    check(_lib.load().emo_speed_encode(_ptr(v), _ptr(centers), _ptr(radii), _ptr(out), v.shape[0], centers.shape[0], dt(dtype),
                                       _stream()), "emo_speed_encode")
    return out


def speed_bucket(v: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    _need_cuda(v, centers)
    idx = torch.empty(v.shape[0], device=v.device, dtype=torch.int32)
    check(_lib.load().emo_speed_bucket(_ptr(v), _ptr(centers), _ptr(idx), v.shape[0], centers.shape[0], _stream()), "emo_speed_bucket")
    return idx


def gather_rows(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    out = torch.empty(idx.shape[0], table.shape[1], device=table.device, dtype=table.dtype)
    check(_lib.load().emo_gather_rows(_ptr(table), _ptr(idx), _ptr(out), idx.shape[0], table.shape[1], table.shape[0], dt(table),
                                      _stream()), "emo_gather_rows")
    return out


def text_embed(ids: torch.Tensor, tok_table: torch.Tensor, pos_table: torch.Tensor) -> torch.Tensor:
    """ids (B, L) integer ids -> (B*L, D) rows tok_table[ids] + pos_table[:L] in the tables' dtype (emo_text_embed).  The ids are
    checked against the vocabulary on the host, before upload: an id outside [0, V) raises IndexError, as nn.Embedding does."""
    _need_cuda(tok_table, pos_table)
    B, L = ids.shape
    V, D = tok_table.shape
    ids_cpu = ids.detach().to("cpu", torch.int64)
    if ids_cpu.numel() and (int(ids_cpu.min()) < 0 or int(ids_cpu.max()) >= V):
        raise IndexError(f"index out of range in self: token ids must lie in [0, {V}), got [{int(ids_cpu.min())}, {int(ids_cpu.max())}]")
    if L > pos_table.shape[0]:
        raise IndexError(f"sequence length {L} exceeds the {pos_table.shape[0]} position embeddings")
    assert tok_table.is_contiguous() and pos_table.is_contiguous() and pos_table.dtype == tok_table.dtype
    idx = ids_cpu.to(torch.int32).reshape(-1).to(tok_table.device)
    out = torch.empty(B * L, D, device=tok_table.device, dtype=tok_table.dtype)
    check(_lib.load().emo_text_embed(_ptr(idx), _ptr(tok_table), _ptr(pos_table), _ptr(out), B, L, D, V, pos_table.shape[0],
                                     dt(tok_table), _stream()), "emo_text_embed")
    return out


def add_rowbias(x: torch.Tensor, rb: torch.Tensor, rows_per_batch: int) -> torch.Tensor:
    px, ldx = _rows(x)
    pr, ldr = _rows(rb)
    y = torch.empty(x.shape[0], x.shape[1], device=x.device, dtype=x.dtype)
    check(_lib.load().emo_add_rowbias(px, ldx, pr, ldr, _ptr(y), y.stride(0), x.shape[0], x.shape[1], rows_per_batch, dt(x), _stream()),
          "emo_add_rowbias")
    return y


# ----------------------------------------------------------------------------- either side of the loop (VAE, audio front-end)
def softmax_rows(x: torch.Tensor, scale: float, out=None) -> torch.Tensor:
    """softmax(scale * x) over the columns of a rows view (M, N)."""
    _need_cuda(x)
    px, ldx = _rows(x)
    y = torch.empty(x.shape[0], x.shape[1], device=x.device, dtype=x.dtype) if out is None else out
    py, ldy = _rows(y)
    check(_lib.load().emo_softmax_rows(px, ldx, py, ldy, x.shape[0], x.shape[1], float(scale), dt(x), _stream()), "emo_softmax_rows")
    return y


def audio_windows(feats: torch.Tensor, m: int = 2, n: int = 2) -> torch.Tensor:
    """(T, D) -> (T, m+n+1, D): features of frames [t-m, t+n], zero-padded at the ends (Net.py:649-667)."""
    _need_cuda(feats)
    feats = feats.contiguous()
    T_, D = feats.shape
    out = torch.empty(T_, m + n + 1, D, device=feats.device, dtype=feats.dtype)
    check(_lib.load().emo_audio_windows(_ptr(feats), _ptr(out), T_, D, m, n, dt(feats), _stream()), "emo_audio_windows")
    return out


def rows_to_video(x: torch.Tensor, B, Cc, F, H, W, mul=0.5, add=0.5, lo=0.0, hi=1.0) -> torch.Tensor:
    """rows ((b f) h w, >= C) -> (B, C, F, H, W) f32 = clamp(x*mul + add, lo, hi) (EMOAnimationPipeline.py:303-306)."""
    _need_cuda(x)
    px, ld = _rows(x)
    y = torch.empty(B, Cc, F, H, W, device=x.device, dtype=torch.float32)
    check(_lib.load().emo_rows_to_video(px, ld, _ptr(y), B, Cc, F, H * W, float(mul), float(add), float(lo), float(hi), dt(x), _stream()),
          "emo_rows_to_video")
    return y


def rows_to_frames_u8(x: torch.Tensor, B, Cc, F, H, W, mul=0.5, add=0.5, lo=0.0, hi=1.0, out=None) -> torch.Tensor:
    """rows ((b f) h w, >= C) -> (B, F, H, W, C) uint8 = trunc(clamp(x*mul + add, lo, hi) * 255): decode_latents' tail and the
    `(x * 255).astype(uint8)` of save_videos_grid in one launch (emo_rows_to_frames_u8).  out: a contiguous uint8 tensor of B*F*H*W*C
    elements to write into (e.g. a slice of a longer clip)."""
    _need_cuda(x, out)
    px, ld = _rows(x)
    assert x.shape[0] == B * F * H * W and x.shape[1] >= Cc, (x.shape, B, Cc, F, H, W)
    if out is None:
        out = torch.empty(B, F, H, W, Cc, device=x.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == B * F * H * W * Cc, (out.dtype, out.shape)
    _launch("rows_to_frames_u8", 0.0, (x.element_size() + 1.0) * out.numel(),
            lambda: check(_lib.load().emo_rows_to_frames_u8(px, ld, _ptr(out), B, Cc, F, H * W, float(mul), float(add), float(lo), float(hi), dt(x),
                                                            _stream()), "emo_rows_to_frames_u8"))
    return out


JPEG_LAYOUTS = {(3, 2, 2): "4:2:0", (3, 2, 1): "4:2:2", (3, 1, 1): "4:4:4", (1, 1, 1): "grey"}      # (components, luminance h, v)


def _jpeg_layout(layout):
    layout = tuple(int(v) for v in layout)
    assert layout in JPEG_LAYOUTS, f"a layout is (components, luminance h, luminance v), one of {sorted(JPEG_LAYOUTS)}; got {layout}"
    return layout


def jpeg_bpm(layout) -> int:
    """blocks per MCU: the luminance blocks, Cb, Cr; one for a grey scan, which is not interleaved (T.81 A.2.2, A.2.3)"""
    nc, hs, vs = _jpeg_layout(layout)
    return 1 if nc == 1 else hs * vs + 2


def jpeg_grid(H: int, W: int, layout=(3, 2, 2)):
    """(MCU rows, MCU columns) of an (H, W) frame: MCUs of 8 h x 8 v pixels"""
    _, hs, vs = _jpeg_layout(layout)
    return (int(H) + 8 * vs - 1) // (8 * vs), (int(W) + 8 * hs - 1) // (8 * hs)


def jpeg_mcus(H: int, W: int, layout=(3, 2, 2)) -> int:
    """MCUs of an (H, W) frame in `layout`: 16x16 ones at 4:2:0 (for grey, the 8x8 blocks of the frame)"""
    mr, mc = jpeg_grid(H, W, layout)
    return mr * mc


def jpeg_blocks(frames: torch.Tensor, quant: torch.Tensor) -> torch.Tensor:
    """packed uint8 RGB frames (n, H, W, 3) -> quantised DCT coefficients int16 (n, MCUs, 6, 64): 4:2:0, blocks Y00 Y01 Y10 Y11 Cb Cr,
    zig-zag order, DC undifferenced (emo_jpeg_blocks; T.81 A.3.3 / A.3.4).  quant: device uint16 (2, 64), natural order."""
    _need_cuda(frames, quant)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous(), (frames.dtype, frames.shape)
    assert quant.dtype == torch.uint16 and quant.numel() == 128 and quant.is_contiguous(), (quant.dtype, quant.shape)
    n, H, W, _ = frames.shape
    coefs = torch.empty(n, jpeg_mcus(H, W), 6, 64, device=frames.device, dtype=torch.int16)
    _launch("jpeg_blocks", 0.0, float(frames.numel() + 2 * coefs.numel()),
            lambda: check(_lib.load().emo_jpeg_blocks(_ptr(frames), _ptr(coefs), n, H, W, _ptr(quant), _stream()), "emo_jpeg_blocks"),
            tag=f"{n}x{H}x{W}")
    return coefs


def _jpeg_entropy_args(coefs, huff):
    _need_cuda(coefs, huff)
    assert coefs.dtype == torch.int16 and coefs.dim() == 4 and tuple(coefs.shape[2:]) == (6, 64) and coefs.is_contiguous(), (coefs.dtype, coefs.shape)
    assert huff.dtype == torch.int32 and tuple(huff.shape) == (4, 256) and huff.is_contiguous(), (huff.dtype, huff.shape)
    return coefs.shape[0], coefs.shape[1]


def _jpeg_restart_mcus(restart_mcus):
    assert restart_mcus is None or (isinstance(restart_mcus, int) and not isinstance(restart_mcus, bool) and restart_mcus > 0), restart_mcus
    return restart_mcus


def jpeg_count_bits(coefs: torch.Tensor, huff: torch.Tensor, restart_mcus=None) -> torch.Tensor:
    """coefficients (n, MCUs, 6, 64) -> the Huffman-coded size of every block in bits, int32 (n, MCUs * 6) (emo_jpeg_count_bits; T.81
    F.1.2).  huff: device int32 (4, 256), length << 16 | code, DC luma / AC luma / DC chroma / AC chroma.  restart_mcus: None, or the
    restart interval in MCUs - the DC predictions return to 0 at every interval's first MCU (emo_jpeg_count_bits_ri; T.81 E.1.4)."""
    n, n_mcu = _jpeg_entropy_args(coefs, huff)
    counts = torch.empty(n, n_mcu * 6, device=coefs.device, dtype=torch.int32)
    if _jpeg_restart_mcus(restart_mcus) is None:
        call = lambda: check(_lib.load().emo_jpeg_count_bits(_ptr(coefs), _ptr(counts), n, n_mcu, _ptr(huff), _stream()), "emo_jpeg_count_bits")
    else:
        call = lambda: check(_lib.load().emo_jpeg_count_bits_ri(_ptr(coefs), _ptr(counts), n, n_mcu, restart_mcus, _ptr(huff), _stream()),
                             "emo_jpeg_count_bits_ri")
    _launch("jpeg_count_bits", 0.0, 2.0 * coefs.numel(), call)
    return counts


def jpeg_emit_bits(coefs: torch.Tensor, huff: torch.Tensor, bit_offsets: torch.Tensor, out: torch.Tensor, restart_mcus=None) -> torch.Tensor:
    """writes every block's codes MSB-first at its bit offset (int64 (n, MCUs * 6), from out's first bit) into out, a ZEROED uint8 buffer
    of a multiple of 4 bytes (emo_jpeg_emit_bits): unstuffed, unpadded streams.  restart_mcus as in jpeg_count_bits
    (emo_jpeg_emit_bits_ri)."""
    n, n_mcu = _jpeg_entropy_args(coefs, huff)
    _need_cuda(bit_offsets, out)
    assert bit_offsets.dtype == torch.int64 and bit_offsets.numel() == n * n_mcu * 6 and bit_offsets.is_contiguous(), (bit_offsets.dtype, bit_offsets.shape)
    assert out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous(), (out.dtype, out.shape)
    if _jpeg_restart_mcus(restart_mcus) is None:
        call = lambda: check(_lib.load().emo_jpeg_emit_bits(_ptr(coefs), _ptr(bit_offsets), _ptr(out), out.numel(), n, n_mcu, _ptr(huff), _stream()),
                             "emo_jpeg_emit_bits")
    else:
        call = lambda: check(_lib.load().emo_jpeg_emit_bits_ri(_ptr(coefs), _ptr(bit_offsets), _ptr(out), out.numel(), n, n_mcu, restart_mcus,
                                                               _ptr(huff), _stream()), "emo_jpeg_emit_bits_ri")
    _launch("jpeg_emit_bits", 0.0, 2.0 * coefs.numel() + out.numel(), call)
    return out


GIF_BINS = 32768                                 # (r >> 3, g >> 3, b >> 3)


def _gif_frames(frames):
    _need_cuda(frames)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous(), (frames.dtype, frames.shape)
    return frames.shape[:3]


def gif_histogram(frames: torch.Tensor, per_frame: bool = False) -> torch.Tensor:
    """packed uint8 RGB frames (n, H, W, 3) -> int64 (n if per_frame else 1, 32768, 4): per bin (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)
    the pixel count and the sums of R, G, B (emo_gif_histogram; 64-bit integer atomics, exact and independent of the order)."""
    n, H, W = _gif_frames(frames)
    hist = torch.zeros(n if per_frame else 1, GIF_BINS, 4, device=frames.device, dtype=torch.int64)
    _launch("gif_histogram", 0.0, float(frames.numel()),
            lambda: check(_lib.load().emo_gif_histogram(_ptr(frames), _ptr(hist), n, H, W, int(bool(per_frame)), _stream()), "emo_gif_histogram"),
            tag=f"{n}x{H}x{W}")
    return hist


def gif_map(frames: torch.Tensor, palettes: torch.Tensor, n_colors: int, dither_strength: int = 0) -> torch.Tensor:
    """frames (n, H, W, 3), palettes uint8 (1 | n, 256, 3) -> uint8 (n, H, W): per pixel the nearest of the first n_colors entries of
    its frame's palette, the lowest index on a tie (emo_gif_map).  dither_strength 1 .. 128 puts the 8x8 Bayer pattern on the pixels
    before the search; 0 does not."""
    n, H, W = _gif_frames(frames)
    _need_cuda(palettes)
    assert palettes.dtype == torch.uint8 and palettes.dim() == 3 and tuple(palettes.shape[1:]) == (256, 3) and palettes.shape[0] in (1, n) \
        and palettes.is_contiguous(), (palettes.dtype, palettes.shape)
    assert isinstance(n_colors, int) and 1 <= n_colors <= 256 and isinstance(dither_strength, int) and 0 <= dither_strength <= 128, \
        (n_colors, dither_strength)
    out = torch.empty(n, H, W, device=frames.device, dtype=torch.uint8)
    per_frame = int(palettes.shape[0] == n and n > 1)
    _launch("gif_map", 8.0 * n_colors * out.numel(), float(frames.numel() + out.numel()),
            lambda: check(_lib.load().emo_gif_map(_ptr(frames), _ptr(palettes), _ptr(out), n, H, W, n_colors, per_frame, dither_strength, _stream()),
                          "emo_gif_map"), tag=f"{n}x{H}x{W}")
    return out


def _gif_strips(indices, strip_rows):
    _need_cuda(indices)
    assert indices.dtype == torch.uint8 and indices.dim() == 3 and indices.is_contiguous(), (indices.dtype, indices.shape)
    n, H, W = indices.shape
    assert isinstance(strip_rows, int) and not isinstance(strip_rows, bool) and strip_rows >= 1, strip_rows
    strip_rows = min(strip_rows, H)
    return n, H, W, strip_rows, -(-H // strip_rows)


def gif_lzw_count(indices: torch.Tensor, strip_rows: int):
    """palette indices uint8 (n, H, W) -> (codes uint16 (n, strips, cap), n_codes int32 (n, strips), bits int32 (n, strips)): every
    strip of strip_rows rows LZW-coded from an empty dictionary (emo_gif_lzw_count; GIF89a Appendix F at code size 8); bits counts the
    Clear in front of a frame's first strip and the Clear / End of Information behind every strip."""
    n, H, W, strip_rows, strips = _gif_strips(indices, strip_rows)
    cap = int(_lib.load().emo_gif_lzw_codes_per_strip(H, W, strip_rows))
    codes = torch.empty(n, strips, cap, device=indices.device, dtype=torch.uint16)
    n_codes = torch.empty(n, strips, device=indices.device, dtype=torch.int32)
    bits = torch.empty(n, strips, device=indices.device, dtype=torch.int32)
    _launch("gif_lzw_count", 0.0, float(indices.numel()),
            lambda: check(_lib.load().emo_gif_lzw_count(_ptr(indices), _ptr(codes), _ptr(n_codes), _ptr(bits), n, H, W, strip_rows, _stream()),
                          "emo_gif_lzw_count"), tag=f"{n}x{H}x{W}/{strip_rows}")
    return codes, n_codes, bits


def gif_lzw_emit(codes: torch.Tensor, n_codes: torch.Tensor, bit_offsets: torch.Tensor, out: torch.Tensor, H: int, W: int, strip_rows: int):
    """writes every strip's codes, least significant bit first, at its bit offset (int64 (n, strips), from out's first bit) into out, a
    ZEROED uint8 buffer of a multiple of 4 bytes (emo_gif_lzw_emit)."""
    _need_cuda(codes, n_codes, bit_offsets, out)
    n, strips, cap = codes.shape
    assert codes.dtype == torch.uint16 and codes.is_contiguous() and strip_rows >= 1 and strips == -(-H // min(strip_rows, H)) \
        and cap == int(_lib.load().emo_gif_lzw_codes_per_strip(H, W, strip_rows)), (codes.dtype, codes.shape, H, W, strip_rows)
    assert n_codes.dtype == torch.int32 and tuple(n_codes.shape) == (n, strips) and n_codes.is_contiguous(), (n_codes.dtype, n_codes.shape)
    assert bit_offsets.dtype == torch.int64 and tuple(bit_offsets.shape) == (n, strips) and bit_offsets.is_contiguous(), (bit_offsets.dtype, bit_offsets.shape)
    assert out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous(), (out.dtype, out.shape)
    _launch("gif_lzw_emit", 0.0, 2.0 * codes.numel() + out.numel(),
            lambda: check(_lib.load().emo_gif_lzw_emit(_ptr(codes), _ptr(n_codes), _ptr(bit_offsets), _ptr(out), out.numel(), n, H, W, strip_rows,
                                                       _stream()), "emo_gif_lzw_emit"), tag=f"{n}x{H}x{W}/{strip_rows}")
    return out


PNG_SYMBOLS = 320                                # slots 0 .. 285: literal / length symbols, 288 .. 317: distance symbols
PNG_MAX_STRIP_BYTES = 65535
PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}


def _png_frames(frames):
    _need_cuda(frames)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.is_contiguous(), (frames.dtype, frames.shape)
    return tuple(int(s) for s in frames.shape)


def png_filter(frames: torch.Tensor, filter: int = 5):
    """packed uint8 frames (n, H, W, C), C in 1 | 3 | 4 -> (filtered uint8 (n, H, 1 + W * C): per scanline the filter type and the
    filtered bytes, adler int32 (n, H, 2): the Adler-32 pair of every filtered row) (emo_png_filter).  filter 0 .. 4: None, Sub, Up,
    Average, Paeth for all rows; 5: per row the type with the smallest sum of min(v, 256 - v)."""
    n, H, W, C = _png_frames(frames)
    filtered = torch.empty(n, H, 1 + W * C, device=frames.device, dtype=torch.uint8)
    adler = torch.empty(n, H, 2, device=frames.device, dtype=torch.int32)
    _launch("png_filter", 0.0, 2.0 * frames.numel(),
            lambda: check(_lib.load().emo_png_filter(_ptr(frames), _ptr(filtered), _ptr(adler), n, H, W, C, int(filter), _stream()), "emo_png_filter"),
            tag=f"{n}x{H}x{W}x{C}")
    return filtered, adler


def _png_strips(filtered, channels, strip_rows):
    _need_cuda(filtered)
    assert filtered.dtype == torch.uint8 and filtered.dim() == 3 and filtered.is_contiguous(), (filtered.dtype, filtered.shape)
    n, H, R = (int(s) for s in filtered.shape)
    assert isinstance(channels, int) and channels >= 1 and (R - 1) % channels == 0 and R > 1, (R, channels)
    assert isinstance(strip_rows, int) and not isinstance(strip_rows, bool) and strip_rows >= 1, strip_rows
    strip_rows = min(strip_rows, H)
    return n, H, (R - 1) // channels, strip_rows, -(-H // strip_rows)


def png_lz_count(filtered: torch.Tensor, channels: int, strip_rows: int):
    """filtered scanlines uint8 (n, H, 1 + W * channels) -> (tokens int32 (n, strips, cap), n_tokens int32 (n, strips), hist int32
    (n, 320)): every strip of strip_rows scanlines tokenised on its own by the greedy single-probe LZ77 of emo_png_lz_count; hist counts
    the frame's literal / length and distance symbols and its one end-of-block."""
    n, H, W, strip_rows, strips = _png_strips(filtered, channels, strip_rows)
    cap = int(_lib.load().emo_png_tokens_per_strip(H, W, channels, strip_rows))
    tokens = torch.empty(n, strips, cap, device=filtered.device, dtype=torch.int32)
    n_tokens = torch.empty(n, strips, device=filtered.device, dtype=torch.int32)
    hist = torch.zeros(n, PNG_SYMBOLS, device=filtered.device, dtype=torch.int32)
    _launch("png_lz_count", 0.0, float(filtered.numel()),
            lambda: check(_lib.load().emo_png_lz_count(_ptr(filtered), _ptr(tokens), _ptr(n_tokens), _ptr(hist), n, H, W, channels, strip_rows,
                                                       _stream()), "emo_png_lz_count"), tag=f"{n}x{H}x{W}x{channels}/{strip_rows}")
    return tokens, n_tokens, hist


def _png_coded(tokens, n_tokens, codes, H, W, channels, strip_rows):
    _need_cuda(tokens, n_tokens, codes)
    n, strips, cap = (int(s) for s in tokens.shape)
    assert tokens.dtype == torch.int32 and tokens.is_contiguous() and strip_rows >= 1 and strips == -(-H // min(strip_rows, H)) \
        and cap == int(_lib.load().emo_png_tokens_per_strip(H, W, channels, strip_rows)), (tokens.dtype, tokens.shape, H, W, channels, strip_rows)
    assert n_tokens.dtype == torch.int32 and tuple(n_tokens.shape) == (n, strips) and n_tokens.is_contiguous(), (n_tokens.dtype, n_tokens.shape)
    assert codes.dtype == torch.int32 and tuple(codes.shape) == (n, PNG_SYMBOLS) and codes.is_contiguous(), (codes.dtype, codes.shape)
    return n, strips


def png_deflate_bits(tokens: torch.Tensor, n_tokens: torch.Tensor, codes: torch.Tensor, H: int, W: int, channels: int, strip_rows: int):
    """-> int32 (n, strips): the bits of every strip's tokens under its frame's table, codes int32 (n, 320) of `length << 16 | the
    bit-reversed code` (emo_png_deflate_bits)."""
    n, strips = _png_coded(tokens, n_tokens, codes, H, W, channels, strip_rows)
    bits = torch.empty(n, strips, device=tokens.device, dtype=torch.int32)
    _launch("png_deflate_bits", 0.0, 4.0 * tokens.numel(),
            lambda: check(_lib.load().emo_png_deflate_bits(_ptr(tokens), _ptr(n_tokens), _ptr(codes), _ptr(bits), n, H, W, channels, strip_rows,
                                                           _stream()), "emo_png_deflate_bits"), tag=f"{n}x{H}x{W}x{channels}/{strip_rows}")
    return bits


def png_deflate_emit(tokens: torch.Tensor, n_tokens: torch.Tensor, codes: torch.Tensor, bit_offsets: torch.Tensor, out: torch.Tensor, H: int,
                     W: int, channels: int, strip_rows: int):
    """writes every strip's tokens, least significant bit first, at its bit offset (int64 (n, strips), from out's first bit) into out, a
    ZEROED uint8 buffer of a multiple of 4 bytes (emo_png_deflate_emit)."""
    n, strips = _png_coded(tokens, n_tokens, codes, H, W, channels, strip_rows)
    _need_cuda(bit_offsets, out)
    assert bit_offsets.dtype == torch.int64 and tuple(bit_offsets.shape) == (n, strips) and bit_offsets.is_contiguous(), (bit_offsets.dtype, bit_offsets.shape)
    assert out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous(), (out.dtype, out.shape)
    _launch("png_deflate_emit", 0.0, 4.0 * tokens.numel() + out.numel(),
            lambda: check(_lib.load().emo_png_deflate_emit(_ptr(tokens), _ptr(n_tokens), _ptr(codes), _ptr(bit_offsets), _ptr(out), out.numel(), n,
                                                           H, W, channels, strip_rows, _stream()), "emo_png_deflate_emit"),
            tag=f"{n}x{H}x{W}x{channels}/{strip_rows}")
    return out


PNG_STATUS = {0: "ok", 1: "a block of type 3", 2: "a stored block whose NLEN is not the complement of its LEN",
              3: "a set of code lengths that makes no Huffman code", 4: "a symbol or bits that the block's codes do not define",
              5: "a distance that reaches in front of the frame's first byte", 6: "the stream ends inside a block",
              7: "more bytes than the frame's scanlines hold", 8: "the last block ends before the frame's last scanline",
              9: "a scanline with a filter type above 4"}   # EMO_PNG_OK / _BAD_BLOCK / _BAD_STORED / _BAD_LENGTHS / _BAD_SYMBOL / _BAD_DISTANCE /
#                                                             _PAST_END / _OVERFLOW / _SHORT / _BAD_FILTER


def png_inflate(streams: torch.Tensor, offsets: torch.Tensor, H: int, W: int, channels: int, out=None, produced=None, status=None):
    """the raw deflate streams of n frames (uint8, a multiple of 4 bytes; frame i in bytes offsets[i] .. offsets[i + 1], int64 (n + 1);
    zlib header and Adler-32 taken off) -> (filtered uint8 (n, H, 1 + W * channels), produced int32 (n), status int32 (n): a key of
    PNG_STATUS) (emo_png_inflate; RFC 1951).  channels 1 .. 4."""
    _need_cuda(streams, offsets)
    assert streams.dtype == torch.uint8 and streams.dim() == 1 and streams.is_contiguous(), (streams.dtype, streams.shape)
    assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.numel() >= 2 and offsets.is_contiguous(), (offsets.dtype, offsets.shape)
    n, H, W, channels = offsets.numel() - 1, int(H), int(W), int(channels)
    filtered = _jpeg_out(out, (n, H, 1 + W * channels), torch.uint8, streams.device, "filtered")
    produced = _jpeg_out(produced, (n,), torch.int32, streams.device, "produced")
    status = _jpeg_out(status, (n,), torch.int32, streams.device, "status")
    _launch("png_inflate", 0.0, float(streams.numel() + filtered.numel()),
            lambda: check(_lib.load().emo_png_inflate(_ptr(streams), streams.numel(), _ptr(offsets), _ptr(filtered), _ptr(produced), _ptr(status), n,
                                                      H, W, channels, _stream()), "emo_png_inflate"), tag=f"{n}x{H}x{W}x{channels}")
    return filtered, produced, status


def png_unfilter(filtered: torch.Tensor, channels: int, out=None, adler=None, status=None):
    """filtered scanlines uint8 (n, H, 1 + W * channels) -> (frames uint8 (n, H, W, channels), adler int32 (n, H, 2): the Adler-32 pair
    of every filtered row as png_filter gives it, status int32 (n): 0 or 9 of PNG_STATUS) (emo_png_unfilter; PNG 9.2 - 9.4)."""
    _need_cuda(filtered)
    assert filtered.dtype == torch.uint8 and filtered.dim() == 3 and filtered.is_contiguous(), (filtered.dtype, filtered.shape)
    n, H, R = (int(s) for s in filtered.shape)
    assert isinstance(channels, int) and channels >= 1 and (R - 1) % channels == 0 and R > 1, (R, channels)
    W = (R - 1) // channels
    frames = _jpeg_out(out, (n, H, W, channels), torch.uint8, filtered.device, "frames")
    adler = _jpeg_out(adler, (n, H, 2), torch.int32, filtered.device, "adler")
    status = _jpeg_out(status, (n,), torch.int32, filtered.device, "status")
    _launch("png_unfilter", 0.0, 2.0 * filtered.numel(),
            lambda: check(_lib.load().emo_png_unfilter(_ptr(filtered), _ptr(frames), _ptr(adler), _ptr(status), n, H, W, channels, _stream()),
                          "emo_png_unfilter"), tag=f"{n}x{H}x{W}x{channels}")
    return frames, adler, status


GIF_FRAME_INTS = 11                              # EMO_GIF_FRAME_INTS: left, top, w, h, transparent | -1, disposal, fill, interlace, table row, entries, slot | -1
GIF_STATUS = {0: "ok", 1: "a code the table does not define yet, or a code above Clear as the first of a table",
              2: "the image data ends before the frame's last pixel and before an End of Information",
              3: "End of Information before the frame's last pixel", 4: "a colour index at or beyond the frame's colour table",
              8: "a frame descriptor that does not fit its canvas, its indices or the tables"}
#                                                  EMO_GIF_OK / _BAD_CODE / _PAST_END / _SHORT / _BAD_INDEX / _BAD_FRAME (the last two are bits)


def gif_status_words(status: int) -> str:
    """a status of gif_lzw_decode or gif_compose in words (gif_compose ORs its two)"""
    status = int(status)
    if status in GIF_STATUS:
        return GIF_STATUS[status]
    words = [GIF_STATUS[b] for b in (4, 8) if status & b]
    return " and ".join(words) if words and not status & ~12 else f"status {status}"


def gif_layout_check(offsets, code_size, out_offsets, stream_bytes: int) -> int:
    """What emo_gif_lzw_decode cannot read before its launch, checked on HOST copies (sequences or numpy arrays) of its three device
    arrays: offsets (n + 1) ascending from >= 0 and inside the stream_bytes of the stream buffer, code_size (n) in 2 .. 8,
    out_offsets (n + 1) ascending from 0 with a sum of at most 2^31 - 1.  -> out_offsets[n], the bytes of `indices`.  EmoHipError
    (EMO_ERR_BAD_SHAPE in words) before any launch otherwise."""
    offsets, code_size, out_offsets = [[int(v) for v in a] for a in (offsets, code_size, out_offsets)]
    n = len(code_size)
    bad = None
    if n < 1 or len(offsets) != n + 1 or len(out_offsets) != n + 1:
        bad = f"n={n} frames with {len(offsets)} offsets and {len(out_offsets)} out_offsets (n >= 1, n + 1 each)"
    elif offsets[0] < 0 or offsets[-1] > int(stream_bytes) or any(b < a for a, b in zip(offsets, offsets[1:])):
        bad = f"offsets must ascend inside the {int(stream_bytes)} bytes of the streams, got {offsets[:4]} .. {offsets[-1]}"
    elif any(not 2 <= c <= 8 for c in code_size):
        bad = f"an LZW minimum code size of {next(c for c in code_size if not 2 <= c <= 8)}: GIF takes 2 .. 8"
    elif out_offsets[0] != 0 or any(b < a for a, b in zip(out_offsets, out_offsets[1:])):
        bad = f"out_offsets must ascend from 0, got {out_offsets[:4]} .. {out_offsets[-1]}"
    elif out_offsets[-1] > 2 ** 31 - 1 or out_offsets[-1] < 1:
        bad = f"{out_offsets[-1]} colour indices in all: the frames' pixels are counted in 31 bits, at least 1"
    if bad:
        raise _lib.EmoHipError(f"emo_gif_lzw_decode: bad shape: {bad}")
    return out_offsets[-1]


def gif_lzw_decode(streams: torch.Tensor, offsets: torch.Tensor, code_size: torch.Tensor, out_offsets: torch.Tensor, total: int, layout=None,
                   out=None, produced=None, status=None):
    """the LZW image data of n GIF frames (uint8, a multiple of 4 bytes; frame i in bytes offsets[i] .. offsets[i + 1], int64 (n + 1);
    sub-blocks joined), their minimum code sizes (int32 (n)) and where each frame's w * h colour indices go (out_offsets int64 (n + 1),
    from 0 to total) -> (indices uint8 (total), in stream order, produced int32 (n), status int32 (n): a key of GIF_STATUS)
    (emo_gif_lzw_decode; GIF89a Appendix F).  layout=(offsets, code_size, out_offsets) as host sequences - the same values - is checked
    by gif_layout_check before the launch; a caller that leaves it out has checked them itself."""
    _need_cuda(streams, offsets, code_size, out_offsets)
    assert streams.dtype == torch.uint8 and streams.dim() == 1 and streams.is_contiguous(), (streams.dtype, streams.shape)
    assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.numel() >= 2 and offsets.is_contiguous(), (offsets.dtype, offsets.shape)
    n, total = offsets.numel() - 1, int(total)
    assert code_size.dtype == torch.int32 and tuple(code_size.shape) == (n,) and code_size.is_contiguous(), (code_size.dtype, code_size.shape)
    assert out_offsets.dtype == torch.int64 and tuple(out_offsets.shape) == (n + 1,) and out_offsets.is_contiguous(), (out_offsets.dtype, out_offsets.shape)
    if layout is not None and gif_layout_check(*layout, streams.numel()) != total:
        raise _lib.EmoHipError(f"emo_gif_lzw_decode: bad shape: out_offsets end at {int(layout[2][-1])}, total={total}")
    if not 1 <= total <= 2 ** 31 - 1:
        raise _lib.EmoHipError(f"emo_gif_lzw_decode: bad shape: total={total} colour indices (1 .. 2^31 - 1)")
    indices = _jpeg_out(out, (total,), torch.uint8, streams.device, "indices")
    produced = _jpeg_out(produced, (n,), torch.int32, streams.device, "produced")
    status = _jpeg_out(status, (n,), torch.int32, streams.device, "status")
    _launch("gif_lzw_decode", 0.0, float(streams.numel() + 2 * total),
            lambda: check(_lib.load().emo_gif_lzw_decode(_ptr(streams), streams.numel(), _ptr(offsets), _ptr(code_size), _ptr(out_offsets),
                                                         _ptr(indices), _ptr(produced), _ptr(status), n, _stream()), "emo_gif_lzw_decode"),
            tag=f"{n}x{total}")
    return indices, produced, status


def gif_compose(indices: torch.Tensor, out_offsets: torch.Tensor, frames: torch.Tensor, tables: torch.Tensor, n_out: int, H: int, W: int,
                out=None, status=None):
    """colour indices in stream order as gif_lzw_decode leaves them, the frames' descriptors (int32 (n, GIF_FRAME_INTS)) and the colour
    tables (uint8 (n_tables, 256, 3)) -> (rgb uint8 (n_out, H, W, 3): the canvas right after each frame whose slot is 0 .. n_out - 1,
    status int32 (n): 0, or bits 4 / 8 of GIF_STATUS) (emo_gif_compose; GIF89a sections 18 - 23, Appendix E)."""
    _need_cuda(indices, out_offsets, frames, tables)
    assert indices.dtype == torch.uint8 and indices.dim() == 1 and indices.is_contiguous(), (indices.dtype, indices.shape)
    assert frames.dtype == torch.int32 and frames.dim() == 2 and frames.shape[1] == GIF_FRAME_INTS and frames.is_contiguous(), (frames.dtype, frames.shape)
    n = int(frames.shape[0])
    assert out_offsets.dtype == torch.int64 and tuple(out_offsets.shape) == (n + 1,) and out_offsets.is_contiguous(), (out_offsets.dtype, out_offsets.shape)
    assert tables.dtype == torch.uint8 and tables.dim() == 3 and tuple(tables.shape[1:]) == (256, 3) and tables.is_contiguous(), (tables.dtype, tables.shape)
    n_out, H, W = int(n_out), int(H), int(W)
    rgb = _jpeg_out(out, (max(n_out, 0), max(H, 0), max(W, 0), 3), torch.uint8, indices.device, "rgb")
    status = _jpeg_out(status, (n,), torch.int32, indices.device, "status")
    _launch("gif_compose", 0.0, float(indices.numel() + rgb.numel()),
            lambda: check(_lib.load().emo_gif_compose(_ptr(indices), _ptr(out_offsets), _ptr(frames), _ptr(tables), _ptr(rgb), _ptr(status), n,
                                                      int(tables.shape[0]), n_out, H, W, _stream()), "emo_gif_compose"), tag=f"{n}x{H}x{W}")
    return rgb, status


JPEG_DECODE_TABLE_INTS = 320                     # EMO_JPEG_DECODE_TABLE_INTS
JPEG_STATUS = {0: "ok", 1: "a code the Huffman table does not define", 2: "the scan ends before the frame's last block",
               3: "a zero run leaves its block"}   # EMO_JPEG_OK / _BAD_CODE / _PAST_END / _BAD_RUN


def _jpeg_out(out, shape, dtype, device, what):
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    _need_cuda(out)
    assert out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous(), (what, out.dtype, out.shape, shape)
    return out


def _jpeg_scan_args(scan, offsets, tables):
    """what both entropy decoders check of their scan buffer, its offsets and the four decoding tables -> len(offsets) - 1"""
    assert scan.dtype == torch.uint8 and scan.dim() == 1 and scan.is_contiguous(), (scan.dtype, scan.shape)
    assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.numel() >= 2 and offsets.is_contiguous(), (offsets.dtype, offsets.shape)
    assert tables.dtype == torch.int32 and tuple(tables.shape) == (4, JPEG_DECODE_TABLE_INTS) and tables.is_contiguous(), (tables.dtype, tables.shape)
    return offsets.numel() - 1


def jpeg_decode_bits(scan: torch.Tensor, offsets: torch.Tensor, tables: torch.Tensor, n_mcu: int, layout=(3, 2, 2), out=None, status=None):
    """the unstuffed scans of n frames in `layout`, a key of JPEG_LAYOUTS (uint8, a multiple of 4 bytes; frame i in bytes offsets[i] ..
    offsets[i + 1], int64 (n + 1)) -> (coefficients int16 (n, n_mcu, bpm, 64) - at 4:2:0 jpeg_blocks' layout -, status int32 (n): a key
    of JPEG_STATUS) (emo_jpeg_decode_bits; T.81 A.2.3, F.2.2).  tables: device int32 (4, JPEG_DECODE_TABLE_INTS),
    video_io.huffman_decode_table of DC luma / AC luma / DC chroma / AC chroma: the first pair decodes component 0, the second Cb and Cr."""
    _need_cuda(scan, offsets, tables)
    nc, hs, vs = _jpeg_layout(layout)
    n, n_mcu = _jpeg_scan_args(scan, offsets, tables), int(n_mcu)
    coefs = _jpeg_out(out, (n, n_mcu, jpeg_bpm(layout), 64), torch.int16, scan.device, "coefs")
    status = _jpeg_out(status, (n,), torch.int32, scan.device, "status")
    _launch("jpeg_decode_bits", 0.0, float(scan.numel() + 2 * coefs.numel()),
            lambda: check(_lib.load().emo_jpeg_decode_bits(_ptr(scan), scan.numel(), _ptr(offsets), _ptr(tables), _ptr(coefs), _ptr(status), n, n_mcu,
                                                           nc, hs, vs, _stream()), "emo_jpeg_decode_bits"),
            tag=f"{JPEG_LAYOUTS[(nc, hs, vs)]} {n}x{n_mcu}")
    return coefs, status


def jpeg_decode_segments(scan: torch.Tensor, seg_offsets: torch.Tensor, seg_first_block: torch.Tensor, seg_blocks: torch.Tensor,
                         tables: torch.Tensor, n: int, n_mcu: int, layout=(3, 2, 2), out=None, status=None):
    """unstuffed segments (restart intervals, or whole frames without restart markers; segment s in bytes seg_offsets[s] ..
    seg_offsets[s + 1] of scan, int64 (n_seg + 1)) -> (coefficients int16 (n, n_mcu, bpm, 64), status int32 (n_seg), a key of JPEG_STATUS
    PER SEGMENT) (emo_jpeg_decode_segments; T.81 E.1.4, F.2.2).  Segment s fills seg_blocks[s] blocks from block seg_first_block[s] on of
    the whole coefficient buffer (both int32 (n_seg), in blocks, bpm to an MCU); blocks no segment names are not written.  scan, tables
    and layout as in jpeg_decode_bits."""
    _need_cuda(scan, seg_offsets, seg_first_block, seg_blocks, tables)
    nc, hs, vs = _jpeg_layout(layout)
    n_seg = _jpeg_scan_args(scan, seg_offsets, tables)
    for tab in (seg_first_block, seg_blocks):
        assert tab.dtype == torch.int32 and tuple(tab.shape) == (n_seg,) and tab.is_contiguous(), (tab.dtype, tab.shape, n_seg)
    n, n_mcu, bpm = int(n), int(n_mcu), jpeg_bpm(layout)
    coefs = _jpeg_out(out, (n, n_mcu, bpm, 64), torch.int16, scan.device, "coefs")
    status = _jpeg_out(status, (n_seg,), torch.int32, scan.device, "status")
    _launch("jpeg_decode_segments", 0.0, float(scan.numel() + 2 * coefs.numel()),
            lambda: check(_lib.load().emo_jpeg_decode_segments(_ptr(scan), scan.numel(), _ptr(seg_offsets), _ptr(seg_first_block), _ptr(seg_blocks),
                                                               _ptr(tables), _ptr(coefs), n * n_mcu * bpm, _ptr(status), n_seg, nc, hs, vs,
                                                               _stream()), "emo_jpeg_decode_segments"),
            tag=f"{JPEG_LAYOUTS[(nc, hs, vs)]} {n_seg}/{n}x{n_mcu}")
    return coefs, status


def jpeg_idct(coefs: torch.Tensor, quant: torch.Tensor, H: int, W: int, layout=(3, 2, 2), out_y=None, out_c=None):
    """coefficients int16 (n, MCUs, bpm, 64) of (H, W) frames in `layout` -> (Y plane uint8 (n, mr * 8 v, mc * 8 h), Cb / Cr planes uint8
    (n, 2, mr * 8, mc * 8); None for grey), mr, mc = jpeg_grid(H, W, layout): dequantisation and libjpeg's integer IDCT (emo_jpeg_idct).
    quant: device uint16 (3, 64), one quantiser per component, natural order (a grey frame: its one table three times)."""
    _need_cuda(coefs, quant)
    nc, hs, vs = _jpeg_layout(layout)
    H, W = int(H), int(W)
    mr, mc = jpeg_grid(H, W, layout)
    assert coefs.dtype == torch.int16 and coefs.dim() == 4 and tuple(coefs.shape[1:]) == (mr * mc, jpeg_bpm(layout), 64) and coefs.is_contiguous(), (coefs.dtype, coefs.shape)
    assert quant.dtype == torch.uint16 and quant.numel() == 192 and quant.is_contiguous(), (quant.dtype, quant.shape)
    n = coefs.shape[0]
    y = _jpeg_out(out_y, (n, mr * 8 * vs, mc * 8 * hs), torch.uint8, coefs.device, "y plane")
    c = _jpeg_out(out_c, (n, 2, mr * 8, mc * 8), torch.uint8, coefs.device, "chroma planes") if nc == 3 else None
    _launch("jpeg_idct", 0.0, float(2 * coefs.numel() + y.numel() + (c.numel() if nc == 3 else 0)),
            lambda: check(_lib.load().emo_jpeg_idct(_ptr(coefs), _ptr(quant), _ptr(y), _ptr(c) if nc == 3 else None, n, H, W, nc, hs, vs, _stream()),
                          "emo_jpeg_idct"),
            tag=f"{JPEG_LAYOUTS[(nc, hs, vs)]} {n}x{H}x{W}")
    return y, c


def jpeg_rgb(y: torch.Tensor, c, H: int, W: int, layout=(3, 2, 2), out=None) -> torch.Tensor:
    """jpeg_idct's planes -> packed uint8 RGB frames (n, H, W, 3): libjpeg's chroma up-sampling of the layout (triangle filters where
    chroma is halved) and its fixed-point colour transform; a grey frame's sample in all three channels (emo_jpeg_rgb).  c: None for
    grey."""
    nc, hs, vs = _jpeg_layout(layout)
    _need_cuda(*((y, c) if nc == 3 else (y,)))
    H, W = int(H), int(W)
    mr, mc = jpeg_grid(H, W, layout)
    n = y.shape[0]
    assert y.dtype == torch.uint8 and tuple(y.shape) == (n, mr * 8 * vs, mc * 8 * hs) and y.is_contiguous(), (y.dtype, y.shape)
    if nc == 3:
        assert c.dtype == torch.uint8 and tuple(c.shape) == (n, 2, mr * 8, mc * 8) and c.is_contiguous(), (c.dtype, c.shape)
    rgb = _jpeg_out(out, (n, H, W, 3), torch.uint8, y.device, "frames")
    _launch("jpeg_rgb", 0.0, float(y.numel() + (c.numel() if nc == 3 else 0) + rgb.numel()),
            lambda: check(_lib.load().emo_jpeg_rgb(_ptr(y), _ptr(c) if nc == 3 else None, _ptr(rgb), n, H, W, nc, hs, vs, _stream()), "emo_jpeg_rgb"),
            tag=f"{JPEG_LAYOUTS[(nc, hs, vs)]} {n}x{H}x{W}")
    return rgb


def jpeg_scan_units(H: int, W: int, layout, scan_comp: int) -> int:
    """units of one scan of a progressive frame (T.81 A.2.2, A.2.3): MCUs when the scan is interleaved (scan_comp -1), else the 8x8
    blocks of component scan_comp's own ceil(W h / hs) x ceil(H v / vs) samples"""
    nc, hs, vs = _jpeg_layout(layout)
    scan_comp = int(scan_comp)
    assert -1 <= scan_comp < nc, (scan_comp, nc)
    if scan_comp < 0 or nc == 1:
        return jpeg_mcus(H, W, layout)
    h, v = (hs, vs) if scan_comp == 0 else (1, 1)
    return (((int(W) * h + hs - 1) // hs + 7) // 8) * (((int(H) * v + vs - 1) // vs + 7) // 8)


def jpeg_progressive_scan(scan: torch.Tensor, seg_offsets: torch.Tensor, seg_frame: torch.Tensor, seg_first_unit: torch.Tensor,
                          seg_units: torch.Tensor, seg_tables: torch.Tensor, tables: torch.Tensor, coefs: torch.Tensor, H: int, W: int, layout,
                          Ss: int, Se: int, Ah: int, Al: int, scan_comp: int, status=None) -> torch.Tensor:
    """ONE scan of a progression, decoded IN PLACE into coefs int16 (n, n_mcu, bpm, 64) - zeroed by the caller before the first scan -
    for all segments at once -> status int32 (n_seg), a key of JPEG_STATUS per segment (emo_jpeg_progressive_scan; T.81 Annex G).
    Segment s - a restart interval of this scan in one frame, or the frame's whole scan - lies in bytes seg_offsets[s] ..
    seg_offsets[s + 1] of scan (int64 (n_seg + 1)), belongs to frame seg_frame[s] and codes seg_units[s] units from seg_first_unit[s]
    on (int32 (n_seg) each; units as jpeg_scan_units counts them); seg_tables int32 (n_seg, 3) indexes tables, int32 (T,
    JPEG_DECODE_TABLE_INTS): the DC table of every component of an interleaved scan, or in column 0 the one table of a one-component
    scan.  scan_comp: -1 interleaved (DC scans only), else the component.  Only positions Ss .. Se of the blocks of the units are
    written; the launches of a progression follow each other in file order on the stream."""
    _need_cuda(scan, seg_offsets, seg_frame, seg_first_unit, seg_units, seg_tables, tables, coefs)
    nc, hs, vs = _jpeg_layout(layout)
    H, W, Ss, Se, Ah, Al, scan_comp = (int(v) for v in (H, W, Ss, Se, Ah, Al, scan_comp))
    assert scan.dtype == torch.uint8 and scan.dim() == 1 and scan.is_contiguous(), (scan.dtype, scan.shape)
    assert seg_offsets.dtype == torch.int64 and seg_offsets.dim() == 1 and seg_offsets.numel() >= 2 and seg_offsets.is_contiguous(), (seg_offsets.dtype, seg_offsets.shape)
    n_seg = seg_offsets.numel() - 1
    for tab in (seg_frame, seg_first_unit, seg_units):
        assert tab.dtype == torch.int32 and tuple(tab.shape) == (n_seg,) and tab.is_contiguous(), (tab.dtype, tab.shape, n_seg)
    assert seg_tables.dtype == torch.int32 and tuple(seg_tables.shape) == (n_seg, 3) and seg_tables.is_contiguous(), (seg_tables.dtype, seg_tables.shape)
    assert tables.dtype == torch.int32 and tables.dim() == 2 and tables.shape[0] >= 1 and tables.shape[1] == JPEG_DECODE_TABLE_INTS and tables.is_contiguous(), (tables.dtype, tables.shape)
    assert coefs.dtype == torch.int16 and coefs.dim() == 4 and coefs.shape[0] >= 1 and coefs.is_contiguous() and \
        tuple(coefs.shape[1:]) == (jpeg_mcus(H, W, layout), jpeg_bpm(layout), 64), (coefs.dtype, coefs.shape)
    assert -1 <= scan_comp < nc, f"scan_comp {scan_comp}: -1 (interleaved) or a component below {nc}"
    assert 0 <= Ss <= Se <= 63 and (Se == 0 if Ss == 0 else scan_comp >= 0), \
        f"a DC scan holds coefficient 0 alone, an AC scan a band inside 1 .. 63 of one component (T.81 G.1.1.1.1); got {Ss} .. {Se}, scan_comp {scan_comp}"
    assert 0 <= Al <= 13 and 0 <= Ah <= 13 and (Ah == 0 or Al == Ah - 1), f"Ah / Al {Ah} / {Al}: 0 .. 13, a refinement steps down by one bit"
    n = coefs.shape[0]
    status = _jpeg_out(status, (n_seg,), torch.int32, scan.device, "status")
    _launch("jpeg_progressive_scan", 0.0, float(scan.numel() + 2 * coefs.numel() * (Se - Ss + 1) / 64),
            lambda: check(_lib.load().emo_jpeg_progressive_scan(_ptr(scan), scan.numel(), _ptr(seg_offsets), _ptr(seg_frame), _ptr(seg_first_unit),
                                                                _ptr(seg_units), _ptr(seg_tables), _ptr(tables), tables.shape[0], _ptr(coefs),
                                                                _ptr(status), n_seg, n, H, W, nc, hs, vs, Ss, Se, Ah, Al, scan_comp, _stream()),
                          "emo_jpeg_progressive_scan"),
            tag=f"{JPEG_LAYOUTS[(nc, hs, vs)]} {n_seg}/{n}x{H}x{W} {Ss}..{Se} {Ah}/{Al} c{scan_comp}")
    return status


def image_resize(frames: torch.Tensor, h: int, w: int, xtaps=None, ytaps=None, out=None) -> torch.Tensor:
    """packed uint8 RGB frames (n, H, W, 3) -> (n, h, w, 3): Pillow's resize of 8-bit pixels, a horizontal integer pass to 8-bit pixels and
    a vertical one over those (emo_image_resize; animation.py:174-185).  xtaps / ytaps: (bounds int32 (w | h, 2), coef int32 (w | h, k))
    on the device, video_io.resize_taps of the axis; the pair of an axis that keeps its size is not read and may be None.  The
    intermediate image is allocated here."""
    _need_cuda(frames, out)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous(), (frames.dtype, frames.shape)
    n, H, W, _ = frames.shape
    h, w = int(h), int(w)
    tabs = []
    for taps, size_in, size_out, axis in ((xtaps, W, w, "x"), (ytaps, H, h, "y")):
        if size_in == size_out:
            tabs += [None, None, 0]
            continue
        if taps is None:
            raise ValueError(f"image_resize: the {axis} axis goes from {size_in} to {size_out} and has no tap tables")
        bounds, coef = taps
        _need_cuda(bounds, coef)
        assert bounds.dtype == torch.int32 and tuple(bounds.shape) == (size_out, 2) and bounds.is_contiguous(), (axis, bounds.dtype, bounds.shape)
        assert coef.dtype == torch.int32 and coef.dim() == 2 and coef.shape[0] == size_out and coef.is_contiguous(), (axis, coef.dtype, coef.shape)
        tabs += [bounds, coef, coef.shape[1]]
    lib = _lib.load()
    out = _jpeg_out(out, (n, h, w, 3), torch.uint8, frames.device, "frames")
    ws_bytes = lib.emo_image_resize_workspace_bytes(n, H, W, h, w)
    ws = torch.empty(ws_bytes, device=frames.device, dtype=torch.uint8) if ws_bytes else None
    _launch("image_resize", 0.0, float(frames.numel() + 2 * ws_bytes + out.numel()),
            lambda: check(lib.emo_image_resize(_ptr(frames), _ptr(out), n, H, W, h, w, _ptr(tabs[0]), _ptr(tabs[1]), tabs[2], _ptr(tabs[3]),
                                               _ptr(tabs[4]), tabs[5], _ptr(ws), ws_bytes, _stream()), "emo_image_resize"),
            tag=f"{n}x{H}x{W}->{h}x{w}")
    return out


INTERP_METHODS = {"linear": 0, "slerp": 1}


def interpolate_frames(latents: torch.Tensor, factor: int, method="slerp", dot_threshold: float = 0.9995, out=None, workspace=None) -> torch.Tensor:
    """f32 latents (B, C, F, H, W) -> (B, C, (F - 1) * factor + 1, H, W): `factor - 1` frames between every two consecutive frames, each
    frame taken as one vector over (B, C, H, W), by slerp (linear when |cos| > dot_threshold) or linear (emo_interp_frames;
    EMOAnimationPipeline.py:479-512, magicanimate/utils/util.py:125-138).  Two launches on the current stream, no host read: capturable.
    out / workspace: optional device buffers (workspace of >= emo_interp_frames_workspace_bytes bytes)."""
    _need_cuda(latents, out, workspace)
    assert latents.dtype == torch.float32 and latents.dim() == 5, (latents.dtype, latents.shape)
    latents = latents.contiguous()
    lib = _lib.load()
    B, Cc, F, H, W = latents.shape
    factor = int(factor)
    m = INTERP_METHODS[method] if isinstance(method, str) else int(method)
    if workspace is None:
        workspace = torch.empty(max(lib.emo_interp_frames_workspace_bytes(B, Cc, F, H * W) // 4, 1), device=latents.device, dtype=torch.float32)
    if out is None:
        out = torch.empty(B, Cc, max((F - 1) * factor + 1, 1), H, W, device=latents.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * Cc * max((F - 1) * factor + 1, 1) * H * W, (out.dtype, out.shape)
    _launch("interp_frames", 0.0, 4.0 * (3.0 * latents.numel() + out.numel()),
            lambda: check(lib.emo_interp_frames(_ptr(latents), _ptr(out), B, Cc, F, H * W, factor, m, float(dot_threshold), _ptr(workspace),
                                                workspace.numel() * workspace.element_size(), _stream()), "emo_interp_frames"),
            tag=f"F={F} k={factor}")
    return out


def channel_norm(x: torch.Tensor, gamma, beta, eps=1e-5, gelu=False) -> torch.Tensor:
    """nn.GroupNorm(C, C) over a sequence: x rows (S, C) normalised per channel over the S rows, affine, optional erf-GELU (emo_channelnorm)."""
    _need_cuda(x)
    lib = _lib.load()
    S, Cc = x.shape
    px, ldx = _rows(x)
    y = torch.empty(S, Cc, device=x.device, dtype=x.dtype)
    ws = torch.empty(max(lib.emo_channelnorm_workspace_bytes(S, Cc) // 4, 1), device=x.device, dtype=torch.float32)
    _launch("channelnorm", 0.0, x.element_size() * 3.0 * S * Cc,
            lambda: check(lib.emo_channelnorm(px, ldx, _ptr(gamma), _ptr(beta), _ptr(y), Cc, S, Cc, float(eps), int(bool(gelu)), _ptr(ws), dt(x), _stream()),
                          "emo_channelnorm"))
    return y


def wav_conv0_ln_act_ok(n: int, Cc: int, k: int, stride: int) -> bool:
    """whether emo_wav_conv0_ln_act serves this first-layer shape (host only; emo_wav_conv0_ln_act_plan)"""
    plan = (C.c_int64 * 6)()
    return _lib.load().emo_wav_conv0_ln_act_plan(int(n), int(Cc), int(k), int(stride), plan) == 0


def wav_conv0_ln_act(wave: torch.Tensor, w: torch.Tensor, bias, gamma, beta, stride: int, eps=1e-5, gelu=True, dtype=torch.float32,
                     out=None) -> torch.Tensor:
    """Conv1d(1, C, k, stride) + bias -> LayerNorm(C) -> optional erf-GELU per time step, straight from the f32 waveform (n,): ->
    ((n - k) // stride + 1, C) rows in `dtype` (emo_wav_conv0_ln_act).  w f32 (C, k); bias / gamma / beta f32 (C,).  out: a rows view
    in `dtype` to write into."""
    _need_cuda(wave, w, bias, gamma, beta, out)
    assert wave.dtype == w.dtype == torch.float32 and wave.dim() == 1 and w.dim() == 2 and wave.is_contiguous() and w.is_contiguous()
    n, (Cc, k) = wave.shape[0], w.shape
    T0 = max((n - k) // stride + 1, 1)
    y = torch.empty(T0, Cc, device=wave.device, dtype=dtype) if out is None else out
    assert y.shape == (T0, Cc), (y.shape, T0, Cc)
    py, ldy = _rows(y)
    _launch("wav_conv0_ln_act", 2.0 * T0 * Cc * k, 4.0 * n + y.element_size() * 1.0 * T0 * Cc,
            lambda: check(_lib.load().emo_wav_conv0_ln_act(_ptr(wave), n, _ptr(w), _ptr(bias), _ptr(gamma), _ptr(beta), py, ldy, Cc, k, int(stride),
                                                           float(eps), int(bool(gelu)), dt(y), _stream()), "emo_wav_conv0_ln_act"),
            tag=f"n={n} C={Cc} k={k} s={stride}")
    return y


def audio_resample(frames: torch.Tensor, taps: torch.Tensor, up: int, down: int, half: int, in_start: int = 0, out_start: int = 0,
                   n_out: int = None) -> torch.Tensor:
    """Interleaved f32 frames (n_in, channels) holding global frames in_start .. -> the n_out mono samples from global output index
    out_start on, resampled by up / down: y[n] = sum_j h[n * down - j * up] * mean_c frames[j, c] (emo_audio_resample; Net.py:627-640).
    taps: the f32 phase table (up, taps_per_phase) of emote_hack_amd.audio_io.phase_table.  n_out defaults to the whole utterance,
    ceil(n_in * up / down) (with in_start = out_start = 0)."""
    _need_cuda(frames, taps)
    assert frames.dtype == torch.float32 and frames.dim() == 2 and frames.is_contiguous(), (frames.dtype, frames.shape)
    assert taps.dtype == torch.float32 and taps.dim() == 2 and taps.is_contiguous(), (taps.dtype, taps.shape)
    n_in, ch = frames.shape
    if n_out is None:
        n_out = -(-n_in * up // down)
    out = torch.empty(n_out, device=frames.device, dtype=torch.float32)
    _launch("audio_resample", 2.0 * n_out * taps.shape[1], 4.0 * (frames.numel() + n_out),
            lambda: check(_lib.load().emo_audio_resample(_ptr(frames), int(in_start), n_in, ch, _ptr(taps), taps.numel(), int(up), int(down), int(half),
                                                         _ptr(out), int(out_start), int(n_out), _stream()), "emo_audio_resample"),
            tag=f"{up}/{down}")
    return out


def waveform_normalize(x: torch.Tensor, eps: float = 1e-7, workspace: torch.Tensor = None) -> torch.Tensor:
    """(x - mean) / sqrt(var + eps) over the n f32 samples of one utterance, population variance, two passes in a fixed order
    (emo_waveform_normalize; Net.py:639).  workspace: optional device buffer of >= emo_waveform_normalize_workspace_bytes(n) bytes."""
    _need_cuda(x, workspace)
    assert x.dtype == torch.float32 and x.is_contiguous(), (x.dtype, x.shape)
    lib = _lib.load()
    n = x.numel()
    if workspace is None:
        workspace = torch.empty(max(lib.emo_waveform_normalize_workspace_bytes(n) // 4, 1), device=x.device, dtype=torch.float32)
    y = torch.empty_like(x)
    _launch("waveform_normalize", 0.0, 16.0 * n,
            lambda: check(lib.emo_waveform_normalize(_ptr(x), _ptr(y), n, float(eps), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                                     _stream()), "emo_waveform_normalize"))
    return y


def maxpool2x2(x: torch.Tensor, n_img: int, H: int, W: int) -> torch.Tensor:
    """nn.MaxPool2d(2, 2) over NHWC rows (Net.py:828)."""
    _need_cuda(x)
    px, ldx = _rows(x)
    y = torch.empty(n_img * (H // 2) * (W // 2), x.shape[1], device=x.device, dtype=x.dtype)
    check(_lib.load().emo_maxpool2x2(px, ldx, _ptr(y), y.stride(0), n_img, H, W, x.shape[1], dt(x), _stream()), "emo_maxpool2x2")
    return y


def bilinear_to_nchw(x: torch.Tensor, n_img: int, Cc: int, h: int, w: int, Ho: int, Wo: int) -> torch.Tensor:
    """F.interpolate(size=(Ho, Wo), mode='bilinear', align_corners=False) of NHWC rows into (n, C, Ho, Wo) f32 (Net.py:851)."""
    _need_cuda(x)
    px, ld = _rows(x)
    y = torch.empty(n_img, Cc, Ho, Wo, device=x.device, dtype=torch.float32)
    check(_lib.load().emo_bilinear_to_nchw(px, ld, _ptr(y), n_img, Cc, h, w, Ho, Wo, dt(x), _stream()), "emo_bilinear_to_nchw")
    return y


# ----------------------------------------------------------------------------- CLIP vision encoder front
def image_preprocess(frames: torch.Tensor, S: int, ytap, yw, xtap, xw, span_max: int, rescale, mean, std) -> torch.Tensor:
    """uint8 RGB frames (n, H, W, 3) -> f32 pixel_values (n, 3, S, S): transformers' CLIPImageProcessor as one launch
    (emo_image_preprocess).  ytap / xtap int32 (S, 2) and yw / xw f32 (S, k) are the per-axis tap tables of the crop window
    (emote_hack_amd.clip_vision.resize_crop_taps builds them on the host); rescale, mean[3], std[3] are host scalars."""
    _need_cuda(frames, ytap, yw, xtap, xw)
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous(), (frames.dtype, frames.shape)
    n, H, W, _ = frames.shape
    for tap, wt in ((ytap, yw), (xtap, xw)):
        assert tap.dtype == torch.int32 and tuple(tap.shape) == (S, 2) and tap.is_contiguous(), (tap.dtype, tap.shape)
        assert wt.dtype == torch.float32 and wt.dim() == 2 and wt.shape[0] == S and wt.is_contiguous(), (wt.dtype, wt.shape)
    out = torch.empty(n, 3, S, S, device=frames.device, dtype=torch.float32)
    m3, s3 = (C.c_float * 3)(*map(float, mean)), (C.c_float * 3)(*map(float, std))
    _launch("image_preprocess", 0.0, float(frames.numel()) + 4.0 * out.numel(),
            lambda: check(_lib.load().emo_image_preprocess(_ptr(frames), _ptr(out), n, H, W, S, _ptr(ytap), _ptr(yw), yw.shape[1], _ptr(xtap),
                                                           _ptr(xw), xw.shape[1], int(span_max), float(rescale), m3, s3, _stream()),
                          "emo_image_preprocess"), tag=f"n={n} {H}x{W}->{S}")
    return out


def patch_rows(pixel_values: torch.Tensor, patch: int, dtype) -> torch.Tensor:
    """pixel_values (B, 3, S, S) f32 -> (B * (S / patch)^2, ld) GEMM A rows in `dtype`, columns (c, py, px), ld = 3 * patch^2 rounded up
    to 8 with zero pad columns (emo_patch_rows)."""
    _need_cuda(pixel_values)
    assert pixel_values.dtype == torch.float32 and pixel_values.dim() == 4 and pixel_values.shape[1] == 3, (pixel_values.dtype, pixel_values.shape)
    pixel_values = pixel_values.contiguous()
    B, _, S, S2 = pixel_values.shape
    assert S == S2 and S % patch == 0, (S, S2, patch)
    ld = (3 * patch * patch + 7) // 8 * 8
    out = torch.empty(B * (S // patch) ** 2, ld, device=pixel_values.device, dtype=dtype)
    _launch("patch_rows", 0.0, 4.0 * pixel_values.numel() + out.element_size() * float(out.numel()),
            lambda: check(_lib.load().emo_patch_rows(_ptr(pixel_values), _ptr(out), B, S, patch, ld, dt(dtype), _stream()), "emo_patch_rows"))
    return out


def vision_embed(patch_out: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, gamma, beta, B: int, eps=1e-5) -> torch.Tensor:
    """patch_out (B * Np, C) rows, cls (C,), pos (Np + 1, C) in the compute dtype, gamma / beta f32 -> (B * (Np + 1), C) rows
    LayerNorm([cls | patch rows] + pos): token assembly and pre_layrnorm in one launch (emo_vision_embed)."""
    _need_cuda(patch_out, cls, pos, gamma, beta)
    pp, ldp = _rows(patch_out)
    Cc = patch_out.shape[1]
    Np = patch_out.shape[0] // B
    assert patch_out.shape[0] == B * Np and tuple(pos.shape) == (Np + 1, Cc) and tuple(cls.shape) == (Cc,), (patch_out.shape, pos.shape, cls.shape)
    assert pos.is_contiguous() and cls.is_contiguous() and pos.dtype == cls.dtype == patch_out.dtype
    assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == Cc
    y = torch.empty(B * (Np + 1), Cc, device=patch_out.device, dtype=patch_out.dtype)
    _launch("vision_embed", 0.0, patch_out.element_size() * (2.0 * B * (Np + 1) * Cc + (Np + 1) * Cc),
            lambda: check(_lib.load().emo_vision_embed(pp, ldp, _ptr(cls), _ptr(pos), _ptr(gamma), _ptr(beta), _ptr(y), Cc, B, Np, Cc, float(eps),
                                                       dt(patch_out), _stream()), "emo_vision_embed"))
    return y
