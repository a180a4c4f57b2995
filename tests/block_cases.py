"""Case tables of the block-level parity tests, shared by tests/test_gpu_blocks.py (which runs the block methods of
emote_hack_amd/unet.py on the device) and tests/test_block_cases_host.py (which asks the library on the host what every case launches,
and checks on the CPU that the oracle itself reacts to what each case is meant to pin).  Plain data plus host-side helpers: nothing here
touches a device.

  GOLDEN_BLOCKS    tests/golden/modules.safetensors -> the block of a host model with the golden's geometry, with the input seeds of
                   tests/test_oracle_golden.py
  CONFIGS          the models part 2 builds: the two-level SD-1.5 reduction block_out_channels=(C, cin - C) of tests/test_gpu_fullsize.py
  CHAIN_CASES      one geometry each: the LAST up block's resnet -> transformer -> motion module, every block on the oracle's output of the
                   block before it; `run` names the blocks the device test launches
  GN_CASES         ops.group_norm alone, as _norm_proj_in and _norm_act_conv call it
  SAMPLER_CASES    the stride-2 and the upsampling 3x3 convs of _run_down / _run_rest

The `*_form` functions are the questions the library answers on the host (ops.gemm_plan, ops.conv_halo_plan,
emo_groupnorm_one_launch_ok, emo_gemm_suggest_split_k, ops.attention_plan): the device test asserts from the recorded launch tags that
the form asked for here is the form that ran."""
import functools

import torch

from tests import cases

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LOWP = [torch.bfloat16, torch.float16]
KINDS = ("resnet", "transformer", "motion")


def round_up(x, m):
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------- state-dict shapes of single modules (local key names)
def resnet_shapes(cin, cout, temb=128):
    d = {"norm1.weight": (cin,), "norm1.bias": (cin,), "conv1.weight": (cout, cin, 3, 3), "conv1.bias": (cout,),
         "time_emb_proj.weight": (cout, temb), "time_emb_proj.bias": (cout,), "norm2.weight": (cout,),
         "norm2.bias": (cout,), "conv2.weight": (cout, cout, 3, 3), "conv2.bias": (cout,)}
    if cin != cout:
        d.update({"conv_shortcut.weight": (cout, cin, 1, 1), "conv_shortcut.bias": (cout,)})
    return d


def tf_shapes(c, ctx, lin):
    from emote_hack_amd.spec import TransformerSpec, _transformer_shapes
    d = {}
    _transformer_shapes(TransformerSpec("t", c, 4, ctx, lin), d)
    return {k[2:]: v for k, v in d.items()}


def motion_shapes(c, heads, pe=24):
    from emote_hack_amd.spec import MotionSpec, _motion_shapes
    d = {}
    _motion_shapes(MotionSpec("m", c, heads, 2, pe), d)
    return {k[2:]: v for k, v in d.items()}


def sampler_shapes(c):
    return {"conv.weight": (c, c, 3, 3), "conv.bias": (c,)}


# ----------------------------------------------------------------------------- part 1: the reference's per-module goldens
# golden: key(s) of modules.safetensors; cfg: the host model (a name of CONFIGS or of tests/cases.py); slot: the block's state-dict prefix;
# salt: the prefix the golden's weights were synthesised under (emote_hack_amd.synth: name-keyed, salt + local key); x / emb / ctx: (shape, seed)
GOLDEN_BLOCKS = [
    dict(name="resnet_sc", kind="resnet", cfg="TINY", slot="down_blocks.1.resnets.0", salt="resnet_sc.", shapes=resnet_shapes(32, 64),
         x=((2, 32, 4, 8, 8), 11), emb=((2, 128), 12), golden="resnet_sc/out"),
    dict(name="resnet_id", kind="resnet", cfg="TINY", slot="down_blocks.1.resnets.1", salt="resnet_id.", shapes=resnet_shapes(64, 64),
         x=((2, 64, 4, 8, 8), 11), emb=((2, 128), 12), golden="resnet_id/out"),
    dict(name="down", kind="down", cfg="TINY", slot="down_blocks.1.downsamplers.0", salt="down.", shapes=sampler_shapes(64),
         x=((1, 64, 3, 8, 8), 13), golden="down/out"),
    dict(name="up", kind="up", cfg="TINY", slot="up_blocks.0.upsamplers.0", salt="up.", shapes=sampler_shapes(64),
         x=((1, 64, 3, 4, 4), 14), golden="up/out"),
    dict(name="tf3d", kind="transformer", cfg="TINY", slot="down_blocks.1.attentions.0", salt="tf3d.", shapes=tf_shapes(64, 32, False),
         x=((2, 64, 3, 4, 4), 40), ctx=((2, 5, 32), 41), golden="tf3d/out"),
    dict(name="tf3d_perframe", kind="transformer", cfg="TINY", slot="down_blocks.1.attentions.0", salt="tf3d.", shapes=tf_shapes(64, 32, False),
         x=((2, 64, 3, 4, 4), 40), ctx=((6, 5, 32), 42), golden="tf3d/out_perframe_ctx"),
    dict(name="tf3d_lin", kind="transformer", cfg="TINY_LINEAR", slot="down_blocks.1.attentions.0", salt="tf3d_lin.", shapes=tf_shapes(64, 32, True),
         x=((2, 64, 3, 4, 4), 40), ctx=((2, 5, 32), 41), golden="tf3d_lin/out"),
    dict(name="tf3d_lin_perframe", kind="transformer", cfg="TINY_LINEAR", slot="down_blocks.1.attentions.0", salt="tf3d_lin.",
         shapes=tf_shapes(64, 32, True), x=((2, 64, 3, 4, 4), 40), ctx=((6, 5, 32), 42), golden="tf3d_lin/out_perframe_ctx"),
    dict(name="motion", kind="motion", cfg="TINY_MOTION", slot="down_blocks.1.motion_modules.0", salt="motion.", shapes=motion_shapes(64, 4),
         x=((2, 64, 4, 4, 4), 50), golden="motion/out"),
    dict(name="motion320", kind="motion", cfg="320", slot="down_blocks.0.motion_modules.0", salt="motion320.", shapes=motion_shapes(320, 8),
         x=((1, 320, 12, 4, 4), 51), golden="motion320/out"),
]
# goldens of modules.safetensors that no block test reads: the product has no stand-alone entry for a bare CrossAttention, a bare
# FeedForward or the timestep MLP (they exist only inside _transformer / _motion / _begin), and a test that re-composed those calls
# would test its own composition
GOLDEN_LEFT_OUT = ("attn40/", "attn80/", "attn160/", "ff/out", "temb/")


def golden_overrides(name):
    """{state-dict key of the host model: CPU tensor} of one GOLDEN_BLOCKS entry - the golden's name-keyed weights under the block's prefix"""
    from emote_hack_amd.synth import synth_state_dict
    g = next(b for b in GOLDEN_BLOCKS if b["name"] == name)
    return {g["slot"] + "." + k: v for k, v in synth_state_dict(g["shapes"], prefix=g["salt"]).items()}


# ----------------------------------------------------------------------------- part 2: the models
def two_level(C, cin):
    return dict(cases.SD15_MOTION, block_out_channels=(C, cin - C), down_block_types=("CrossAttnDownBlock3D", "DownBlock3D"),
                up_block_types=("UpBlock3D", "CrossAttnUpBlock3D"), layers_per_block=1)


# cpu: the state-dict prefixes the ORACLE reads (name-keyed weights drawn on the host, as the goldens'); every other entry only has to
# exist and is drawn on the device.  up_blocks.1 of a two-level model: resnets.0 (cin -> C), resnets.1 (C + C -> C), attentions, motion_modules
CONFIGS = {
    "320": dict(cfg=two_level(320, 960), cpu=("up_blocks.1.resnets.", "up_blocks.1.attentions.0.", "up_blocks.1.motion_modules.0.",
                                               "down_blocks.0.resnets.0.", "down_blocks.0.downsamplers.0."), golden=("motion320",)),
    "320u": dict(cfg=two_level(320, 640), cpu=("up_blocks.0.upsamplers.0.",), golden=()),      # the only 320-channel upsampler of the family
    "640": dict(cfg=two_level(640, 1280), cpu=("up_blocks.1.resnets.0.", "up_blocks.1.attentions.0.", "down_blocks.0.downsamplers.0."), golden=()),
    "1280": dict(cfg=two_level(1280, 2560), cpu=("up_blocks.1.resnets.0.", "up_blocks.1.attentions.0.", "up_blocks.1.motion_modules.0."), golden=()),
    "tiny": dict(cfg=cases.TINY_MOTION, cpu=("up_blocks.3.resnets.0.",), golden=()),
}


@functools.lru_cache(maxsize=None)
def spec_of(cfg_name):
    from emote_hack_amd.spec import build_spec
    return build_spec(CONFIGS[cfg_name]["cfg"] if cfg_name in CONFIGS else getattr(cases, cfg_name))


@functools.lru_cache(maxsize=None)
def cpu_state(cfg_name):
    """the name-keyed CPU weights of a config's blocks under test (what the oracle reads, and what the device model is overwritten with)"""
    from emote_hack_amd.spec import param_shapes
    from emote_hack_amd.synth import synth_state_dict
    shapes = param_shapes(spec_of(cfg_name))
    sd = synth_state_dict({k: s for k, s in shapes.items() if k.startswith(CONFIGS[cfg_name]["cpu"])})
    for g in CONFIGS[cfg_name]["golden"]:
        sd.update(golden_overrides(g))
    return sd


# ----------------------------------------------------------------------------- part 2: the chains
# cfg, B, F, H, W: the geometry;  res: which resnet of the last up block heads the chain (0: cin -> C, 1: 2C -> C);
# blk: "up" the last up block | "down0" the first down block (its resnet is C -> C: no shortcut, the input itself is the residual);
# run: the blocks the device test launches (the chain's oracle runs up to the last of them);
# ctx: "row" (B, 77, D) | "frame" (B * F, 5, D) | "shared" (1, 77, D) through context_kv() + ctx_kv=;
# bank: None | "banks" (c.banks) | "bank_kv" (c.bank_kv + c.bank_row);  half: shared_half=True on two identical halves;
# scale: _resnet's output scale factor;  strided: the blocks that run a second time on column views with sentinel columns;
# dtypes: f32 everywhere; the 2-byte types wherever the oracle's own sensitivity clears 3 x their gate (tests/test_block_cases_host.py)
def _chain(name, cfg, B, F, H, W, run, **kw):
    c = dict(name=name, cfg=cfg, B=B, F=F, H=H, W=W, run=tuple(run), res=0, blk="up", ctx="row", bank=None, half=False, scale=1.0, strided=(),
             dtypes=tuple(DTYPES), raises=False)
    c.update(kw)
    return c


CHAIN_CASES = [
    # --- transformer: the q | k | v launch forms
    _chain("tf320_4x4", "320", 2, 3, 4, 4, ["transformer"]),                       # HW = 16: two launches
    _chain("tf320_8x8", "320", 1, 2, 8, 8, ["transformer"], strided=("transformer",)),   # merged, 64x64 tile
    _chain("tf640_24x24_f2", "640", 1, 2, 24, 24, ["transformer"]),                # HW = 576, merged ...
    _chain("tf640_24x24_f4", "640", 1, 4, 24, 24, ["transformer"]),                # ... and refused at twice the rows
    _chain("tf1280_24x24", "1280", 1, 2, 24, 24, ["transformer"]),                 # refused; d = 160, 576 keys
    _chain("tf1280_12x12", "1280", 1, 3, 12, 12, ["transformer"]),                 # HW = 144
    _chain("tf1280_32x32", "1280", 1, 4, 32, 32, ["transformer"]),                 # 128x128 tile in f32, the 256x256 phase loop in bf16
    _chain("tf320_5x3", "320", 1, 2, 5, 3, ["transformer"]),                       # 15 tokens: V^T leading dimension 16
    # --- context forms
    _chain("tf320_ctx_frame", "320", 2, 2, 8, 8, ["transformer"], ctx="frame"),
    _chain("tf320_ctx_shared", "320", 2, 2, 8, 8, ["transformer"], ctx="shared"),
    # --- reference-bank read: the first batch row is uncond and skips the bank
    _chain("tf320_banks", "320", 2, 2, 8, 8, ["transformer"], bank="banks"),
    _chain("tf320_bank_kv", "320", 2, 2, 8, 8, ["transformer"], bank="bank_kv"),
    _chain("tf320_half", "320", 2, 2, 8, 8, ["transformer"], half=True),
    # --- resnet: the 3x3 conv and GroupNorm forms
    _chain("res960_16x32", "320", 1, 2, 16, 32, ["resnet"], strided=("resnet",)),  # few tiles, K = 8640: the planner splits K - im2col loader, 1x1 shortcut
    _chain("res960_24x32", "320", 2, 11, 24, 32, ["resnet"], strided=("resnet",)),  # halo, 8-row patches, 128 + 128 + 64, the input the whole [hidden | skip] buffer
    _chain("res1280_24x24", "640", 1, 12, 24, 24, ["resnet"]),                     # halo, ragged patches (overlapped last patch column)
    _chain("res2560_12x12", "1280", 1, 3, 12, 12, ["resnet"]),                     # 12-pixel rows: im2col, the planner's split-K
    _chain("res640_64x64", "320", 1, 5, 64, 64, ["resnet"], res=1),                # halo, 16-row patches, 192-column tail, two-launch GroupNorm
    _chain("res320_64x64", "320", 1, 5, 64, 64, ["resnet"], blk="down0", strided=("resnet",)),   # level 0, identity shortcut: the residual is the input view
    _chain("res640_scale2", "320", 1, 1, 16, 16, ["resnet"], res=1, scale=2.0),
    _chain("res96_tiny_16x16", "tiny", 1, 2, 16, 16, ["resnet"]),                  # conv2 has Cin = 32 on 16-pixel rows: below the 2-byte K-tile, im2col
    # --- motion module (f32: the generic temporal kernel; 2-byte types: the MFMA one)
    _chain("mo320_f1", "320", 2, 1, 4, 4, ["motion"], dtypes=(torch.float32,)),    # one frame has no order to reverse: f32 only
    _chain("mo320_f2", "320", 2, 2, 4, 4, ["motion"]),
    _chain("mo320_f16", "320", 2, 16, 4, 4, ["motion"], strided=("motion",)),
    _chain("mo320_f17", "320", 2, 17, 4, 4, ["motion"]),
    _chain("mo320_f24", "320", 2, 24, 4, 4, ["motion"]),
    _chain("mo320_f25", "320", 2, 25, 4, 4, ["motion"], raises=True),              # past temporal_position_encoding_max_len
    _chain("mo1280_2x2_f24", "1280", 1, 24, 2, 2, ["motion"]),
    _chain("mo320_5x3_f3", "320", 1, 3, 5, 3, ["motion"]),
]
CHAIN = {c["name"]: c for c in CHAIN_CASES}
BANK_ROWS, BANK_ROW = 3, 1      # "bank_kv": the projected banks of a group of 3 timesteps, the device word names row 1


def blocks_of(spec, case):
    blk = spec.up[-1] if case["blk"] == "up" else spec.down[0]
    return blk.resnets[case["res"]], blk.attentions[0], blk.motions[0]


def chain_blocks(case):
    """(ResnetSpec, TransformerSpec, MotionSpec) of a chain: the block's resnet `res` and its first transformer / motion module"""
    return blocks_of(spec_of(case["cfg"]), case)


def chain_seed(case):
    return 1000 + 10 * CHAIN_CASES.index(CHAIN[case["name"]])


def chain_inputs(case, alt=None):
    """The seeded inputs of a chain: x (B, cin, F, H, W), emb (B, 4 C0), ctx in the case's form, bank (rows, H * W, C) or None.
    alt = "ctx" | "emb": the same with ANOTHER context / time embedding (the sensitivity probes)."""
    from emote_hack_amd.synth import seeded_randn
    r, a, _mo = chain_blocks(case)
    s, B, F, H, W = chain_seed(case), case["B"], case["F"], case["H"], case["W"]
    if case["half"]:
        x = seeded_randn((B // 2, r.cin, F, H, W), s).repeat(2, 1, 1, 1, 1)
    else:
        x = seeded_randn((B, r.cin, F, H, W), s)
    emb = seeded_randn((B, r.temb), s + (5 if alt == "emb" else 1))
    if case["half"]:    # the halves share the time embedding as well (unet._begin: halves_identical)
        emb = emb[:B // 2].repeat(2, 1)
    shape = {"row": (B, 77, a.ctx_dim), "frame": (B * F, 5, a.ctx_dim), "shared": (1, 77, a.ctx_dim)}[case["ctx"]]
    ctx = seeded_randn(shape, s + (6 if alt == "ctx" else 2))
    bank = None
    if case["bank"] == "banks":
        bank = seeded_randn((B, H * W, a.channels), s + 3)
    elif case["bank"] == "bank_kv":
        bank = seeded_randn((BANK_ROWS, H * W, a.channels), s + 3)
    return dict(x=x, emb=emb, ctx=ctx, bank=bank)


def oracle_bank(case, bank):
    """the (B, L, C) bank the reference's read hook sees: one row per batch row (the uncond row's is dead)"""
    if case["bank"] == "bank_kv":
        return bank[BANK_ROW:BANK_ROW + 1].repeat(case["B"], 1, 1)
    return bank


def oracle_stage(case, kind, x, inp, *, bank=True, emb=None, ctx=None):
    """one block of a chain on the CPU oracle (oracle/unet_ref.py); bank=False withholds the bank from the read"""
    from oracle import unet_ref as U
    r, a, mo = chain_blocks(case)
    sd, cfg = cpu_state(case["cfg"]), spec_of(case["cfg"]).cfg
    G = cfg["norm_num_groups"]
    with torch.no_grad():
        if kind == "resnet":
            return U.resnet_block(sd, r.prefix, x, inp["emb"] if emb is None else emb, G, cfg["norm_eps"], case["scale"])
        if kind == "transformer":
            c = inp["ctx"] if ctx is None else ctx
            if case["ctx"] == "shared":
                c = c.expand(case["B"], -1, -1)
            kw = {}
            if case["bank"]:
                kw = dict(bank_mode="read", bank=oracle_bank(case, inp["bank"]) if bank else None, uc_rows=cases.uc_rows(case["B"], case["F"]))
            return U.transformer3d(sd, a.prefix, x, c, a.heads, G, **kw)
        return U.motion_module(sd, mo.prefix, x, mo.heads)


def chain_stages(case):
    """the blocks a chain's oracle runs: up to the last block the device test launches"""
    return KINDS[:max(KINDS.index(k) for k in case["run"]) + 1]


@functools.lru_cache(maxsize=None)
def _chain_oracle(name):
    case = CHAIN[name]
    inp = chain_inputs(case)
    out, x = {}, inp["x"]
    for kind in chain_stages(case):
        out[kind + "/in"] = x
        x = out[kind] = oracle_stage(case, kind, x, inp)
    return inp, out


def chain_oracle(case):
    """(inputs, {kind + "/in": the block's input, kind: the oracle's output}) of a chain, computed once and shared: leave it unchanged"""
    return _chain_oracle(case["name"])


# ----------------------------------------------------------------------------- part 2: GroupNorm alone and the samplers
# (instances, rows per instance, channels): ops.group_norm as _norm_proj_in (per frame, eps 1e-6, no activation) and _norm_act_conv
# (joint over a batch row's frames, eps 1e-5, SiLU) call it, against f32 torch.nn.functional.group_norm
GN_CASES = [dict(name="gn_2x64_320", n=2, S=64, C=320), dict(name="gn_1x128_320", n=1, S=128, C=320),
            dict(name="gn_1x512_1280", n=1, S=512, C=1280), dict(name="gn_1x1152_640", n=1, S=1152, C=640)]
GN_GROUPS = 32

# kind "down": 3x3, stride 2 (_run_down);  "up": nearest x2 + 3x3 (_run_rest);  "up_to": nearest to `to` + 3x3 (forward_upsample_size)
SAMPLER_CASES = [
    dict(name="down640_24x24", kind="down", cfg="640", slot="down_blocks.0.downsamplers.0", C=640, B=1, F=2, H=24, W=24, strided=True),
    dict(name="down320_5x3", kind="down", cfg="320", slot="down_blocks.0.downsamplers.0", C=320, B=1, F=2, H=5, W=3),
    dict(name="up320_8x8", kind="up", cfg="320u", slot="up_blocks.0.upsamplers.0", C=320, B=1, F=2, H=8, W=8),            # few tiles: split-K, im2col
    dict(name="up320_8x8_f65", kind="up", cfg="320u", slot="up_blocks.0.upsamplers.0", C=320, B=5, F=13, H=8, W=8, strided=True),   # halo on the doubled frame
    dict(name="up320_12x12", kind="up", cfg="320u", slot="up_blocks.0.upsamplers.0", C=320, B=1, F=29, H=12, W=12),      # halo, 24 x 24: ragged
    dict(name="up320_3x2_to_5x3", kind="up_to", cfg="320u", slot="up_blocks.0.upsamplers.0", C=320, B=1, F=2, H=3, W=2, to=(5, 3)),
]


def sampler_seed(case):
    return 3000 + SAMPLER_CASES.index(case)


@functools.lru_cache(maxsize=None)
def _sampler_oracle(name):
    case = next(s for s in SAMPLER_CASES if s["name"] == name)
    from emote_hack_amd.synth import seeded_randn
    from oracle import unet_ref as U
    sd = cpu_state(case["cfg"])
    x = seeded_randn((case["B"], case["C"], case["F"], case["H"], case["W"]), sampler_seed(case))
    with torch.no_grad():
        if case["kind"] == "down":
            return x, U._conv_per_frame(sd, case["slot"] + ".conv", x, stride=2, padding=1)
        return x, U.upsample(sd, case["slot"], x, (case["F"],) + tuple(case["to"]) if case["kind"] == "up_to" else None)


def sampler_oracle(case):
    """(input, the oracle's output) of a sampler case, computed once and shared: leave it unchanged"""
    return _sampler_oracle(case["name"])


# ----------------------------------------------------------------------------- what the library launches for a case (host side)
def _lib():
    from emote_hack_amd import _lib as L
    return L.load()


def _dt(dtype):
    from emote_hack_amd import ops
    return ops.dt(dtype)


def qkv_form(C, HW, nb, dtype):
    """attn1's q | k | v projection of nb batches of HW tokens as _transformer asks for it (MERGE_QKV): dict(merged, tile, phase) - the
    planned tile / main loop of the merged launch, or merged=False where the library refuses the split store and two launches run"""
    from emote_hack_amd import ops
    from emote_hack_amd._lib import EmoHipError
    try:
        p = ops.gemm_plan(dtype=dtype, M=nb * HW, N=3 * C, K=C, bias=True, ln=True, vt_cols=C, vt_rows=HW, vt_ld=round_up(HW, 8))
    except EmoHipError:
        return dict(merged=False, tile=0, phase=0)
    assert p[3] & 8, p
    return dict(merged=True, tile=p[1], phase=p[2])


def conv_form(dtype, n_img, H, W, Cin, N, *, upsample2x=False, rowbias_rows=0, ld_rowbias=None, residual=False, out_scale=1.0, lda=None, ldc=None,
              ldr=None):
    """a stride-1 3x3 conv as ops.conv3x3 launches it: the planner's split-K first (a split conv runs on the im2col loader), then the
    halo-reuse kernel's verdict.  dict(kind "halo" | "im2col", sk, ph, main, tail, ragged)"""
    from emote_hack_amd import ops
    He, We = (2 * H, 2 * W) if upsample2x else (H, W)
    sk = _lib().emo_gemm_suggest_split_k(n_img * He * We, N, 9 * Cin, _dt(dtype), 0, 0)
    if sk > 1:
        return dict(kind="im2col", sk=sk, ph=0, main=0, tail=0, ragged=False)
    p = ops.conv_halo_plan(dtype=dtype, n_img=n_img, H=H, W=W, Cin=Cin, N=N, upsample2x=upsample2x, lda=lda, ldc=ldc, bias=True,
                           rowbias=bool(rowbias_rows), rows_per_batch=rowbias_rows, ld_rowbias=ld_rowbias, residual=residual, ldr=ldr,
                           out_scale=out_scale)
    if not p[0]:
        return dict(kind="im2col", sk=1, ph=0, main=0, tail=0, ragged=False)
    return dict(kind="halo", sk=1, ph=p[1], main=p[2], tail=p[5], ragged=bool(He % 8 or We % 16))


def gn_one_launch(n_inst, S, C, groups, dtype):
    return bool(_lib().emo_groupnorm_one_launch_ok(n_inst, S, C, groups, _dt(dtype)))


def temb_width(cfg_name):
    sp = spec_of(cfg_name)
    return sum(r.temb_cols for blk in sp.down + [sp.mid] + sp.up for r in blk.resnets)


def resnet_form(case, dtype, lda=None, ldc=None):
    """the launches of _resnet for a chain: conv1 (bias + temb row bias; it reads the GroupNorm's contiguous output), conv2 (bias +
    residual, scaled), the two GroupNorms.  lda / ldc: the leading dimensions of the input and of out= when they are column views - the
    input is conv2's residual where the resnet has no shortcut"""
    r, _a, _mo = chain_blocks(case)
    B, F, H, W = case["B"], case["F"], case["H"], case["W"]
    G = spec_of(case["cfg"]).cfg["norm_num_groups"]
    return dict(conv1=conv_form(dtype, B * F, H, W, r.cin, r.cout, rowbias_rows=F * H * W, ld_rowbias=temb_width(case["cfg"])),
                conv2=conv_form(dtype, B * F, H, W, r.cout, r.cout, residual=True, out_scale=1.0 / case["scale"], ldc=ldc,
                                ldr=None if r.has_shortcut else lda),
                gn1=gn_one_launch(B, F * H * W, r.cin, G, dtype), gn2=gn_one_launch(B, F * H * W, r.cout, G, dtype))


def transformer_form(case, dtype):
    """the launches of _transformer for a chain: the q | k | v form, the per-frame GroupNorm's, and the attention plans of attn1
    (HW keys, + the bank's) and attn2 (the context's keys)"""
    from emote_hack_amd import ops
    _r, a, _mo = chain_blocks(case)
    B, F, HW = case["B"], case["F"], case["H"] * case["W"]
    nb, d = B * F, a.channels // a.heads
    nb1 = nb // 2 if case["half"] else nb
    ctx_len = 5 if case["ctx"] == "frame" else 77
    return dict(qkv=qkv_form(a.channels, HW, nb1, dtype), gn=gn_one_launch(nb1, HW, a.channels, spec_of(case["cfg"]).cfg["norm_num_groups"], dtype),
                d=d, keys=("bank" if case["bank"] else "self", "ctx"),
                attn1=ops.attention_plan(dtype=dtype, B=nb1, Lq=HW, Lk0=HW, heads=a.heads, d=d, Lk1=HW if case["bank"] else 0),
                attn2=ops.attention_plan(dtype=dtype, B=nb, Lq=HW, Lk0=ctx_len, heads=a.heads, d=d))


def sampler_out_hw(case):
    if case["kind"] == "down":
        return (case["H"] - 1) // 2 + 1, (case["W"] - 1) // 2 + 1       # 3x3, stride 2, padding 1
    return tuple(case["to"]) if case["kind"] == "up_to" else (2 * case["H"], 2 * case["W"])


def sampler_form(case, dtype):
    """a sampler conv: x2 asks the halo kernel behind the planner's split-K; stride 2 and an odd upsampling target always take the
    im2col loader (with the planner's split)"""
    n_img, C = case["B"] * case["F"], case["C"]
    if case["kind"] == "up":
        return conv_form(dtype, n_img, case["H"], case["W"], C, C, upsample2x=True)
    Ho, Wo = sampler_out_hw(case)
    return dict(kind="im2col", sk=_lib().emo_gemm_suggest_split_k(n_img * Ho * Wo, C, 9 * C, _dt(dtype), 0, 0), ph=0, main=0, tail=0, ragged=False)


# ----------------------------------------------------------------------------- the project's gate, as numbers (tests.test_gpu_unet.check)
def gate_mean(ref, dtype):
    """the MEAN error `check` lets through for this reference tensor: the f32 bound rtol 1e-3 / atol 1e-4 at the tensor's mean magnitude,
    the low-precision yard-stick otherwise"""
    from tests.test_gpu_unet import yardstick
    if dtype == torch.float32:
        return 1e-4 + 1e-3 * float(ref.abs().mean())
    return 1.25 * yardstick(dtype)[0] * float(ref.abs().mean()) + 1e-5
