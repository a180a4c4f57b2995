"""GPU parity of the BLOCK methods of emote_hack_amd/unet.py - _resnet, _norm_act_conv, _transformer, _norm_proj_in, _motion and the
sampler convs of _run_down / _run_rest: the layer that picks a launch form per op, folds LayerNorm / GroupNorm / the positional
encoding / ff.net.2 + proj_out into weights at load time and wires operands as column views of wider buffers.  Tables:
tests/block_cases.py; what they reach is proved on the host by tests/test_block_cases_host.py.

Part 1 - the reference's own per-module outputs (tests/golden/modules.safetensors) through the HIP blocks: the host model whose spec has
a block of the golden's geometry gets the golden's name-keyed weights under that block's prefix BEFORE .to("cuda", dtype), so
_pack_weights (re-layout, folds, the fused temb_all table) runs on them; then the product's block method is called.
The attn*/..., ff/out and temb/* goldens stay with the CPU oracle (tests/test_oracle_golden.py): the product has no stand-alone entry
for a bare CrossAttention, a bare FeedForward or the timestep MLP, and a test that re-composed _transformer's calls would test itself.

Part 2 - the blocks of the two-level SD-1.5 reduction across the launch forms between the tiny model and the benchmark's geometry,
against the oracle (oracle/unet_ref.py) on the CPU, each block on the oracle's output of the block before it; one case per block kind
runs a second time with its input as the right-hand column view of a wider buffer and out= as the left-hand column view of another
(the zero-copy skip plumbing), whose other columns must keep their bits.  Around each call a KernelProfiler records the launch tags:
the form the host test predicted is the form that ran.

Gate: tests.test_gpu_unet.check - rtol 1e-3 / atol 1e-4 in f32, the reference's own low-precision error scale otherwise."""
import os

import pytest
import torch
from safetensors.torch import load_file

from emote_hack_amd.synth import seeded_randn, synth_state_dict
from tests import block_cases as B
from tests import cases
from tests.test_gpu_unet import check

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64            # sentinel columns beside a column view (a multiple of 16 bytes in every dtype)
SENTINEL = 1000.0   # exact in f32, bf16 and f16
IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


# ----------------------------------------------------------------------------- models, one per (config, dtype)
@pytest.fixture(scope="module")
def models():
    from emote_hack_amd.spec import param_shapes
    from emote_hack_amd.unet import UNet3DConditionModel
    states, built = {}, {}

    def state(cfg_name):
        if cfg_name not in states:
            if cfg_name in B.CONFIGS:   # the blocks under test name-keyed from the host, the rest drawn on the device
                sd = synth_state_dict(param_shapes(B.spec_of(cfg_name)), device=DEV)
                sd.update({k: v.to(DEV) for k, v in B.cpu_state(cfg_name).items()})
            else:                       # a tiny config of tests/cases.py with the goldens' weights in their blocks
                sd = synth_state_dict(param_shapes(B.spec_of(cfg_name)))
                for g in B.GOLDEN_BLOCKS:
                    if g["cfg"] == cfg_name:
                        sd.update(B.golden_overrides(g["name"]))
            states[cfg_name] = sd
        return states[cfg_name]

    def get(cfg_name, dtype):
        if (cfg_name, dtype) not in built:
            m = UNet3DConditionModel(**(B.CONFIGS[cfg_name]["cfg"] if cfg_name in B.CONFIGS else getattr(cases, cfg_name)))
            m.load_state_dict(state(cfg_name))
            built[cfg_name, dtype] = m.to(DEV, dtype)
        return built[cfg_name, dtype]

    yield get
    built.clear()
    states.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def mods():
    return load_file(os.path.join(cases.GOLDEN_DIR, "modules.safetensors"))


def ops():
    from emote_hack_amd import ops as o
    return o


def find(m, prefix):
    for blk in m.spec.down + [m.spec.mid] + m.spec.up:
        for s in list(blk.resnets) + list(blk.attentions) + list(blk.motions):
            if s is not None and s.prefix == prefix:
                return s
    raise KeyError(prefix)


def temb_table(m, emb, dtype):
    """the fused time_emb_proj table as _begin forms it: F.silu(emb) W^T + b for every resnet of the model, f32"""
    o = ops()
    return o.convert(o.gemm(o.silu(o.convert(emb.to(DEV), dtype)), m._w["temb_all.w"], m._w["temb_all.b"]), torch.float32)


class Views:
    """input as the right-hand column view of a wider buffer, out= as the left-hand column view of another; the other columns hold a
    sentinel whose bits must survive the block, and so must the input's"""

    def __init__(self, rows, out_rows, cout):
        self.buf_in = torch.full((rows.shape[0], PAD + rows.shape[1]), SENTINEL, device=DEV, dtype=rows.dtype)
        self.buf_in[:, PAD:] = rows
        self.buf_out = torch.full((out_rows, cout + PAD), SENTINEL, device=DEV, dtype=rows.dtype)
        self.x, self.out = self.buf_in[:, PAD:], self.buf_out[:, :cout]
        self.before = self.buf_in.clone()

    def verify(self, y):
        assert y.data_ptr() == self.out.data_ptr() and y.stride(0) == self.out.stride(0), "the block did not write into out="
        assert torch.equal(self.buf_in.view(torch.uint8), self.before.view(torch.uint8)), "the input buffer changed"
        side = self.buf_out[:, self.out.shape[1]:]
        assert bool((side == SENTINEL).all()), f"{int((side != SENTINEL).sum())} elements beside out= were overwritten"


class Witness:
    """records the launch tags of the calls inside the `with` block (ops.PROFILER), and restores the profiler"""

    def __enter__(self):
        o = ops()
        self.saved, o.PROFILER = o.PROFILER, o.KernelProfiler()
        self.prof = o.PROFILER
        return self

    def __exit__(self, *exc):
        ops().PROFILER = self.saved
        return False

    def tags(self, name):
        return [r[5] for r in self.prof.records if r[0] == name]


def operands(rows, out_rows, cout, strided):
    if not strided:
        return rows, None, None
    v = Views(rows, out_rows, cout)
    return v.x, v.out, v


# ----------------------------------------------------------------------------- the block calls
def run_resnet(m, r, x5, emb, dtype, scale=1.0, strided=False):
    from emote_hack_amd.unet import _Ctx
    o = ops()
    Bn, _c, F, H, W = x5.shape
    rows = o.ncfhw_to_rows(x5.to(DEV), dtype)
    x, out, v = operands(rows, rows.shape[0], r.cout, strided)
    with Witness() as wit:
        y = m._resnet(r, x, temb_table(m, emb, dtype), _Ctx(Bn, F, H, W), H, W, scale, out=out)
    if v is not None:
        v.verify(y)
    return o.rows_to_ncfhw(y, Bn, r.cout, F, H, W), wit


def run_transformer(m, a, x5, ctx, dtype, *, form="row", bank=None, bank_form=None, half=False, strided=False):
    from emote_hack_amd.unet import _Ctx
    o = ops()
    Bn, C, F, H, W = x5.shape
    c = _Ctx(Bn, F, H, W)
    rows = o.ncfhw_to_rows((x5[:Bn // 2] if half else x5).to(DEV), dtype)
    x, out, v = operands(rows, Bn * F * H * W, C, strided)
    ctx_rows, ctx_kv = None, None
    if form == "shared":     # one context row for every batch row: the attn2 projections hoisted out of the step (context_kv + ctx_kv=)
        ctx_kv, ctx_div = m.context_kv(ctx.to(DEV)), Bn * F
    else:
        ctx_rows = o.convert(ctx.to(DEV).float().reshape(-1, ctx.shape[2]), dtype)
        ctx_div = F if ctx.shape[0] == Bn else 1
        assert ctx.shape[0] in (Bn, Bn * F)
    if bank is not None:     # what ReferenceAttentionControl._prepare / the pipeline's reference group set up under CFG
        c.bank_mode, c.active, c.uc_batches = "read", {a.prefix}, (Bn // 2) * F
        bank_rows = o.convert(bank.reshape(-1, C).to(DEV), dtype)
        if bank_form == "banks":
            c.banks, c.bank_rows, c.bank_skip = {a.prefix: bank_rows}, bank.shape[0], 0
        else:
            kb, vbt = m.bank_kv(a.prefix, bank_rows, bank.shape[1])
            c.bank_kv, c.bank_row = {a.prefix: (kb, vbt, bank.shape[1])}, torch.tensor([B.BANK_ROW], dtype=torch.int32, device=DEV)
    with Witness() as wit:
        y = m._transformer(a, x, ctx_rows, ctx.shape[1], ctx_div, c, H, W, out=out, ctx_kv=ctx_kv, shared_half=half)
    if v is not None:
        v.verify(y)
    return o.rows_to_ncfhw(y, Bn, C, F, H, W), wit


def run_motion(m, mo, x5, dtype, strided=False):
    from emote_hack_amd.unet import _Ctx
    o = ops()
    Bn, C, F, H, W = x5.shape
    rows = o.ncfhw_to_rows(x5.to(DEV), dtype)
    x, out, v = operands(rows, rows.shape[0], C, strided)
    with Witness() as wit:
        y = m._motion(mo, x, _Ctx(Bn, F, H, W), H, W, out=out)
    if v is not None:
        v.verify(y)
    return o.rows_to_ncfhw(y, Bn, C, F, H, W), wit


def run_sampler(m, slot, kind, x5, dtype, to=None, strided=False):
    """the sampler convs as _run_down (stride 2) and _run_rest (upsample_to=) call ops.conv3x3 with the model's packed weights"""
    o = ops()
    Bn, C, F, H, W = x5.shape
    rows = o.ncfhw_to_rows(x5.to(DEV), dtype)
    if kind == "down":
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    else:
        Ho, Wo = to if to is not None else (2 * H, 2 * W)
    x, out, v = operands(rows, Bn * F * Ho * Wo, C, strided)
    with Witness() as wit:
        if kind == "down":
            y, h_, w_ = o.conv3x3(x, m._w[slot + ".w"], m._w[slot + ".b"], Bn * F, H, W, stride=2, out=out)
        else:
            y, h_, w_ = o.conv3x3(x, m._w[slot + ".w"], m._w[slot + ".b"], Bn * F, H, W, upsample_to=(Ho, Wo), out=out)
    assert (h_, w_) == (Ho, Wo)
    if v is not None:
        v.verify(y)
    return o.rows_to_ncfhw(y, Bn, C, F, Ho, Wo), wit


# ----------------------------------------------------------------------------- the witnesses: the predicted form is the one that ran
def sk_of(tag):
    return next((int(t[2:]) for t in tag.split() if t.startswith("sk") and t[2:].isdigit()), 1)


def witness_resnet(wit, form):
    convs, gns = wit.tags("gemm_conv3x3"), wit.tags("groupnorm")
    assert len(convs) == 2 and len(gns) == 2, (convs, gns)
    assert [sk_of(t) for t in convs] == [form["conv1"]["sk"], form["conv2"]["sk"]], (convs, form)
    assert [t.endswith(" 1L") for t in gns] == [form["gn1"], form["gn2"]], (gns, form)


def witness_transformer(wit, form, C, HW, bank):
    dense = wit.tags("gemm_dense")
    merged = [t for t in dense if f" vt{C}" in t]
    qk = [t for t in dense if f" N={2 * C} K={C}" in t and t.endswith(" ln")]
    vt = [t for t in dense if f" N={C} K={C} T" in t and t.endswith(" ln")]
    if form["qkv"]["merged"]:
        assert len(merged) == 1 and not qk and not vt, dense
    else:
        assert not merged and len(qk) == 1 and len(vt) == 1, dense
    gns = wit.tags("groupnorm")
    assert len(gns) == 1 and gns[0].endswith(" 1L") == form["gn"], (gns, form)
    att = wit.tags("attention")
    assert len(att) == 2 and f" Lk={HW}+{HW if bank else 0} " in att[0], att


# ----------------------------------------------------------------------------- part 1: the reference's goldens through the HIP blocks
@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("name", [g["name"] for g in B.GOLDEN_BLOCKS])
def test_reference_module_goldens_through_the_hip_blocks(models, mods, name, dtype):
    g = next(b for b in B.GOLDEN_BLOCKS if b["name"] == name)
    m = models(g["cfg"], dtype)
    x = seeded_randn(*g["x"])
    if g["kind"] == "resnet":
        got, _ = run_resnet(m, find(m, g["slot"]), x, seeded_randn(*g["emb"]), dtype)
    elif g["kind"] == "transformer":
        ctx = seeded_randn(*g["ctx"])
        got, _ = run_transformer(m, find(m, g["slot"]), x, ctx, dtype)
    elif g["kind"] == "motion":
        got, _ = run_motion(m, find(m, g["slot"]), x, dtype)
    else:
        got, _ = run_sampler(m, g["slot"], g["kind"], x, dtype)
    ref = mods[g["golden"]]
    assert got.shape == ref.shape
    check(got, ref, dtype)


# ----------------------------------------------------------------------------- part 2: the chains
def _chain_params(kind):
    return [pytest.param(c["name"], d, id=f"{c['name']}-{IDS[d]}") for c in B.CHAIN_CASES if kind in c["run"] and not c["raises"]
            for d in c["dtypes"]]


def _blocks(m, case):
    return B.blocks_of(m.spec, case)


@pytest.mark.parametrize("name,dtype", _chain_params("resnet"))
def test_resnet_across_conv_and_groupnorm_forms_vs_oracle(models, name, dtype):
    case = B.CHAIN[name]
    inp, ora = B.chain_oracle(case)
    m = models(case["cfg"], dtype)
    r = _blocks(m, case)[0]
    assert (r.prefix, r.cin) == (B.chain_blocks(case)[0].prefix, inp["x"].shape[1])
    for strided in (False, True) if "resnet" in case["strided"] else (False,):
        got, wit = run_resnet(m, r, ora["resnet/in"], inp["emb"], dtype, case["scale"], strided)
        check(got, ora["resnet"], dtype)
        # (conv1 reads the GroupNorm's contiguous output; conv2 writes the view, and without a shortcut its residual is the input view)
        witness_resnet(wit, B.resnet_form(case, dtype, lda=r.cin + PAD if strided else None, ldc=r.cout + PAD if strided else None))


@pytest.mark.parametrize("name,dtype", _chain_params("transformer"))
def test_transformer_across_qkv_context_and_bank_forms_vs_oracle(models, name, dtype):
    case = B.CHAIN[name]
    inp, ora = B.chain_oracle(case)
    m = models(case["cfg"], dtype)
    a = _blocks(m, case)[1]
    for strided in (False, True) if "transformer" in case["strided"] else (False,):
        got, wit = run_transformer(m, a, ora["transformer/in"], inp["ctx"], dtype, form=case["ctx"], bank=inp["bank"], bank_form=case["bank"],
                                   half=case["half"], strided=strided)
        check(got, ora["transformer"], dtype)
        witness_transformer(wit, B.transformer_form(case, dtype), a.channels, case["H"] * case["W"], case["bank"])


@pytest.mark.parametrize("name,dtype", _chain_params("motion"))
def test_motion_module_across_frame_counts_vs_oracle(models, name, dtype):
    case = B.CHAIN[name]
    _inp, ora = B.chain_oracle(case)
    m = models(case["cfg"], dtype)
    mo = _blocks(m, case)[2]
    for strided in (False, True) if "motion" in case["strided"] else (False,):
        got, wit = run_motion(m, mo, ora["motion/in"], dtype, strided)
        check(got, ora["motion"], dtype)
        assert len(wit.tags("temporal_attention")) == mo.n_attn and all(f" F={case['F']} " in t for t in wit.tags("temporal_attention"))


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS.get)
def test_motion_module_refuses_more_frames_than_positions(models, dtype):
    from emote_hack_amd.unet import _Ctx
    case = B.CHAIN["mo320_f25"]
    m = models(case["cfg"], dtype)
    mo = _blocks(m, case)[2]
    rows = torch.zeros(case["B"] * case["F"] * case["H"] * case["W"], mo.channels, device=DEV, dtype=dtype)
    with pytest.raises(ValueError, match="temporal_position_encoding_max_len"):
        m._motion(mo, rows, _Ctx(case["B"], case["F"], case["H"], case["W"]), case["H"], case["W"])


# ----------------------------------------------------------------------------- part 2: GroupNorm alone, the samplers
@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("name", [g["name"] for g in B.GN_CASES])
def test_groupnorm_one_and_two_launch_forms_vs_torch(name, dtype):
    """ops.group_norm as _norm_proj_in (eps 1e-6, no activation) and _norm_act_conv (eps 1e-5, SiLU, in place or not) call it, against
    f32 torch.nn.functional.group_norm; contiguous and on column views"""
    g = next(c for c in B.GN_CASES if c["name"] == name)
    o = ops()
    n, S, C = g["n"], g["S"], g["C"]
    seed = 2000 + B.GN_CASES.index(g)
    x = seeded_randn((n, C, S), seed) * 1.5 + 0.3
    gamma, beta = 1.0 + 0.1 * seeded_randn((C,), seed + 1), 0.1 * seeded_randn((C,), seed + 2)
    rows = o.convert(x.permute(0, 2, 1).reshape(n * S, C).contiguous().to(DEV), dtype)
    one = B.gn_one_launch(n, S, C, B.GN_GROUPS, dtype)
    for eps, silu in ((1e-6, False), (1e-5, True)):
        ref = torch.nn.functional.group_norm(x, B.GN_GROUPS, gamma, beta, eps)
        ref = (torch.nn.functional.silu(ref) if silu else ref).permute(0, 2, 1).reshape(n * S, C)
        for strided in (False, True):
            xin, out, v = operands(rows, n * S, C, strided)
            with Witness() as wit:
                y = o.group_norm(xin, gamma.to(DEV), beta.to(DEV), n, B.GN_GROUPS, eps, silu, out=out)
            if v is not None:
                v.verify(y)
            check(y, ref, dtype)
            assert [t.endswith(" 1L") for t in wit.tags("groupnorm")] == [one]


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS.get)
@pytest.mark.parametrize("name", [s["name"] for s in B.SAMPLER_CASES])
def test_sampler_convs_vs_oracle(models, name, dtype):
    case = next(s for s in B.SAMPLER_CASES if s["name"] == name)
    x, ref = B.sampler_oracle(case)
    m = models(case["cfg"], dtype)
    form = B.sampler_form(case, dtype)
    for strided in (False, True) if case.get("strided") else (False,):
        got, wit = run_sampler(m, case["slot"], case["kind"], x, dtype, to=case.get("to"), strided=strided)
        assert got.shape == ref.shape
        check(got, ref, dtype)
        assert [sk_of(t) for t in wit.tags("gemm_conv3x3")] == [form["sk"]], (wit.tags("gemm_conv3x3"), form)
