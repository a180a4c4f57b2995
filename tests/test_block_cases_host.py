"""The block tables of tests/block_cases.py, checked without a device (style: test_host_logic.test_gemm_sweeps_reach_every_instantiation):

  * the library is asked on the host what every case of tests/test_gpu_blocks.py launches (ops.gemm_plan with the vt_* arguments,
    ops.conv_halo_plan behind the planner's split-K, emo_groupnorm_one_launch_ok, ops.attention_plan): the tables as a WHOLE must reach
    every launch form the block methods of emote_hack_amd/unet.py choose between - no verdict is written down per shape, so a planner
    change that moves a case to another kernel shows here as a form that is no longer reached;
  * the oracle alone must react to what each case pins by at least 3 x the gate the device test applies (a residual block passes a loose
    gate with a dead branch): another context for attn2, the frames reversed for the motion module, another emb for the resnet, the bank
    withheld from the read."""
import pytest
import torch

from tests import block_cases as B


def _chains(kind):
    return [c for c in B.CHAIN_CASES if kind in c["run"] and not c["raises"]]


def test_golden_table_covers_every_block_golden_of_the_reference():
    import os
    from safetensors.torch import load_file
    from tests import cases
    mods = load_file(os.path.join(cases.GOLDEN_DIR, "modules.safetensors"))
    used = {g["golden"] for g in B.GOLDEN_BLOCKS}
    rest = {k for k in mods if k not in used}
    assert used <= set(mods) and all(k.startswith(B.GOLDEN_LEFT_OUT) for k in rest), sorted(rest)
    for g in B.GOLDEN_BLOCKS:      # the block of the host model has the golden's geometry: same keys, same shapes
        from emote_hack_amd.spec import param_shapes
        shapes = param_shapes(B.spec_of(g["cfg"]))
        for k, s in g["shapes"].items():
            assert tuple(shapes[g["slot"] + "." + k]) == tuple(s), (g["name"], k)
        assert tuple(mods[g["golden"]].shape)[:1] == g["x"][0][:1]


def test_transformer_cases_reach_every_qkv_and_attention_form():
    merged_tiles, refused, verdicts, classes = set(), set(), {}, {}
    for c in _chains("transformer"):
        _r, a, _mo = B.chain_blocks(c)
        HW = c["H"] * c["W"]
        for dtype in c["dtypes"]:
            f = B.transformer_form(c, dtype)
            q = f["qkv"]
            if q["merged"]:
                merged_tiles.add(q["tile"])
                assert q["phase"] == int(q["tile"] == 7)
            else:
                refused.add((a.channels, HW))
            verdicts.setdefault((a.channels, HW, dtype), set()).add(q["merged"])
            for key, plan in zip(f["keys"], (f["attn1"], f["attn2"])):
                classes.setdefault((f["d"], key), set()).add((dtype == torch.float32, plan[0]))
    assert merged_tiles >= {1, 2, 7}, merged_tiles                       # 64x64, 128x128, the 256x256 phase loop
    assert any(HW % 64 for _, HW in refused), refused                    # no 64-row tile inside a frame: HW = 15, 16, 144
    assert any(HW == 576 for _, HW in refused), refused
    assert any(v == {True, False} for v in verdicts.values()), "no (width, HW, dtype) is served at one M and refused at another"
    # every head-dim class with the context's keys, the frame's own keys and the frame's + the bank's
    assert set(classes) >= {(40, "ctx"), (40, "self"), (40, "bank"), (80, "ctx"), (80, "self"), (160, "ctx"), (160, "self")}, sorted(classes)
    for two_byte in (False, True):       # d = 40 / 80 / 160 are three different loaders in either element size
        assert len({next(cl for f32, cl in classes[(d, "self")] if f32 != two_byte) for d in (40, 80, 160)}) == 3


def test_resnet_and_sampler_cases_reach_every_conv_and_groupnorm_form():
    convs, gn = set(), set()
    for c in _chains("resnet"):
        r, _a, _mo = B.chain_blocks(c)
        for dtype in c["dtypes"]:
            f = B.resnet_form(c, dtype)
            for name, cin in (("conv1", r.cin), ("conv2", r.cout)):
                v = f[name]
                two = dtype != torch.float32
                if v["kind"] == "halo":
                    convs.add(("halo", v["ph"], v["tail"]))
                    if v["ragged"]:
                        convs.add("ragged")
                elif c["W"] < 16 or c["H"] < 8:
                    convs.add("unserved_width")                            # narrower than a patch, whatever the planner splits
                    if v["sk"] > 1:
                        convs.add("split_k")
                elif v["sk"] > 1:
                    convs.add("split_k")                                   # few tiles and a long K: the planner splits, the im2col loader runs
                elif two and cin % 64:
                    convs.add("unserved_cin_2byte")
                else:
                    raise AssertionError(("a conv off the halo kernel for no reason the table knows", c["name"], name, dtype, v))
            gn |= {f["gn1"], f["gn2"]}
    assert ("halo", 8, 64) in convs and ("halo", 16, 192) in convs, convs   # 128 + 128 + 64 | 128 + 192 at N = 320
    assert {"ragged", "split_k", "unserved_width", "unserved_cin_2byte"} <= convs, convs
    assert gn == {True, False}
    up = {}
    for s in [s for s in B.SAMPLER_CASES if s["kind"] == "up"]:
        for dtype in B.DTYPES:
            up.setdefault(B.sampler_form(s, dtype)["kind"], []).append((s["name"], s["H"], B.sampler_form(s, dtype)["ragged"]))
    g = next(g for g in B.GOLDEN_BLOCKS if g["kind"] == "up")
    (b, c_, f_, h, w), _seed = g["x"]
    assert all(B.conv_form(d, b * f_, h, w, c_, c_, upsample2x=True)["kind"] == "im2col" for d in B.DTYPES)    # 4x4: not served
    assert set(up) == {"halo", "im2col"}, up                                # x2 served and not
    assert {r for _n, _h, r in up["halo"]} == {False, True}                 # 16 x 16 whole, 24 x 24 ragged
    kinds = {s["kind"] for s in B.SAMPLER_CASES}
    assert kinds == {"down", "up", "up_to"}


def test_groupnorm_cases_reach_both_verdicts_in_both_element_sizes():
    v = {(g["name"], dtype): B.gn_one_launch(g["n"], g["S"], g["C"], B.GN_GROUPS, dtype) for g in B.GN_CASES for dtype in B.DTYPES}
    for dtype in B.DTYPES:
        assert {v[g["name"], dtype] for g in B.GN_CASES} == {True, False}, dtype
    # ... and the verdict depends on the element size for some shape, and on (instances, rows) at one width
    assert any(v[g["name"], torch.float32] != v[g["name"], torch.bfloat16] for g in B.GN_CASES)
    by_c = {}
    for g in B.GN_CASES:
        by_c.setdefault(g["C"], set()).add(v[g["name"], torch.float32])
    assert {True, False} in by_c.values()
    # the per-frame GroupNorm of the transformer cases takes both forms as well
    assert {B.transformer_form(c, d)["gn"] for c in _chains("transformer") for d in c["dtypes"]} == {True, False}


def test_tables_hold_every_context_bank_and_frame_count_form():
    names = {c["name"] for c in B.CHAIN_CASES}
    assert len(names) == len(B.CHAIN_CASES)
    assert {c["ctx"] for c in _chains("transformer")} == {"row", "frame", "shared"}
    assert {c["bank"] for c in _chains("transformer")} == {None, "banks", "bank_kv"}
    assert any(c["half"] for c in _chains("transformer")) and any(c["scale"] != 1.0 for c in _chains("resnet"))
    assert {c["F"] for c in _chains("motion") if c["cfg"] == "320" and c["H"] == 4} == {1, 2, 16, 17, 24}
    mo = B.chain_blocks(B.CHAIN["mo320_f25"])[2]
    assert B.CHAIN["mo320_f25"]["raises"] and B.CHAIN["mo320_f25"]["F"] == mo.pe_len + 1
    for kind in B.KINDS:       # every block kind runs once on column views, and in every dtype somewhere
        assert any(kind in c["strided"] for c in B.CHAIN_CASES), kind
        assert {d for c in _chains(kind) for d in c["dtypes"]} == set(B.DTYPES)
    assert all(torch.float32 in c["dtypes"] for c in B.CHAIN_CASES)
    for c in B.CHAIN_CASES:
        assert set(c["strided"]) <= set(c["run"])


def _moved(a, b):
    return float((a - b).abs().mean())


@pytest.mark.parametrize("name", [c["name"] for c in B.CHAIN_CASES if not c["raises"]])
def test_oracle_sensitivity_clears_three_times_the_gate(name):
    """What the case pins is live in the ORACLE: perturbing it moves the oracle's output by at least 3 x the mean error the device test's
    gate lets through in every dtype the case runs in (tests.test_gpu_unet.check: rtol 1e-3 / atol 1e-4 in f32, the low-precision
    yard-stick otherwise).  A case that falls short of a 2-byte gate keeps f32 only - that is decided in the table, not here."""
    case = B.CHAIN[name]
    inp, out = B.chain_oracle(case)
    for kind in case["run"]:
        x, ref = out[kind + "/in"], out[kind]
        if kind == "resnet":
            moved = _moved(B.oracle_stage(case, kind, x, inp, emb=B.chain_inputs(case, alt="emb")["emb"]), ref)
        elif kind == "transformer":
            moved = _moved(B.oracle_stage(case, kind, x, inp, ctx=B.chain_inputs(case, alt="ctx")["ctx"]), ref)
            if case["bank"]:
                gone = _moved(B.oracle_stage(case, kind, x, inp, bank=False), ref)
                # (the uncond batch row never reads the bank: only the other half can move)
                uc = case["B"] // 2
                assert float((B.oracle_stage(case, kind, x, inp, bank=False)[:uc] - ref[:uc]).abs().max()) < 1e-5
                moved = min(moved, gone)
        else:
            if case["F"] == 1:     # one frame has no order: nothing to reverse, and the table keeps the case to f32
                assert case["dtypes"] == (torch.float32,)
                continue
            moved = _moved(B.oracle_stage(case, kind, x.flip(2), inp).flip(2), ref)
        for dtype in case["dtypes"]:
            gate = B.gate_mean(ref, dtype)
            print(f"{name} {kind} {dtype}: the oracle moves by {moved:.4f}, gate {gate:.5f}")
            assert moved >= 3.0 * gate, (name, kind, dtype, moved, gate)
