"""N>1 path on CPU: multi-process `gloo` runs of the product pipeline's sharded sampling loop
(emote_hack_amd/denoise_loop.py: (window x CFG-branch) units dealt `U[rank::world_size]`, a group's ReferenceNet timesteps dealt
over ranks + all_gather of the packed banks, ONE all_gather of the eps slices per step, redundant deterministic
accumulate + sampler step).

There is no GPU here, so the HIP launches are replaced IN THIS TEST by the CPU oracle (test infrastructure):
the UNet / ReferenceNet are oracle-backed stubs and the sampler ops are monkeypatched.  What is under
test is the distributed host logic: every rank must end with latents identical to every other rank's and equal to the
single-process oracle loop - for 2 ranks on one window (uncond || cond), 2 ranks on two windows, 3 ranks on 4 units
(uneven), and 8 ranks on 4 windows (BASELINE configs[3]: every rank exactly one unit) and on 2 windows (surplus ranks idle)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from tests import cases


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class OracleBackedUNet:
    """Stand-in with the product UNet's surface; arithmetic by oracle/unet_ref.py (CPU)."""

    def __init__(self, cfg, sd, has_out=True):
        from emote_hack_amd.config import normalize_unet_config
        from emote_hack_amd.spec import build_spec, reference_block_order
        self.cfg, self.sd = cfg, sd
        self.config = normalize_unet_config(dict(cfg), strict=False)
        self.spec = build_spec(cfg, has_out=has_out)
        self.in_channels, self.dtype, self.device = 4, torch.float32, torch.device("cpu")
        self._reference_control = None
        self._order = lambda fusion: reference_block_order(self.spec, fusion)

    def bank_order(self, fusion="midup"):
        return self._order(fusion)

    # the sampler hoists these projections out of the step; the stub keeps the un-projected inputs
    def context_kv(self, ctx):
        return {"ctx": ctx}

    def bank_kv(self, prefix, rows, L):
        return rows, rows.new_zeros(rows.shape[0] // L, 1, 1)

    def __call__(self, sample, timestep, encoder_hidden_states, return_dict=False, _return_rows=False, audio_features=None,
                 speed_embeddings=None, _ctx_kv=None, _halves_identical=False):
        from oracle import unet_ref as U
        rc = self._reference_control
        if sample.dim() == 4:
            sample = sample.unsqueeze(2)
        B, _, F, H, W = sample.shape
        sd = self.sd if self.spec.has_out else {k: v for k, v in self.sd.items() if not k.startswith(("conv_out", "conv_norm_out"))}
        ctx = encoder_hidden_states
        if ctx.shape[0] == 1 and B > 1:
            ctx = ctx.expand(B, -1, -1)
        if rc is not None and rc.mode == "write":
            _, written = U.unet_forward(sd, self.cfg, sample, timestep, ctx, bank_mode="write", fusion_blocks=rc.fusion_blocks)
            for p in rc.order:
                rc.bank[p].append(written[p])
            return (None,)
        kw = {}
        if rc is not None and rc.mode == "read":
            assert rc.kv_cache is not None, "the sampler hands the banks over as projected caches"
            row, n_uc = int(rc.kv_row.item()), rc.uc_units
            banks = {}
            for p in rc.order:
                k_all, _, L = rc.kv_cache[p]
                bank = k_all[row * L:(row + 1) * L].unsqueeze(0)
                # one bank row per unit; uncond units get a zero row - the oracle overwrites the uc rows like the reference
                banks[p] = torch.cat([torch.zeros_like(bank)] * n_uc + [bank] * (B - n_uc))
            uc_rows = torch.zeros(B * F, dtype=torch.bool)
            uc_rows[:n_uc * F] = True
            kw = dict(bank_mode="read", banks=banks, uc_rows=uc_rows, fusion_blocks=rc.fusion_blocks)
        y = U.unet_forward(sd, self.cfg, sample, timestep, ctx, speed_embeddings=speed_embeddings, **kw)
        if _return_rows:
            return y.permute(0, 2, 3, 4, 1).reshape(-1, y.shape[1]).contiguous()
        return (y,)


def _patch_ops():
    """CPU stand-ins for the three HIP sampler ops + convert (oracle semantics)."""
    from emote_hack_amd import ops
    from oracle.scheduler_ref import counter_normal

    def convert(src, dtype, fp16_round=False):
        return (src.half().float() if fp16_round else src).to(dtype)

    def accumulate_window(pred_rows, npb, counter, frames, *, C_, F, HW, add_counter):
        nf = frames.numel()
        npb.view(C_, F, HW)[:, frames.long()] += pred_rows.reshape(nf, HW, C_).permute(2, 0, 1)
        if add_counter:
            counter[frames.long()] += 1

    def sched_step(noise_pred, counter, latents, history, lat_in, *, C_, F, HW, guidance_scale, a, b, c_x, c, slot, c_noise, s_next,
                   seed, step, eps_out=None):   # include/emo_hip.h emo_sched_step
        avg = noise_pred.view(-1, C_, F, HW) / counter.view(1, 1, F, 1)
        eps = (avg[0] + guidance_scale * (avg[1] - avg[0]) if guidance_scale > 1.0 else avg[0]).reshape(-1)
        x = latents.view(-1)
        d = a * x + b * eps
        out = c_x * x + c[0] * d
        for k in range(1, 4):      # the ring is read before d_n is written into it
            if slot[k] >= 0:
                out = out + c[k] * history[slot[k]]
        if slot[0] >= 0:
            history[slot[0]] = d
        if c_noise != 0.0:
            out = out + c_noise * counter_normal(seed, step, x.numel())
        x.copy_(out)
        if lat_in is not None:
            lat_in.view(-1).copy_(s_next * out)
        if eps_out is not None:
            eps_out.copy_(eps)

    def sched_scale(latents, lat_in, *, C_, F, HW, s):
        lat_in.copy_(s * latents)

    ops.convert, ops.accumulate_window, ops.sched_step, ops.sched_scale = convert, accumulate_window, sched_step, sched_scale


def _models():
    from emote_hack_amd.spec import build_spec, param_shapes
    from emote_hack_amd.synth import synth_state_dict
    unet_sd = synth_state_dict(param_shapes(build_spec(cases.TINY_MOTION)))
    ref_sd = synth_state_dict(param_shapes(build_spec(cases.TINY)), prefix=cases.REF_PREFIX)
    return unet_sd, ref_sd


def _inputs(f_tot=8):
    from emote_hack_amd.synth import seeded_randn
    return seeded_randn((1, 4, f_tot, 16, 16), 5), seeded_randn((1, 4, 16, 16), 3), seeded_randn((2, 5, 32), 2)


def _worker(rank, world, port, kind, out_dir, f_tot, ref_group, cbs=1, gs=7.5, overlap=0):
    import torch.distributed as td
    torch.set_num_threads(1 if world > 4 else 2)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    _patch_ops()
    from emote_hack_amd import DDIMScheduler, DDPMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    unet_sd, ref_sd = _models()
    unet = OracleBackedUNet(cases.TINY_MOTION, unet_sd)
    ref = OracleBackedUNet(cases.TINY, ref_sd, has_out=False)
    pipe = EMOAnimationPipeline(unet=unet, scheduler=DDIMScheduler() if kind == "ddim" else DDPMScheduler())
    lat, refl, text = _inputs(f_tot)
    out = pipe.denoise(lat, refl, text, appearance_encoder=ref, num_inference_steps=3, guidance_scale=gs, context_frames=4,
                       context_stride=1, context_overlap=overlap, seed=0, dist=True, rank=rank, world_size=world,
                       reference_group=ref_group, context_batch_size=cbs)
    torch.save(out.clone(), os.path.join(out_dir, f"lat_{kind}_{rank}.pt"))
    td.barrier()
    td.destroy_process_group()


# (world, frames, reference_group): 8 frames = 2 windows of 4 = 4 units; 4 frames = 1 window = 2 units (uc || c);
# 16 frames = 4 windows = 8 units (BASELINE configs[3] shape: one unit per rank at world 8)
@pytest.mark.parametrize("kind,world,f_tot,ref_group", [("ddim", 2, 8, 10), ("ddpm", 2, 8, 2), ("ddpm", 2, 4, 10), ("ddim", 3, 8, 2),
                                                        ("ddpm", 8, 16, 10), ("ddim", 8, 8, 2)])
def test_multi_rank_gloo_loop_matches_single_process_oracle(tmp_path, kind, world, f_tot, ref_group):
    from oracle.pipeline_ref import denoise_loop
    from oracle.scheduler_ref import SchedulerRef
    mp.spawn(_worker, args=(world, _free_port(), kind, str(tmp_path), f_tot, ref_group), nprocs=world, join=True)
    lats = [torch.load(os.path.join(tmp_path, f"lat_{kind}_{r}.pt")) for r in range(world)]
    for r in range(1, world):
        assert torch.equal(lats[0], lats[r]), f"rank {r}: ranks must hold identical latents without a broadcast"
    unet_sd, ref_sd = _models()
    lat, refl, text = _inputs(f_tot)
    ref = denoise_loop(unet_sd, cases.TINY_MOTION, ref_sd, cases.TINY, lat, refl, text, scheduler=SchedulerRef(kind),
                       num_inference_steps=3, guidance_scale=7.5, context_frames=4, context_stride=1, context_overlap=0, seed=0)
    # (the pipeline's write pass runs on the cond image only and batches timesteps, its UNet calls batch units differently
    # from the oracle's [uc, c] pairs: same maths, different f32 summation order inside the CPU GEMMs; the stochastic DDPM
    # sampler amplifies that to a few 1e-4 on isolated elements)
    torch.testing.assert_close(lats[0], ref, rtol=2e-3, atol=5e-4)


@pytest.mark.parametrize("world,cbs,gs,overlap", [(1, 2, 7.5, 2), (2, 2, 7.5, 2), (3, 2, 7.5, 0), (1, 1, 1.0, 2), (2, 1, 1.0, 2), (2, 2, 1.0, 0)])
def test_context_batch_size_and_no_cfg_match_the_oracle(tmp_path, world, cbs, gs, overlap):
    """context_batch_size 2 (three windows at overlap 2: a full batch of two + a partial one) reproduces the reference's literal
    text / bank pairing at cbs > 1 (row r = branch * n + j runs under text row r % 2 and reads the bank written under it), which
    needs a SECOND ReferenceNet variant (uncond text) and per-variant UNet calls; guidance_scale 1.0 drops the uncond branch
    altogether.  Single rank and sharded, every rank identical, equal to the oracle loop (itself pinned by the `ddim_cbs2` /
    `ddim_nocfg` goldens of tests/golden/loop_tiny.safetensors)."""
    from oracle.pipeline_ref import denoise_loop
    from oracle.scheduler_ref import SchedulerRef
    mp.spawn(_worker, args=(world, _free_port(), "ddim", str(tmp_path), 8, 10, cbs, gs, overlap), nprocs=world, join=True)
    lats = [torch.load(os.path.join(tmp_path, f"lat_ddim_{r}.pt")) for r in range(world)]
    for r in range(1, world):
        assert torch.equal(lats[0], lats[r])
    unet_sd, ref_sd = _models()
    lat, refl, text = _inputs(8)
    ref = denoise_loop(unet_sd, cases.TINY_MOTION, ref_sd, cases.TINY, lat, refl, text, scheduler=SchedulerRef("ddim"),
                       num_inference_steps=3, guidance_scale=gs, context_frames=4, context_stride=1, context_overlap=overlap, seed=0,
                       context_batch_size=cbs)
    torch.testing.assert_close(lats[0], ref, rtol=2e-3, atol=5e-4)


def test_unit_dealing_covers_every_window_branch_once():
    """U[rank::world]: every (window, branch) unit belongs to exactly one rank; with 4 windows on 8 ranks every
    rank owns exactly one unit; slots address the gathered buffer consistently."""
    for n_win, world in ((4, 8), (1, 2), (2, 3), (4, 2), (2, 8), (5, 4)):
        units = [(w, br) for br in (0, 1) for w in range(n_win)]
        seen = []
        n_slots = -(-len(units) // world)
        for r in range(world):
            mine = units[r::world]
            assert len(mine) <= n_slots
            seen += mine
            for slot, u in enumerate(mine):
                i = units.index(u)
                assert (i % world, i // world) == (r, slot)
        assert sorted(seen) == sorted(units)
        if (n_win, world) == (4, 8):
            assert all(len(units[r::world]) == 1 for r in range(world))


def test_window_dealing_covers_every_frame_once():
    """With overlap 0 every frame belongs to exactly one window; with overlap the per-frame counters are >= 1."""
    from emote_hack_amd.context import uniform
    for f_tot, ctx, ov in ((48, 12, 0), (96, 12, 0), (48, 16, 4), (24, 16, 4)):
        windows = list(uniform(0, 50, f_tot, ctx, 1, ov))
        total = torch.zeros(f_tot)
        for w in windows:
            total[w] += 1
        assert bool((total >= 1).all())
        if ov == 0:
            assert bool((total == 1).all())
