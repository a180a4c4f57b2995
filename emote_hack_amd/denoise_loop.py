"""The sampling loop of EMOAnimationPipeline (the reference's hot loop, EMOAnimationPipeline.py:698-823), re-designed for MI355X (DESIGN.md
sections 1 and 5): per step the Backbone read passes over this rank's (context window x CFG branch) units, ONE all_gather of the eps slices
(it replaces gather-to-root + broadcast, :796-821) and window average + CFG + scheduler step fused in one kernel on f32 master latents, run
redundantly on every rank; the ReferenceNet write pass hoisted out of the step - T timesteps per batched pass, projected once with the
Backbone's attn1 weights, two groups resident, the next group on a second stream; the attn2 K / V^T of the context once per clip.

`loop_plan` decides WHO computes WHAT, on the host, from plain numbers; CLIP_INPUTS is the one table of what a prepared state can be re-armed
with; LoopState / LoopCall are the declared state; DenoiseLoop is the base class EMOAnimationPipeline inherits the loop from."""
from __future__ import annotations

import copy
from collections import namedtuple
from types import SimpleNamespace

import torch

from . import ops
from .context import get_context_scheduler
from .reference_control import ReferenceAttentionControl


# One input a prepared state can be re-armed with.  key: how it enters the plan key - by "shape", "presence", "value", "cfg" (the guidance on /
# off bit) or None, not at all; default: what a "value" / "cfg" key takes for an omitted input; hit: what an omitted input MEANS on a plan-cache
# hit in `denoise` (None: not re-bound); buffer: the state field that holds it - a state without it refuses the input as "prepared without
# {without}", and the inputs keyed by shape are copied into it with the shape check.
ClipInput = namedtuple("ClipInput", "name key default hit buffer without", defaults=(None,) * 5)

CLIP_INPUTS = (
    ClipInput("latents", "shape", buffer="latents"),
    ClipInput("ref_image_latents", "shape"),
    ClipInput("text_embeddings", "shape"),
    ClipInput("audio_features", "shape", buffer="audio_features", without="audio_features"),
    ClipInput("speed_embeddings", "shape", buffer="speed", without="speed_embeddings"),       # per clip or per frame
    ClipInput("motion_latents", "shape"),
    ClipInput("controlnet_cond", "shape", buffer="cn_cond", without="a ControlNet"),
    ClipInput("controlnet_conditioning_scale", "value", default=1.0),                          # baked into the captured ControlNet pass
    ClipInput("guidance_scale", "cfg", default=7.5, hit=7.5),
    ClipInput("eta", hit=0.0),
    ClipInput("seed", hit=0),
    ClipInput("face_mask", "presence", buffer="face_rows", without="face_mask"),   # (either size ends in the same (h*w, C0) rows)
    ClipInput("face_mask_threshold"),
)
CLIP_INPUT_NAMES = tuple(r.name for r in CLIP_INPUTS)


class LoopCall:
    """One UNet call of a rank.  From loop_plan: its units [(window, branch)] - uncond units first, n_uc of them -, their slots in the
    exchange buffer, the bank variant its cond units read (None: no cond unit), whether the two halves list the same windows, its frames;
    from prepare_denoise the index tensors; from `_bind_inputs` the context, its K / V^T and the speed rows, rewritten in place per clip."""
    __slots__ = ("units", "slots", "bank_tv", "n_uc", "halves_identical", "frames", "idx", "cn_sel", "ctx", "ctx_kv", "speed")

    def __init__(self, units, slots, bank_tv):
        self.units, self.slots, self.bank_tv, self.n_uc = units, slots, bank_tv, sum(1 for u in units if u[1] == 0)
        self.idx = self.cn_sel = self.ctx = self.speed = None
        self.ctx_kv = {}


class LoopState:
    """A prepared loop.  PLAN: loop_plan's fields, then what prepare_denoise fixes - geometry, models and their controls, streams, pools,
    index tensors; BUFFERS: what the inputs are copied into in place (captured graphs keep reading them), the eps hand-off, accumulators,
    device words, the bound scalars; CACHES: filled while the loop runs.  Nothing else can be set."""
    PLAN = ("cfg cbs f_tot nf num_inference_steps windows global_context frame_idx dist rank world_size emulate branches np_slot units unit_tv "
            "bank_variants n_slots calls cn_frames T groups row_table "
            "timesteps t_dtype t_table C4 h w HW n_ref_images ring bank_C appearance_encoder writer reader controlnet sched_frozen return_eps "
            "use_graphs graph_pool writer_pool lookahead side cn_pos cn_chunks cn_text text_c").split()
    BUFFERS = ("latents lat_in history text ref_lat audio_features speed face_rows cn_cond send recv noise_pred counter t_buf ref_t bank_idx "
               "guidance_scale eta seed cn_scale").split()
    CACHES = "plans graphs ref_ctx_kv kv_all ref_sel ref_recv ref_gath bank_pack stage".split()        # dicts, keyed as their users say
    __slots__ = PLAN + BUFFERS + CACHES + "bank_L cn_embed cn_down cn_mid group_ready group_pending groups_launched eps_trace sched_first".split()

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, {} if k in self.CACHES else None)
        self.group_ready, self.group_pending, self.groups_launched, self.eps_trace = -1, -1, 0, []


def reference_group_size(reference_group, n_steps, world_size=1):
    """ReferenceNet timesteps per batched pass: at least 1, never more than the loop has steps; with world_size > 1 the ranks deal a group's
    timesteps among themselves, and a size that is not a multiple of world_size would pad every rank to ceil(T / world) timesteps (10 over 8
    ranks: 16 computed and shipped, 10 used) - rounded up to a multiple instead, still capped by the step count."""
    T = max(1, min(int(reference_group), int(n_steps)))
    if world_size > 1:
        T = min(-(-T // world_size) * world_size, int(n_steps))
    return T


def loop_plan(f_tot, num_inference_steps, n_timesteps, *, context_frames=16, context_stride=1, context_overlap=4, context_batch_size=1,
              context_schedule="uniform", cfg=True, text_pairing="reference", rank=0, world_size=1, dist=False, _emulate_rank=None,
              reference_group=10):
    """The host half of prepare_denoise, from plain numbers to a plan of Python lists, dicts and ints (its fields are LoopState's first PLAN
    names; the calls are LoopCall records): windows, window batches, duplicate-frame marks, work units, each unit's text / bank variant, the
    rank's UNet calls and slots, the frames its ControlNet pass covers, the ReferenceNet groups and the bank row table.
    text_pairing (matters at context_batch_size > 1 only): "reference" = the upstream row pairing, literally (see `unit_tv` below: odd
    windows of a batch run their uncond row under the cond text and vice versa, which cancels guidance for them); "branch" = the evidently
    intended one, every row under its own branch's text and the cond-text bank - the same function as context_batch_size 1, batched.
    _emulate_rank=(r, n): MEASUREMENT aid (bench.py --emulate-rank): the work of rank r of an n-rank job - its units, its share of every
    ReferenceNet group - in ONE process without collectives (so the latents are not a sample of anything): a rank's critical path per step."""
    if text_pairing not in ("reference", "branch"):
        raise ValueError(f"text_pairing must be 'reference' or 'branch', got {text_pairing!r}")
    p = SimpleNamespace(cfg=bool(cfg), cbs=int(context_batch_size), f_tot=int(f_tot), num_inference_steps=num_inference_steps)
    cbs = p.cbs
    if cbs < 1:
        raise ValueError("context_batch_size must be >= 1")
    scheduler_fn = get_context_scheduler(context_schedule)
    # the reference recomputes the (step-independent: step arg is always 0) window list every step (:748-755)
    p.windows = [list(map(int, c)) for c in scheduler_fn(0, num_inference_steps, p.f_tot, context_frames, context_stride, context_overlap)]
    p.nf = len(p.windows[0])
    if any(len(c) != p.nf for c in p.windows):
        raise ValueError("context windows of unequal length")
    p.global_context = [p.windows[i:i + cbs] for i in range(0, len(p.windows), cbs)]      # the reference's window batches (:752-755)
    # `noise_pred[:, :, c] = noise_pred[:, :, c] + pred` (:792-794) with a frame listed twice in c (wrapped windows at
    # context_stride > 1) keeps ONE occurrence (the last write wins): positions of earlier duplicates are marked -1
    p.frame_idx = []
    for c in p.windows:
        last = {k: j for j, k in enumerate(c)}
        p.frame_idx.append([k if last[k] == j else -1 for j, k in enumerate(c)])
    # ---- work units: U = [(window, branch)], branch 0 = uncond, 1 = cond; rank r owns U[r::world].  A UNet
    # call batches up to 2*cbs of the rank's units, uncond units first (they skip the reference banks, :243-256) - at
    # world_size 1 that is exactly the reference's [uc x cbs, c x cbs] batch (:759-763).
    p.dist = bool(dist)
    p.rank, p.world_size = (int(rank), int(world_size)) if p.dist else (0, 1)
    p.emulate = _emulate_rank is not None
    if p.emulate:
        if p.dist:
            raise ValueError("_emulate_rank replaces dist=True")
        p.rank, p.world_size = int(_emulate_rank[0]), int(_emulate_rank[1])
    # (branch-major order: with as many windows as ranks a rank owns BOTH branches of one window - balanced, the cond
    # branch costs ~8 % more - and with twice as many ranks as windows, BASELINE configs[3], every rank owns one unit)
    p.branches = (0, 1) if p.cfg else (1,)
    p.np_slot = {br: i for i, br in enumerate(p.branches)}           # branch -> plane of the noise_pred accumulator
    p.units = [(w, br) for br in p.branches for w in range(len(p.windows))]
    # Text / bank VARIANT of a unit.  The reference stacks `torch.cat([text_embeddings] * context_batch_size)` (:631) = [uc, c, uc, c, ..] against
    # latent rows [w0, w1, .., w0, w1, ..] (:759-763) and a uc mask [1, .., 0, ..] (mutual_self_attention.py:186-197): row r = branch * n + j of a
    # batch of n windows is paired with text row r % 2, and a cond row reads bank row r - written by the ReferenceNet under text row r % 2 as well
    # (:711-716).  At context_batch_size 1 that is variant = branch; at context_batch_size > 1 it is NOT (window 0's cond row runs under the uncond
    # text and the uncond-text bank) - reference behaviour, reproduced (golden `ddim_cbs2`); text_pairing="branch" pairs by branch instead.
    p.unit_tv = {}
    pos = 0
    for wb in p.global_context:
        n = len(wb)
        for j in range(n):
            for br in p.branches:
                p.unit_tv[(pos + j, br)] = (br if text_pairing == "branch" else (br * n + j) % 2) if p.cfg else 1
        pos += n
    p.bank_variants = sorted({p.unit_tv[u] for u in p.units if u[1] == 1})   # the same on every rank
    mine = p.units[p.rank::p.world_size]
    p.n_slots = -(-len(p.units) // p.world_size)                    # units per rank, padded
    p.calls = []
    # which of the rank's units share a UNet call (a unit's SLOT - its place in the exchange buffer - stays its index in `mine`).  context_batch_size
    # 1: the two branches of a window go together, [uncond, cond] - the reference's batch (:759-763), and the one whose halves share their prefix
    # (unet._begin); units whose sibling lives on another rank are batched in pairs.  context_batch_size > 1: consecutive units, 2 * cbs per call.
    if cbs == 1 and p.cfg:
        byw = {}
        for k, (w_, br) in enumerate(mine):
            byw.setdefault(w_, {})[br] = k
        chunks = [[byw[w_][0], byw[w_][1]] for w_ in sorted(byw) if len(byw[w_]) == 2]
        singles = sorted((k for w_ in byw if len(byw[w_]) == 1 for k in byw[w_].values()), key=lambda k: (mine[k][1], k))
        chunks += [singles[i:i + 2] for i in range(0, len(singles), 2)]
    else:
        n_per = len(p.branches) * cbs
        chunks = [list(range(i, min(i + n_per, len(mine)))) for i in range(0, len(mine), n_per)]
    for idxs in chunks:
        chunk = [mine[k] for k in idxs]
        uc = [k for k, u in enumerate(chunk) if u[1] == 0]
        # one UNet call reads ONE bank (the row named by a device word): cond units are batched per bank variant
        for n_call, tv in enumerate(sorted({p.unit_tv[u] for u in chunk if u[1] == 1}, reverse=True) or [None]):
            order = (uc if n_call == 0 else []) + [k for k, u in enumerate(chunk) if u[1] == 1 and p.unit_tv[u] == tv]
            call = LoopCall([chunk[k] for k in order], [idxs[k] for k in order], tv)
            # [uncond windows..., cond windows...] over the SAME windows in the same order: the two halves of the UNet batch
            # carry identical latents and differ only from the first cross-attention on (unet._begin shares that prefix)
            call.halves_identical = (call.n_uc * 2 == len(call.units) and call.n_uc > 0 and
                                     [u[0] for u in call.units[:call.n_uc]] == [u[0] for u in call.units[call.n_uc:]])
            call.frames = [k for w, _ in call.units for k in p.windows[w]]
            p.calls.append(call)
    # the frames this rank's units touch: the ControlNet residuals are computed once per such frame and step
    p.cn_frames = sorted({k for call in p.calls for k in call.frames})
    if p.emulate:          # no exchange: the accumulators see this rank's units only
        p.units = mine
    # ---- ReferenceNet groups: the banks depend on the timestep only (never on the latents): T timesteps per pass, two groups resident
    p.T = T = reference_group_size(reference_group, n_timesteps, p.world_size)
    p.groups = [list(range(i, min(i + T, n_timesteps))) for i in range(0, n_timesteps, T)]
    p.row_table = [((s_ // T) % 2) * T + s_ % T for s_ in range(n_timesteps)]
    return p


class DenoiseLoop:
    """The loop's methods; EMOAnimationPipeline inherits them and supplies unet, scheduler, vae_scale_factor, face_region_controller, _plan_cache."""
    reference_group_size = staticmethod(reference_group_size)

    @torch.no_grad()
    def prepare_denoise(self, latents, ref_image_latents, text_embeddings, *, appearance_encoder, num_inference_steps=50, guidance_scale=7.5,
                        eta=0.0, context_frames=16, context_stride=1, context_overlap=4, context_batch_size=1, context_schedule="uniform",
                        audio_features=None, speed_embeddings=None, seed=0, fusion_blocks="midup", dist=False, rank=0, world_size=1,
                        return_eps=False, use_graphs=None, controlnet=None, controlnet_cond=None, controlnet_conditioning_scale=1.0,
                        reference_group=10, reference_lookahead=None, motion_latents=None, text_pairing="reference", _emulate_rank=None,
                        face_mask=None, face_mask_threshold=None):
        """Set up the loop state (EMOAnimationPipeline.py:628-696) in three steps - `loop_plan` (which also explains text_pairing and
        _emulate_rank), its lists as device tensors, the allocations - and bind the inputs (CLIP_INPUTS).  latents f32 (1,4,F_tot,h,w);
        ref_image_latents (1,4,h,w); text_embeddings (2,L,D) = [uncond, cond].
        reference_group = T: ReferenceNet timesteps computed per batched pass (1 = the reference's per-step order).
        use_graphs: None (default) = HIP-graph replay of the UNet / ReferenceNet passes whenever the model lives on a HIP device (the path
        bench.py measures; ~1700 launches per step leave the host), False = every kernel launched from Python.
        motion_latents (n_m, 4, h, w): latents of the previous clip's last frames, next to the reference image (see denoise_chained).
        speed_embeddings (1 | 2, 4*C0) is one embedding per clip, (1 | 2, F_tot, 4*C0) one per frame, gathered per UNet call like the audio context.
        face_mask: an (H, W) / (1, 1, H, W) map at pixel or latent size, turned into (h*w, C0) rows ONCE per clip (`_face_feature_rows`);
        face_mask_threshold=t pools (mask > t) instead of the mask (FaceLocator logits: t = 0).  Both are replicated on every rank."""
        unet, sch, dev = self.unet, self.scheduler, self.unet.device
        if face_mask is not None:      # (argument errors before anything is allocated or launched)
            self._check_face_mask(face_mask, latents.shape[3] * self.vae_scale_factor, latents.shape[4] * self.vae_scale_factor)
        self._check_speed_embeddings(speed_embeddings, latents.shape[2])
        # `do_classifier_free_guidance = guidance_scale > 1.0` (:622).  Without it the UNet batch is the window batch (:759-763 `.repeat(1)`), the text
        # is the cond embedding alone, every row reads the bank and eps = noise_pred / counter.  (The reference's own lines do not run in that mode:
        # :790 unpacks a one-row batch and the reader of :634 would mask half of the FRAMES off the bank; pinned by the `ddim_nocfg` loop golden.)
        cfg = self._do_cfg(guidance_scale)
        if latents.shape[0] != 1:
            raise ValueError("batch_size must be 1 (EMOAnimationPipeline.py:641-642); run clips as separate calls")
        text_embeddings = self._text_rows(text_embeddings, cfg)
        timesteps = list(sch.set_timesteps(num_inference_steps))
        # ---- 1. the plan
        st, plan = LoopState(), loop_plan(latents.shape[2], num_inference_steps, len(timesteps), context_frames=context_frames, context_stride=context_stride,
            context_overlap=context_overlap, context_batch_size=context_batch_size, context_schedule=context_schedule, cfg=cfg,
            text_pairing=text_pairing, rank=rank, world_size=world_size, dist=dist, _emulate_rank=_emulate_rank, reference_group=reference_group)
        for k, v in vars(plan).items():
            setattr(st, k, v)
        # ---- 2. its lists on the device.  Every step is emo_sched_step with a per-step plan: the state keeps its own copy of the scheduler's tables
        # (the object is shared: another set_timesteps must not move a state still being stepped), a ring of earlier model outputs and `lat_in`, the
        # next step's model input, written by the step kernel and gathered by the UNet / ControlNet passes - no input scale is baked into a graph
        st.timesteps = timesteps
        st.t_dtype = torch.float32 if getattr(sch, "float_timesteps", False) else torch.int64
        st.sched_frozen = copy.deepcopy(sch)
        st.t_table = torch.tensor(timesteps, dtype=st.t_dtype, device=dev)   # INT timestep table, bit-exact (f32: Euler / LMS)
        st.frame_idx = [torch.tensor(f, dtype=torch.int32, device=dev) for f in plan.frame_idx]
        st.row_table = torch.tensor(plan.row_table, dtype=torch.int32, device=dev)
        for call in st.calls:      # a unit's frames, one index tensor per unit
            call.idx = list(torch.tensor(call.frames, dtype=torch.int64, device=dev).split(st.nf))
        # ---- 3. allocations
        st.latents = torch.empty(tuple(latents.shape), device=dev, dtype=torch.float32)
        _, st.C4, _, st.h, st.w = st.latents.shape
        st.HW = st.h * st.w
        # text rows indexed by VARIANT: 0 = uncond, 1 = cond (without guidance both name the cond row)
        st.text = torch.empty(2, *text_embeddings.shape[1:], device=dev, dtype=torch.float32)
        st.text_c = st.text[1:2]
        st.appearance_encoder = appearance_encoder
        st.writer = ReferenceAttentionControl(appearance_encoder, do_classifier_free_guidance=True, mode="write",
                                              batch_size=st.cbs, fusion_blocks=fusion_blocks)      # :633
        st.reader = ReferenceAttentionControl(unet, do_classifier_free_guidance=cfg, mode="read", batch_size=st.cbs,
                                              fusion_blocks=fusion_blocks)                        # :634
        st.lat_in = torch.empty_like(st.latents)
        st.ring = int(sch.history)
        st.history = torch.empty(st.ring, st.latents.numel(), device=dev, dtype=torch.float32) if st.ring else None
        # ReferenceNet images = [reference, motion frames] (Net.py:56-72 intent; junk/EMo-write-up.txt:104-110)
        st.n_ref_images = 1 + (0 if motion_latents is None else self._motion_rows(motion_latents).shape[0])
        st.ref_lat = torch.empty(st.n_ref_images, st.C4, st.h, st.w, device=dev, dtype=torch.float32)
        st.t_buf = torch.zeros(1, dtype=st.t_dtype, device=dev)
        st.use_graphs = (use_graphs is None or bool(use_graphs)) and dev.type == "cuda"   # None: the measured path is the default on a HIP device
        if st.use_graphs:
            # (the writer has its own pool: the ReferenceNet pass runs concurrently with the Backbone)
            st.graph_pool, st.writer_pool = torch.cuda.graph_pool_handle(), torch.cuda.graph_pool_handle()
        # ---- contexts of the attn2 layers: their K / V^T projections depend on the context only -> once per clip (_bind_inputs)
        st.audio_features = None if audio_features is None else torch.empty(tuple(audio_features.shape), device=dev, dtype=torch.float32)
        st.speed = None if speed_embeddings is None else torch.empty(tuple(speed_embeddings.shape), device=dev, dtype=torch.float32)
        # the face-region rows every UNet call adds behind conv_in: ONE buffer, rewritten per clip (captured graphs keep its address)
        st.face_rows = None if face_mask is None else torch.empty(st.HW, unet.config.block_out_channels[0], device=dev, dtype=unet.dtype)
        # ---- eps hand-off: every unit's rows (nf*HW, C4); slot = position in the rank's unit list
        st.send = torch.zeros(st.n_slots, st.nf * st.HW, st.C4, device=dev, dtype=unet.dtype)
        st.recv = torch.zeros(st.world_size, st.n_slots, st.nf * st.HW, st.C4, device=dev, dtype=unet.dtype) if st.dist else None
        st.noise_pred = torch.empty(len(st.branches), st.C4, st.f_tot, st.HW, device=dev, dtype=torch.float32)
        st.counter = torch.empty(st.f_tot, device=dev, dtype=torch.float32)
        st.return_eps = return_eps
        st.ref_t = torch.zeros(st.T, dtype=st.t_dtype, device=dev)
        st.bank_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        spec_r = appearance_encoder.spec
        chan = {a.prefix: a.channels for blk in spec_r.down + [spec_r.mid] + spec_r.up for a in blk.attentions if a is not None}
        st.bank_C = [chan[p] for p in st.writer.order]
        # look-ahead = group g+1's ReferenceNet pass on a second stream under group g's Backbone steps.  With world_size > 1 the side stream carries
        # the WRITE passes only; the bank all_gather stays on the main stream and on the communicator of the per-step eps all_gather (see
        # _ensure_group): one program order of collectives on every rank, so the overlap is safe at any world size and on by default (None).
        st.lookahead = (reference_lookahead is None or bool(reference_lookahead)) and dev.type == "cuda"
        st.side = torch.cuda.Stream() if st.lookahead else None
        # ControlNet branch (EMOAnimationPipeline.py:643-650,678-679,718-746): (F_tot,3,H,W) conditioning images in [0,1]
        st.controlnet = controlnet
        if controlnet is not None:
            if controlnet_cond is None or controlnet_cond.shape[0] != st.f_tot:
                raise ValueError("controlnet_cond must hold one (3,H,W) conditioning image per frame")
            st.cn_cond = torch.empty(tuple(controlnet_cond.shape), device=dev, dtype=torch.float32)
            # residuals are computed once per frame this rank touches (plan.cn_frames) and step, in chunks of context_frames (the reference caches
            # them per frame from overlap-0 windows: the network is per-frame, so the chunking does not enter the result)
            st.cn_pos = {k: i for i, k in enumerate(st.cn_frames)}
            st.cn_chunks = [torch.tensor(st.cn_frames[i:i + context_frames], dtype=torch.int64, device=dev)
                            for i in range(0, len(st.cn_frames), context_frames)]
            st.cn_text = st.text_c                                   # cond text embedding (:678-679)
            for call in st.calls:
                call.cn_sel = torch.tensor([st.cn_pos[k] for k in call.frames], dtype=torch.int64, device=dev)
        given = locals()      # every clip input is a parameter of this function under its name in the table
        self._bind_inputs(st, **{r.name: given[r.name] for r in CLIP_INPUTS})
        return st

    # ---- the INPUTS of a prepared loop state, copied into its buffers in place (the captured graphs keep reading them)
    @staticmethod
    def _do_cfg(guidance_scale):
        """`do_classifier_free_guidance = guidance_scale > 1.0` (:622), decided on the f32 value emo_sched_step receives: a scale
        in (1, 1 + 2^-24] would otherwise allocate two noise_pred planes for a kernel that reads one."""
        import numpy as np
        return bool(np.float32(guidance_scale) > np.float32(1.0))

    @staticmethod
    def _text_rows(text_embeddings, cfg):
        if text_embeddings.shape[0] == 2 and not cfg:
            text_embeddings = text_embeddings[1:]          # [uncond, cond] handed over anyway: the cond row is the prompt
        if text_embeddings.shape[0] != (2 if cfg else 1):
            raise ValueError("text_embeddings must be (2, L, D) = [uncond, cond] (:631), or (1, L, D) = [cond] without guidance")
        return text_embeddings

    @staticmethod
    def _motion_rows(motion_latents):
        return motion_latents[0].permute(1, 0, 2, 3) if motion_latents.dim() == 5 else motion_latents

    @staticmethod
    def _check_speed_embeddings(speed_embeddings, video_length):
        """(1 | 2, 4*C0): one embedding per clip, shared or [uncond, cond]; (1 | 2, video_length, 4*C0): one per frame"""
        se = speed_embeddings
        if se is None:
            return
        if se.dim() not in (2, 3) or se.shape[0] not in (1, 2):
            raise ValueError("speed_embeddings must have 1 row (shared) or 2 rows [uncond, cond]: (1 | 2, 4*C0) per clip or "
                             f"(1 | 2, video_length, 4*C0) per frame, got {tuple(se.shape)}")
        if se.dim() == 3 and se.shape[1] != video_length:
            raise ValueError(f"per-frame speed_embeddings hold {se.shape[1]} frames, the clip has {video_length}")

    def _check_face_mask(self, face_mask, height, width, locate_ok=False):
        """The argument checks of `face_mask=` (nothing is launched): a FaceRegionController(1, block_out_channels[0]) on the pipeline,
        and an (H, W) / (1, 1, H, W) map at pixel size (height, width) or at latent size (height / 8, width / 8).
        Returns "pixel" or "latent" (or "locate" for that string where the caller resolves it)."""
        ctl = getattr(self, "face_region_controller", None)
        C0 = self.unet.config.block_out_channels[0]
        if ctl is None:
            raise ValueError("face_mask= needs a face_region_controller on the pipeline (emote_hack_amd.conditioning.FaceRegionController(1, "
                             f"{C0}) with loaded weights: pass face_region_controller= to the constructor or assign pipe.face_region_controller)")
        if ctl.in_channels != 1 or ctl.out_channels != C0:
            raise ValueError(f"the face_region_controller maps {ctl.in_channels} -> {ctl.out_channels} channels; the mask has 1 and conv_in's "
                             f"output {C0}: build FaceRegionController(1, {C0})")
        if isinstance(face_mask, str):
            if face_mask == "locate" and locate_ok:
                return "locate"
            raise ValueError(f"face_mask={face_mask!r}: a map, or \"locate\" in the pipeline call")
        m = torch.as_tensor(face_mask)
        f = self.vae_scale_factor
        hw = tuple(m.shape) if m.dim() == 2 else tuple(m.shape[2:]) if (m.dim() == 4 and tuple(m.shape[:2]) == (1, 1)) else None
        if hw == (height, width):
            return "pixel"
        if hw == (height // f, width // f):
            return "latent"
        raise ValueError(f"face_mask must be an (H, W) or (1, 1, H, W) map at pixel size ({height}, {width}) or at latent size "
                         f"({height // f}, {width // f}), got {tuple(m.shape)}")

    def _face_feature_rows(self, st, face_mask, threshold=None):
        """face mask -> FaceRegionController input rows (h*w, 8) -> (h*w, C0) rows (train_stage_3_speedlayers.py:57-76).  A pixel-size
        map is pooled 8 x 8 (ops.mask_pool, after the optional threshold); a latent-size one goes in as it is."""
        f = self.vae_scale_factor
        kind = self._check_face_mask(face_mask, st.h * f, st.w * f)
        dev, dtp = st.latents.device, self.unet.dtype
        m = torch.as_tensor(face_mask).to(dev).float()
        m = m.reshape(m.shape[-2], m.shape[-1]).contiguous()
        if kind == "pixel":
            rows = ops.mask_pool(m, dtp, threshold=threshold)
        else:
            if threshold is not None:
                m = (m > threshold).float()
            rows = ops.ncfhw_to_rows(m.reshape(1, 1, 1, st.h, st.w), dtp, cpad=8)
        return self.face_region_controller.forward_rows(rows, 1, st.h, st.w)

    def _bind_inputs(self, st, latents, ref_image_latents=None, text_embeddings=None, **given):
        """Copy a clip's inputs - the keywords are CLIP_INPUTS' names - into the buffers of a prepared state (None = keep what is bound).  What
        is derived from them (the attn2 K / V^T of the context per UNet call, the ReferenceNet's text K / V^T) is recomputed INTO the tensors the
        captured graphs already read; the ReferenceNet groups are marked stale (the reference image and the motion frames enter them)."""
        given.update(latents=latents, ref_image_latents=ref_image_latents, text_embeddings=text_embeddings)
        for k in given:
            if k not in CLIP_INPUT_NAMES:
                raise TypeError(f"_bind_inputs() got an unexpected keyword argument {k!r}")
        unet, dev = self.unet, st.latents.device

        def put(dst, src, what):
            src = src.to(dev).float()
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"{what} {tuple(src.shape)} != prepared {tuple(dst.shape)}")
            dst.copy_(src)
        if st.side is not None:   # nothing of the previous clip may still be writing the bank cache
            torch.cuda.current_stream().wait_stream(st.side)
        speed_embeddings, motion_latents = given.get("speed_embeddings"), given.get("motion_latents")
        if speed_embeddings is not None and st.speed is not None and speed_embeddings.dim() != st.speed.dim():
            raise ValueError(f"the state was prepared with {'per-frame' if st.speed.dim() == 3 else 'per-clip'} speed_embeddings "
                             f"{tuple(st.speed.shape)}, got {tuple(speed_embeddings.shape)}")
        # ---- the generic part: an input the state has no buffer for is refused, one keyed by shape is copied into its buffer
        for rec in CLIP_INPUTS:
            if rec.buffer is not None and given.get(rec.name) is not None:
                if getattr(st, rec.buffer) is None:
                    raise ValueError(f"the state was prepared without {rec.without}")
                if rec.key == "shape":
                    put(getattr(st, rec.buffer), given[rec.name], rec.name)
        # ---- what each input entails
        if ref_image_latents is not None:
            put(st.ref_lat[:1], ref_image_latents.reshape(1, st.C4, st.h, st.w), "ref_image_latents")
        if motion_latents is not None:
            ml = self._motion_rows(motion_latents)
            if st.n_ref_images == 1 or tuple(ml.shape) != (st.n_ref_images - 1, st.C4, st.h, st.w):
                raise ValueError(f"motion_latents must be ({st.n_ref_images - 1}, {st.C4}, {st.h}, {st.w}), got {tuple(ml.shape)}")
            put(st.ref_lat[1:], ml, "motion_latents")
        elif st.n_ref_images != 1 and ref_image_latents is not None:
            raise ValueError("the state was prepared with motion frames: pass motion_latents")
        if given.get("guidance_scale") is not None:
            if self._do_cfg(given["guidance_scale"]) != st.cfg:
                raise ValueError("guidance_scale crosses 1.0: classifier-free guidance on / off is part of the plan (prepare again)")
            st.guidance_scale = float(given["guidance_scale"])
        if given.get("eta") is not None:
            st.eta = given["eta"]
            if hasattr(st.sched_frozen, "eta"):   # DDIM: the plans read it, so none of the previous clip's may be kept
                st.sched_frozen.eta = st.eta
                st.plans = {}
        if given.get("seed") is not None:
            st.seed = given["seed"]
        ctx_stale = given.get("audio_features") is not None
        if text_embeddings is not None:
            t = self._text_rows(text_embeddings, st.cfg).to(dev).float()
            put(st.text, t if st.cfg else t.expand(2, -1, -1), "text_embeddings")
            ctx_stale = True
            for tv in st.bank_variants:
                for pr, kv in st.appearance_encoder.context_kv(st.text[tv:tv + 1]).items():
                    self._put_kv(st.ref_ctx_kv.setdefault(tv, {}), pr, kv)
        if given.get("face_mask") is not None:
            st.face_rows.copy_(self._face_feature_rows(st, given["face_mask"], given.get("face_mask_threshold")))
        for call in st.calls:
            if ctx_stale:
                if st.audio_features is None:
                    ctx = torch.cat([st.text[st.unit_tv[u]:st.unit_tv[u] + 1] for u in call.units])    # (n, L, D)
                else:   # per-frame audio context; uncond units get a zero context (design choice)
                    rows = [st.audio_features.index_select(0, ix) for ix in call.idx]
                    ctx = torch.cat([a if br == 1 else torch.zeros_like(a) for (_, br), a in zip(call.units, rows)])     # (n*F, L_a, D)
                call.ctx = ctx if call.ctx is None else call.ctx.copy_(ctx)      # (in place: captured graphs hold its address)
                for pr, kv in unet.context_kv(call.ctx).items():
                    self._put_kv(call.ctx_kv, pr, kv)
            if speed_embeddings is not None:
                se = st.speed
                rows = [br if se.shape[0] == 2 else 0 for _, br in call.units]      # shared, or [uncond, cond]
                if se.dim() == 3:   # per frame: the rows of each unit's window, gathered like the audio context -> (n, nf, 4*C0)
                    sp = torch.stack([se[r].index_select(0, ix) for r, ix in zip(rows, call.idx)])
                else:
                    sp = torch.cat([se[r:r + 1] for r in rows])
                call.speed = sp if call.speed is None else call.speed.copy_(sp)
        if given.get("controlnet_cond") is not None:
            # the conditioning embedding (controlnet.py:523) depends on the conditioning images only: once per clip, not per step
            embeds = [st.controlnet.cond_embedding(st.cn_cond.index_select(0, idx)) for idx in st.cn_chunks]
            if st.cn_embed is None:
                st.cn_embed = embeds
            else:
                for (dst, _, _), (src, _, _) in zip(st.cn_embed, embeds):
                    dst.copy_(src)
        if given.get("controlnet_conditioning_scale") is not None and st.controlnet is not None:
            scale = float(given["controlnet_conditioning_scale"])
            if st.cn_scale not in (None, scale) and st.graphs.get("controlnet") not in (None, "warm"):
                raise ValueError("controlnet_conditioning_scale is baked into the captured ControlNet pass (prepare again)")
            st.cn_scale = scale
        st.group_ready, st.group_pending, st.eps_trace = -1, -1, []
        st.sched_first = None      # the multistep warm-up and lat_in restart at the next step that runs

    @staticmethod
    def _put_kv(store, key, kv):
        """store[key] = (K rows, V^T) - into the tensors already there, if any (captured graphs hold their addresses)"""
        if key in store:
            for dst, src in zip((store[key],) if torch.is_tensor(store[key]) else store[key], (kv,) if torch.is_tensor(kv) else kv):
                dst.copy_(src)
        else:
            store[key] = kv

    # ---- ReferenceNet: one batched write pass per GROUP of timesteps, one group ahead of the Backbone on a second stream
    def _ref_sel(self, st, Tg):
        """group-local timestep indices this rank computes (rank r: r, r+world, ...; padded by repeating the last one)"""
        if Tg not in st.ref_sel:
            mine = [min(st.rank + i * st.world_size, Tg - 1) for i in range(-(-Tg // st.world_size))]
            st.ref_sel[Tg] = torch.tensor(mine, dtype=torch.int64, device=st.ref_t.device)
        return st.ref_sel[Tg]

    def _part_reference_write(self, st, Tg, tv):
        """ReferenceNet write pass (:711-716) under text variant tv (1 = the cond text) for this rank's share of the group's timesteps, batched:
        (n,4,h,w) with one timestep per row.  The reference runs [uncond-text, cond-text] copies every step; only the variants some cond unit reads
        (st.bank_variants) are computed - the uc rows never use their bank row (mutual_self_attention.py:243-256) and the ReferenceNet is
        batch-independent.  Banks are rounded through fp16 like reader.update() does (:588) and packed for the exchange."""
        t = st.ref_t[:Tg] if st.world_size == 1 else st.ref_t.index_select(0, self._ref_sel(st, Tg))
        n, k = t.numel(), st.n_ref_images
        st.appearance_encoder._reference_control = st.writer   # (another prepared state on the same models may have attached its own)
        st.writer.clear()
        # batch rows timestep-major: (t0: reference image, motion frames...), (t1: ...) - the k images of one timestep are
        # consecutive, so their LN1 rows (k, L, C) read as ONE bank of k*L tokens (the reference concatenates several bank
        # entries along tokens the same way, mutual_self_attention.py:239)
        imgs = st.ref_lat.expand(n, -1, -1, -1) if k == 1 else st.ref_lat.repeat(n, 1, 1, 1)
        tt = t if k == 1 else t.repeat_interleave(k)
        st.appearance_encoder(imgs, tt, encoder_hidden_states=st.text[tv:tv + 1], return_dict=False, _ctx_kv=st.ref_ctx_kv[tv])
        tgt = self.unet.dtype
        st.bank_L = [k * st.writer.bank[p][0].shape[1] for p in st.writer.order]
        banks = [ops.convert(st.writer.bank[p][0], tgt, fp16_round=True).reshape(n, -1) for p in st.writer.order]
        st.writer.clear()                                                                      # :823
        # (keyed by the group size as well: a replayed graph of another group size writes ITS tensors, not the last ones bound here)
        st.bank_pack[(Tg, tv)] = banks if st.world_size == 1 else torch.cat(banks, dim=1)      # (n, total) plumbing copy

    def _part_reference_project(self, st, Tg, tv):
        """K / V^T projections of the group's banks with the BACKBONE's attn1.to_k / to_v (the read side of
        mutual_self_attention.py:238-241), once per group instead of once per step."""
        st.stage[(Tg, tv)] = {}
        off = 0
        for i, (pr, L, C_) in enumerate(zip(st.reader.order, st.bank_L, st.bank_C)):
            if st.world_size == 1:
                rows = st.bank_pack[(Tg, tv)][i]
            else:   # bank i occupies columns [off, off + L*C) of every gathered row (rows in group order)
                rows = st.ref_gath[(Tg, tv)][:Tg, off:off + L * C_].contiguous()
                off += L * C_
            k, vt = self.unet.bank_kv(pr, rows.reshape(-1, C_), L)
            st.stage[(Tg, tv)][pr] = (k, vt, L)

    def _reference_write(self, st, g):
        """Phase 1 of group g: this rank's share of the group's ReferenceNet write passes (no communication) on the CURRENT stream."""
        steps = st.groups[g]
        Tg = len(steps)
        st.groups_launched += 1
        st.ref_t[:Tg].copy_(st.t_table[steps[0]:steps[0] + Tg], non_blocking=True)
        for tv in st.bank_variants:
            self._run(st, ("ref_write", Tg, tv), lambda tv=tv: self._part_reference_write(st, Tg, tv), pool=st.writer_pool)

    def _reference_finish(self, st, g):
        """Phase 2 of group g on the CURRENT stream: the bank exchange (world_size > 1), the K / V^T projection of the whole group with the
        Backbone's weights, and the copy into slot g % 2 of the resident cache."""
        steps = st.groups[g]
        Tg, T, slot = len(steps), st.T, g % 2
        for tv in st.bank_variants:
            if st.world_size > 1:
                # north_star: "RCCL all-gather over xGMI to broadcast ReferenceNet features" - rank r computed timesteps r, r+world, ... of the group;
                # ONE all_gather hands every rank every timestep's banks.  Same communicator and stream as the per-step eps all_gather: every rank
                # issues its collectives in ONE program order (eps, banks of the next group, eps, ...), so no start-order hazard exists by construction
                import torch.distributed as td
                send = st.bank_pack[(Tg, tv)]
                n = send.shape[0]
                if (Tg, tv) not in st.ref_gath:
                    st.ref_recv[(Tg, tv)] = torch.empty(st.world_size * n, send.shape[1], device=send.device, dtype=send.dtype)
                    st.ref_gath[(Tg, tv)] = torch.empty(st.world_size * n, send.shape[1], device=send.device, dtype=send.dtype)
                if st.emulate:      # (stands in for the gathered rows: this rank's banks, repeated)
                    st.ref_recv[(Tg, tv)].view(st.world_size, -1).copy_(send.contiguous().view(1, -1).expand(st.world_size, -1))
                else:
                    td.all_gather_into_tensor(st.ref_recv[(Tg, tv)].view(-1), send.contiguous().view(-1))
                # row (rank r, slot i) is group-local timestep i*world + r -> group order
                st.ref_gath[(Tg, tv)].view(n, st.world_size, -1).copy_(st.ref_recv[(Tg, tv)].view(st.world_size, n, -1).transpose(0, 1))
            self._run(st, ("ref_project", Tg, tv), lambda tv=tv: self._part_reference_project(st, Tg, tv), pool=st.writer_pool)
            if tv not in st.kv_all:   # resident cache: two groups of T timesteps per block
                st.kv_all[tv] = {}
                for pr, (k, vt, L) in st.stage[(Tg, tv)].items():
                    st.kv_all[tv][pr] = (torch.zeros(2 * T * L, k.shape[1], device=k.device, dtype=k.dtype),
                                         torch.zeros(2 * T, vt.shape[1], vt.shape[2], device=vt.device, dtype=vt.dtype), L)
            dsts, srcs = [], []
            for pr, (k, vt, L) in st.stage[(Tg, tv)].items():
                ka, va, _ = st.kv_all[tv][pr]
                dsts += [ka[slot * T * L:slot * T * L + Tg * L], va[slot * T:slot * T + Tg]]
                srcs += [k[:Tg * L], vt[:Tg]]
            torch._foreach_copy_(dsts, srcs)

    def _reference_group(self, st, g):
        """Compute group g's projected banks on the CURRENT stream and store them in slot g % 2 of the resident cache."""
        self._reference_write(st, g)
        self._reference_finish(st, g)

    def _ensure_group(self, st, si):
        """Group of step si resident (waiting for / computing it if needed), the NEXT group launched on the side stream: the whole pass (write,
        projection, cache copy) at world_size 1, only its communication-free WRITE pass at world_size > 1 - the bank all_gather and the projection
        are issued on the MAIN stream when the loop reaches the group, in program order with the per-step eps all_gather on the one communicator
        both use (EMOAnimationPipeline.py:796-821 is the exchange this replaces)."""
        g = si // st.T
        cuda = self.unet.device.type == "cuda"
        main = torch.cuda.current_stream() if cuda else None
        split = st.world_size > 1
        if st.group_ready != g:
            if st.group_pending == g:
                main.wait_stream(st.side)
                if split:
                    self._reference_finish(st, g)
            else:
                if st.group_pending >= 0 and cuda:   # a look-ahead pass for ANOTHER group is in flight (the caller jumped): it shares the
                    main.wait_stream(st.side)        # timestep buffer and the captured write graphs with the pass below
                self._reference_group(st, g)
            st.group_ready, st.group_pending = g, -1
            if g + 1 < len(st.groups) and st.lookahead:
                # slot (g+1) % 2 held group g-1: every step of it is already enqueued on the main stream
                st.side.wait_stream(main)
                with torch.cuda.stream(st.side):
                    if split:
                        self._reference_write(st, g + 1)
                    else:
                        self._reference_group(st, g + 1)
                st.group_pending = g + 1

    # ---- ControlNet (per-frame residual cache of the step, :718-746)
    def _part_controlnet(self, st):
        downs, mids = [], []
        for i, idx in enumerate(st.cn_chunks):
            x = st.lat_in.index_select(2, idx)[0].permute(1, 0, 2, 3).contiguous()     # the scaled model input, written by the step kernel
            d, m = st.controlnet(x, st.t_buf, encoder_hidden_states=st.cn_text.repeat(idx.numel(), 1, 1), controlnet_cond=None,
                                 conditioning_scale=st.cn_scale, return_dict=False, _cond_rows=st.cn_embed[i])
            downs.append(d)
            mids.append(m)
        st.cn_down = [torch.cat([d[i] for d in downs]) for i in range(len(downs[0]))]
        st.cn_mid = torch.cat(mids)

    def _controlnet_residuals(self, st, call):
        """select_controlnet_res_samples (:514-540): frames of the call's units, '(b f) c h w -> b c f h w' (the CFG repeat of
        the reference is the uncond and the cond unit of a window selecting the same frames)."""
        if st.controlnet is None:
            return {}
        n, nf = len(call.units), st.nf

        def to5(t):
            y = t.index_select(0, call.cn_sel)
            return y.reshape(n, nf, *y.shape[1:]).permute(0, 2, 1, 3, 4)
        return dict(down_block_additional_residuals=tuple(to5(t) for t in st.cn_down), mid_block_additional_residual=to5(st.cn_mid))

    # ---- one UNet call = the rank's next <= 2*cbs units; reads the timestep from the device buffer st.t_buf and the bank row
    #      from st.bank_idx, so it is captured once into a HIP graph and replayed for the other steps
    def _part_unet(self, st, ci):
        call = st.calls[ci]
        x = torch.cat([st.lat_in.index_select(2, ix) for ix in call.idx])   # :759-763; the scaled model input, written by the step kernel
        # (a call of uncond units only names any resident cache: every one of its batches skips the bank segment)
        bank_tv = call.bank_tv if call.bank_tv is not None else st.bank_variants[0]
        self.unet._reference_control = st.reader
        st.reader.set_projected_banks(st.kv_all[bank_tv], st.bank_idx, call.n_uc)               # replaces reader.update (:774)
        face = {} if st.face_rows is None else dict(face_features=st.face_rows)      # (a call without one launches what it always did)
        rows = self.unet(x, st.t_buf, encoder_hidden_states=call.ctx, speed_embeddings=call.speed, return_dict=False,
                         _return_rows=True, _ctx_kv=call.ctx_kv, _halves_identical=call.halves_identical,
                         **self._controlnet_residuals(st, call), **face)   # :777-786
        n_rows = st.nf * st.HW
        for k, slot in enumerate(call.slots):
            st.send[slot].copy_(rows[k * n_rows:(k + 1) * n_rows])

    def _accumulate_all(self, st):
        """noise_pred[:, :, c] += pred; counter[:, :, c] += 1 (:790-794) over EVERY unit in global order - each rank does this
        redundantly on the gathered rows, so the accumulators (and the latents) are bit-identical on all ranks."""
        for i, (w, br) in enumerate(st.units):
            rows = st.send[i] if not st.dist else st.recv[i % st.world_size, i // st.world_size]
            ops.accumulate_window(rows, st.noise_pred[st.np_slot[br]], st.counter, st.frame_idx[w], C_=st.C4, F=st.f_tot, HW=st.HW,
                                  add_counter=(br == st.branches[0]))

    def _run(self, st, key, fn, pool=None):
        """Eager on first use (warm-up: lazy kernel attributes, allocator), HIP-graph capture on the second, replay after.
        Launch-bound host code (~1700 kernel launches per step from Python) disappears from the critical path."""
        if not st.use_graphs or ops.PROFILER is not None:
            return fn()
        state = st.graphs.get(key)
        if state is None:
            fn()
            st.graphs[key] = "warm"
            return
        if state == "warm":
            g = torch.cuda.CUDAGraph()
            # thread_local: only this thread's calls are checked during capture - the RCCL watchdog thread of a multi-GPU
            # run polls events concurrently and must not invalidate the capture
            with torch.cuda.graph(g, pool=pool if pool is not None else st.graph_pool, capture_error_mode="thread_local"):
                fn()
            st.graphs[key] = g
            state = g
        state.replay()

    @torch.no_grad()
    def denoise_step(self, st, si):
        """One iteration of the hot loop (EMOAnimationPipeline.py:698-823)."""
        if st.sched_first is None:    # the first step that runs: its model input, one scale-only launch
            st.sched_first = si
            ops.sched_scale(st.latents, st.lat_in, C_=st.C4, F=st.f_tot, HW=st.HW, s=st.sched_frozen.input_scale(si))
        self._ensure_group(st, si)                                     # :711-716, hoisted: banks of T timesteps per pass
        st.t_buf.copy_(st.t_table[si:si + 1], non_blocking=True)       # device-to-device: the INT timestep of this step
        st.bank_idx.copy_(st.row_table[si:si + 1], non_blocking=True)  # ... and its row in the resident bank cache
        st.noise_pred.zero_()
        st.counter.zero_()
        if st.emulate:
            st.counter.add_(1e-6)       # frames of the other ranks' windows: 0 / 1e-6 instead of 0 / 0
        if st.controlnet is not None and st.calls:   # per-frame residual cache of this step (:718-746)
            self._run(st, "controlnet", lambda: self._part_controlnet(st))
        for ci in range(len(st.calls)):                                                        # :757
            self._run(st, ("unet", ci), lambda ci=ci: self._part_unet(st, ci))
        if st.dist:   # replaces gather-to-root (:796-809) + broadcast (:819-821): ONE all_gather of the eps slices
            import torch.distributed as td
            td.all_gather_into_tensor(st.recv.view(-1), st.send.view(-1))
        self._accumulate_all(st)
        eps_out = torch.empty(st.C4 * st.f_tot * st.HW, device=self.unet.device, dtype=torch.float32) if st.return_eps else None
        p, slot = self._step_plan(st, si)   # :812-817 fused
        ops.sched_step(st.noise_pred, st.counter, st.latents, st.history, st.lat_in, C_=st.C4, F=st.f_tot, HW=st.HW,
                       guidance_scale=st.guidance_scale, a=p.a, b=p.b, c_x=p.c_x, c=p.c, slot=slot, c_noise=p.c_noise,
                       s_next=p.s_next, seed=st.seed, step=si, eps_out=eps_out)
        if st.return_eps:
            st.eps_trace.append(eps_out.view(1, st.C4, st.f_tot, st.h, st.w))

    @staticmethod
    def _step_plan(st, si):
        """(StepPlan, ring slots) of step si: d_n goes to slot (si - first) % ring, d_{n-k} is read from slot (si - first - k) % ring
        - the ring restarts with the first step that runs."""
        key = (st.sched_first, si)
        if key not in st.plans:
            p = st.sched_frozen.step_plan(si, st.sched_first)
            j = si - st.sched_first
            slot = [j % st.ring if st.ring else -1]
            for k in range(1, 4):
                if p.c[k] != 0.0:
                    if k > j or k >= st.ring:
                        raise RuntimeError(f"step plan of step {si} reads d_(n-{k}), which the ring does not hold")
                    slot.append((j - k) % st.ring)
                else:
                    slot.append(-1)
            st.plans[key] = (p, tuple(slot))
        return st.plans[key]

    def _run_loop(self, st, num_actual_inference_steps=None, callback=None, callback_steps=1):
        for si, t in enumerate(st.timesteps):
            if num_actual_inference_steps is not None and si < st.num_inference_steps - num_actual_inference_steps:   # :699-700
                continue
            self.denoise_step(st, si)
            if callback is not None and si % callback_steps == 0:
                callback(si, t, st.latents)
        return (st.latents, st.eps_trace) if st.return_eps else st.latents

    @torch.no_grad()
    def denoise(self, latents, ref_image_latents, text_embeddings, *, num_actual_inference_steps=None, callback=None,
                callback_steps=1, reuse_state=False, **kw):
        """The whole loop; returns the denoised latents f32 (1,4,F_tot,h,w) (and the eps trace if asked).  reuse_state: keep the prepared state
        (plan + captured HIP graphs) on the pipeline and re-arm it when the next call has the same plan - same shapes, step count, window /
        guidance / distribution settings, same loaded weights; only the inputs are copied in.  `__call__` turns it on."""
        if not reuse_state:
            st = self.prepare_denoise(latents, ref_image_latents, text_embeddings, **kw)
            return self._run_loop(st, num_actual_inference_steps, callback, callback_steps)
        key = self._plan_key(latents, ref_image_latents, text_embeddings, kw)
        cached = self._plan_cache
        if cached is not None and cached[0] == key:
            st = cached[1]
            # every clip input that was given is re-bound.  An omitted guidance_scale / eta / seed means the documented DEFAULT, not "what
            # the previous clip used" (they are not part of the plan key, so the hit happens either way; "None = keep" is reset_denoise's
            # contract, not this one's)
            given = dict(kw, latents=latents, ref_image_latents=ref_image_latents, text_embeddings=text_embeddings)
            bind = {r.name: r.hit if given.get(r.name) is None else given[r.name] for r in CLIP_INPUTS}
            self._bind_inputs(st, **{k: v for k, v in bind.items() if v is not None})
        else:
            self._plan_cache = None          # drop the old graphs before the new plan allocates
            st = self.prepare_denoise(latents, ref_image_latents, text_embeddings, **kw)
            self._plan_cache = (key, st)
        res = self._run_loop(st, num_actual_inference_steps, callback, callback_steps)
        # (the state's latents are overwritten by the next clip)
        return (res[0].clone(), list(res[1])) if isinstance(res, tuple) else res.clone()

    def clear_plan_cache(self):
        """Release the prepared state `denoise(reuse_state=True)` / `__call__` keep (buffers, captured HIP graphs, bank cache)."""
        self._plan_cache = None

    def _plan_key(self, latents, ref_image_latents, text_embeddings, kw):
        """Everything a prepared state's PLAN depends on (prepare_denoise above `_bind_inputs`): the clip inputs as CLIP_INPUTS says each
        enters (tensor shapes, presence, value, the guidance bit), the settings that shape windows / units / groups / graphs, and the
        identity of the packed weights the graphs were captured over."""
        from . import unet as unet_mod

        def wid(m):   # a re-pack (load_state_dict / .to) builds a new dict of packed tensors: captured graphs are stale
            return None if m is None else (id(m), id(getattr(m, "_w", None)), str(getattr(m, "dtype", None)))
        def sched_id(s):   # the scheduler OBJECT the state steps with and everything its tables depend on
            c = s.config   # (a user-supplied scheduler may carry a leaner config: absent fields key as None)
            return (id(s), type(s).__name__) + tuple(getattr(c, f, None) for f in (
                "num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "steps_offset", "set_alpha_to_one", "timestep_spacing",
                "solver_order", "use_karras_sigmas", "final_sigmas_type", "lower_order_final", "lms_order"))

        def pg_id():       # a state prepared with dist=True holds communicators of the default group it was made under
            if not kw.get("dist"):
                return None
            import torch.distributed as td
            return id(td.group.WORLD) if td.is_initialized() else None     # (the public handle of the default group)
        given = dict(kw, latents=latents, ref_image_latents=ref_image_latents, text_embeddings=text_embeddings)
        how = {"shape": lambda r: None if given.get(r.name) is None else tuple(given[r.name].shape),
               "presence": lambda r: given.get(r.name) is not None,
               "value": lambda r: given.get(r.name, r.default),
               "cfg": lambda r: self._do_cfg(given.get(r.name, r.default))}
        plan = {k: v for k, v in kw.items() if k not in CLIP_INPUT_NAMES + ("appearance_encoder", "controlnet")}
        return (tuple(how[r.key](r) for r in CLIP_INPUTS if r.key is not None), wid(self.unet), wid(kw.get("appearance_encoder")),
                wid(kw.get("controlnet")), sched_id(self.scheduler), pg_id(), unet_mod.SHARE_CFG_PREFIX, unet_mod.GN_FOLD_MIN_HW,
                unet_mod.GN_CONV_MIN_HW, unet_mod.MERGE_QKV, tuple(sorted((k, repr(v)) for k, v in plan.items())))

    def reset_denoise(self, st, latents, motion_latents=None, **inputs):
        """Re-arm a prepared loop state for another clip of the SAME geometry: new noisy latents (and motion frames; optionally any other input of
        CLIP_INPUTS, those with a buffer only for a state prepared with them) are copied IN PLACE, so captured HIP graphs, resident bank cache and
        communicators are reused - only the context K / V^T and the ReferenceNet groups are recomputed."""
        if tuple(latents.shape) != tuple(st.latents.shape):
            raise ValueError(f"reset_denoise: latents {tuple(latents.shape)} != prepared {tuple(st.latents.shape)}")
        if motion_latents is None and st.n_ref_images != 1:
            raise ValueError("reset_denoise: the state was prepared with motion frames")
        if motion_latents is not None:
            ml = self._motion_rows(motion_latents)
            if ml.shape[0] != st.n_ref_images - 1 or tuple(ml.shape[1:]) != (st.C4, st.h, st.w):
                raise ValueError(f"reset_denoise: motion_latents must be ({st.n_ref_images - 1}, {st.C4}, {st.h}, {st.w}), got {tuple(ml.shape)}")
        self._bind_inputs(st, latents, motion_latents=motion_latents, **inputs)
        return st

    @torch.no_grad()
    def denoise_chained(self, clips, ref_image_latents, text_embeddings, *, n_motion_frames=4, **kw):
        """Long-video generation by clip chaining (intent of Net.py:56-72 `pre_extract_motion_features` and
        junk/EMo-write-up.txt:104-110 - the reference never wires it; a design choice): clip k+1 is denoised with the LAST n_motion_frames latent
        frames of the denoised clip k as motion frames, the first clip with zero maps.  They pass through the ReferenceNet with the reference image
        and their LN1 features join the banks as extra tokens (Lk1 = (1 + n_motion_frames) * L).  `clips`: noisy latents (1, 4, F, h, w), each
        with F >= n_motion_frames; clips of one geometry share ONE prepared state.  Returns the list of denoised latents."""
        out, prev, st = [], None, None
        run_kw = {k: kw.pop(k) for k in ("num_actual_inference_steps", "callback", "callback_steps") if k in kw}
        for lat in clips:
            _, c4, f, h, w = lat.shape
            if n_motion_frames > 0:
                if f < n_motion_frames:
                    raise ValueError(f"denoise_chained: a clip of {f} frames cannot hand over {n_motion_frames} motion frames")
                motion = torch.zeros(n_motion_frames, c4, h, w) if prev is None else prev[0, :, -n_motion_frames:].permute(1, 0, 2, 3)
                if motion.shape[0] != n_motion_frames or tuple(motion.shape[2:]) != (h, w):
                    raise ValueError("denoise_chained: consecutive clips must share the latent size")
            else:
                motion = None
            if st is not None and tuple(st.latents.shape) == tuple(lat.shape):
                # (same conditioning for every clip of the chain: the face mask, per-frame speeds and the rest stay bound)
                self.reset_denoise(st, lat, motion)
            else:
                st = self.prepare_denoise(lat, ref_image_latents, text_embeddings, motion_latents=motion, **kw)
            res = self._run_loop(st, **run_kw)
            prev = (res[0] if isinstance(res, tuple) else res).clone()   # (the state's latents are overwritten by the next clip)
            out.append(prev)
        return out
