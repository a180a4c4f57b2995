"""The host plan of the sampling loop (emote_hack_amd.denoise_loop.loop_plan) over a sweep of geometries, guidance modes, text pairings,
world sizes and ReferenceNet group sizes, with every property restated from its definition; and the one table of clip inputs
(CLIP_INPUTS) against the three pieces of code derived from it: the plan key, `denoise`'s re-bind on a cache hit, `_bind_inputs`.
No model, no device."""
import inspect
import itertools

import pytest
import torch

from emote_hack_amd.context import uniform
from emote_hack_amd.denoise_loop import CLIP_INPUTS, DenoiseLoop, loop_plan, reference_group_size


def _geometries():
    for f_tot, overlap, stride, cbs, cfg, pairing in itertools.product((4, 6, 8, 12, 16), (0, 2), (1, 2), (1, 2, 3), (True, False),
                                                                       ("reference", "branch")):
        yield dict(f_tot=f_tot, overlap=overlap, stride=stride, cbs=cbs, cfg=cfg, pairing=pairing)


def _plan(g, world, rank, group, steps, emulate):
    return loop_plan(g["f_tot"], steps, steps, context_frames=4, context_stride=g["stride"], context_overlap=g["overlap"],
                     context_batch_size=g["cbs"], cfg=g["cfg"], text_pairing=g["pairing"], reference_group=group,
                     **(dict(_emulate_rank=(rank, world)) if emulate else dict(dist=world > 1, rank=rank, world_size=world)))


SHARED = ("windows", "nf", "global_context", "frame_idx", "branches", "np_slot", "unit_tv", "bank_variants", "T", "groups", "row_table")


def _check_shared(g, p, steps, group, world):
    """what every rank's plan holds alike: windows, duplicate marks, units, text variants, groups"""
    windows = [list(c) for c in uniform(0, steps, g["f_tot"], 4, g["stride"], g["overlap"])]
    assert p.windows == windows and p.nf == len(windows[0])
    assert p.global_context == [windows[i:i + g["cbs"]] for i in range(0, len(windows), g["cbs"])]
    # a frame listed twice in a window keeps its LAST occurrence
    for c, marks in zip(windows, p.frame_idx):
        assert marks == [k if k not in c[j + 1:] else -1 for j, k in enumerate(c)]
    branches = (0, 1) if g["cfg"] else (1,)
    assert tuple(p.branches) == branches and [p.np_slot[b] for b in branches] == list(range(len(branches)))
    # the text row of every batch row, built as the reference builds its batch: latent rows [w0 .. w(n-1)] * 2 against
    # cat([uc, c] * cbs)[:2n]
    want_tv, pos = {}, 0
    for batch in p.global_context:
        n = len(batch)
        if g["cfg"]:
            rows = list(range(pos, pos + n)) * 2
            text = (["uc", "c"] * g["cbs"])[:2 * n]
            for r, w in enumerate(rows):
                branch = r // n
                want_tv[(w, branch)] = branch if g["pairing"] == "branch" else {"uc": 0, "c": 1}[text[r]]
                assert text[r] == ("uc", "c")[r % 2]
        else:
            want_tv.update({(w, 1): 1 for w in range(pos, pos + n)})
        pos += n
    assert p.unit_tv == want_tv
    assert p.bank_variants == sorted({tv for (w, br), tv in want_tv.items() if br == 1})
    # ReferenceNet groups
    assert p.T == reference_group_size(group, steps, world)
    assert [s for grp in p.groups for s in grp] == list(range(steps)) and all(1 <= len(grp) <= p.T for grp in p.groups)
    assert p.row_table == [((s // p.T) % 2) * p.T + s % p.T for s in range(steps)]


def _check_calls(g, p):
    seen = []
    for call in p.calls:
        brs = [br for _, br in call.units]
        assert 1 <= len(call.units) <= len(p.branches) * g["cbs"] and brs == sorted(brs)                # uncond units first
        assert call.n_uc == brs.count(0) and len(call.slots) == len(call.units)
        cond = [u for u in call.units if u[1] == 1]
        assert all(p.unit_tv[u] == call.bank_tv for u in cond) and (call.bank_tv is None) == (not cond)
        uc_w, c_w = [w for w, br in call.units if br == 0], [w for w, br in call.units if br == 1]
        assert call.halves_identical == (uc_w == c_w and len(uc_w) > 0)
        assert call.frames == [k for w, _ in call.units for k in p.windows[w]]
        seen += zip(call.units, call.slots)
    return seen


def test_loop_plan_over_the_sweep():
    n_run = 0
    for g in _geometries():
        for world, group, steps, emulate in itertools.product((1, 2, 3, 4, 8), (1, 2, 10), (2, 5), (False, True)):
            plans = [_plan(g, world, r, group, steps, emulate) for r in range(world)]      # (the window scheduler refuses none of these)
            n_run += world
            every = [(w, br) for br in ((0, 1) if g["cfg"] else (1,)) for w in range(len(plans[0].windows))]
            placed = {}
            for r, p in enumerate(plans):
                if r == 0:
                    _check_shared(g, p, steps, group, world)
                assert all(getattr(p, f) == getattr(plans[0], f) for f in SHARED)
                assert (p.dist, p.emulate, p.world_size) == (world > 1 and not emulate, emulate, world)
                assert p.rank == r and p.n_slots == -(-len(every) // world)
                # emulation: `units` is the rank's own share; otherwise every rank lists every unit, in one order
                assert p.units == (every[r::world] if emulate else every)
                mine = every[r::world]
                seen = _check_calls(g, p)
                assert sorted(u for u, _ in seen) == sorted(mine) and all(mine[slot] == u for u, slot in seen)
                assert p.cn_frames == sorted({k for u, _ in seen for k in p.windows[u[0]]})       # the frames the rank's ControlNet pass covers
                for u, slot in seen:
                    assert u not in placed
                    placed[u] = (r, slot)
            # global unit i sits at (rank i % world, slot i // world): the address _accumulate_all reads
            assert placed == {u: (i % world, i // world) for i, u in enumerate(every)}
    assert n_run == 5 * 2 * 2 * 3 * 2 * 2 * (1 + 2 + 3 + 4 + 8) * 3 * 2 * 2                    # nothing of the sweep is skipped


def test_loop_plan_refusals():
    with pytest.raises(ValueError, match="text_pairing must be 'reference' or 'branch'"):
        loop_plan(8, 2, 2, context_frames=4, context_overlap=0, text_pairing="both")
    with pytest.raises(ValueError, match="context_batch_size must be >= 1"):
        loop_plan(8, 2, 2, context_frames=4, context_overlap=0, context_batch_size=0)
    with pytest.raises(ValueError, match="_emulate_rank replaces dist=True"):
        loop_plan(8, 2, 2, context_frames=4, context_overlap=0, dist=True, world_size=2, _emulate_rank=(0, 2))
    with pytest.raises(ValueError, match="Unknown context_overlap policy"):
        loop_plan(8, 2, 2, context_frames=4, context_overlap=0, context_schedule="other")


# ------------------------------------------------------------------------------------------------ the table of clip inputs
BASE = dict(latents=torch.zeros(1, 4, 2, 2, 2), ref_image_latents=torch.zeros(1, 4, 2, 2), text_embeddings=torch.zeros(2, 1, 5),
            audio_features=torch.zeros(2, 3, 5), speed_embeddings=torch.zeros(1, 32), motion_latents=torch.zeros(2, 4, 2, 2),
            controlnet_cond=torch.zeros(2, 3, 16, 16), controlnet_conditioning_scale=1.0, guidance_scale=7.5, eta=0.0, seed=0,
            face_mask=torch.zeros(16, 16), face_mask_threshold=None)
# per record: (another value that leaves the plan alone, one that changes it - None where nothing of the input enters the plan)
OTHER = dict(controlnet_conditioning_scale=(None, 0.5), guidance_scale=(3.0, 1.0), eta=(0.5, None), seed=(7, None),
             face_mask=(torch.ones(2, 2), None), face_mask_threshold=(0.0, None))


def test_every_clip_input_enters_the_plan_key_as_its_record_says(monkeypatch):
    from emote_hack_amd import DDIMScheduler
    from tests.test_audio_io_host import _pipe
    p = _pipe(monkeypatch, {})
    p.scheduler = DDIMScheduler()

    def key(**change):
        kw = dict(BASE, **change)
        return p._plan_key(kw.pop("latents"), kw.pop("ref_image_latents"), kw.pop("text_embeddings"), kw)
    assert [r.name for r in CLIP_INPUTS] == list(BASE)
    base = key()
    for rec in CLIP_INPUTS:
        v = BASE[rec.name]
        same, changed = (v + 1, torch.zeros(*v.shape[:-1], v.shape[-1] + 1)) if rec.key == "shape" else OTHER[rec.name]
        if same is not None:
            assert key(**{rec.name: same}) == base, rec
        if rec.key is not None:      # (presence: `changed` is None, the input left out)
            assert key(**{rec.name: changed}) != base, rec
        else:
            assert changed is None, rec
    # a plan setting is no clip input: it enters by value
    assert key(context_frames=4) != base and key(context_frames=4) == key(context_frames=4)


def test_a_cache_hit_rebinds_and_bind_inputs_takes_the_tables_names(monkeypatch):
    from emote_hack_amd import DDIMScheduler
    from tests.test_audio_io_host import _pipe, _Stop
    p = _pipe(monkeypatch, {})
    p.scheduler = DDIMScheduler()
    names = [r.name for r in CLIP_INPUTS]
    bound = {}

    def bind(st, **kw):
        bound.update(kw, st=st)
        raise _Stop

    def hit(given):      # `denoise` itself (the stub pipeline replaces it), on a plan cache that holds this very plan
        given, bound["st"] = dict(given), None
        a = [given.pop(k) for k in ("latents", "ref_image_latents", "text_embeddings")]
        p._plan_cache, p._bind_inputs = (p._plan_key(*a, given), "the state"), bind
        with pytest.raises(_Stop):
            DenoiseLoop.denoise(p, *a, reuse_state=True, **given)
        assert bound.pop("st") == "the state"
        return dict(bound)
    assert sorted(hit(dict(BASE, face_mask_threshold=0.0))) == sorted(names)      # everything given is re-bound
    # nothing but the three required tensors given: guidance_scale / eta / seed mean their documented defaults, the rest stays bound
    bound.clear()
    lean = hit({k: BASE[k] for k in ("latents", "ref_image_latents", "text_embeddings")})
    assert {k: v for k, v in lean.items() if not torch.is_tensor(v)} == dict(guidance_scale=7.5, eta=0.0, seed=0)
    assert sorted(lean) == sorted(["latents", "ref_image_latents", "text_embeddings", "guidance_scale", "eta", "seed"])
    assert {r.name: r.hit for r in CLIP_INPUTS if r.hit is not None} == dict(guidance_scale=7.5, eta=0.0, seed=0)
    # _bind_inputs names no input of its own beyond the positional three, and refuses a name the table does not hold
    params = inspect.signature(DenoiseLoop._bind_inputs).parameters
    named = [k for k, v in params.items() if v.kind is not inspect.Parameter.VAR_KEYWORD and k not in ("self", "st")]
    assert set(named) <= set(names) and any(v.kind is inspect.Parameter.VAR_KEYWORD for v in params.values())
    with pytest.raises(TypeError, match="unexpected keyword argument 'context_frames'"):
        DenoiseLoop()._bind_inputs(None, BASE["latents"], context_frames=4)
