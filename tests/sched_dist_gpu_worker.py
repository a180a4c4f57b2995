"""Worker of tests/test_gpu_schedulers_dist.py: one rank of a world_size 2 run of the product loop with a sigma-space sampler
(ranks share cuda:0 and exchange through gloo, like tests/dist_gpu_worker.py).  Every rank steps redundantly on the gathered eps, so
the latents - and the model-output history ring behind them - must be bit-identical on all ranks, and equal the single-process loop."""
import os
import sys

import torch
import torch.distributed as td

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    name, graphs = sys.argv[1], sys.argv[2] == "1"
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    td.init_process_group("gloo")
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    from tests.test_gpu_schedulers_loop import KW, STEPS, _inputs, _models, _product
    ref, unet = _models()
    sch = _product(name)
    sch.set_timesteps(STEPS)
    lat0, refl, text = _inputs(sch.init_noise_sigma)
    kw = dict(KW, appearance_encoder=ref, num_inference_steps=STEPS, use_graphs=graphs, reference_group=2)
    lat = EMOAnimationPipeline(unet=unet, scheduler=sch).denoise(lat0.to("cuda"), refl, text, dist=True, rank=rank, world_size=world, **kw)
    torch.cuda.synchronize()
    all_l = torch.zeros(world, lat.numel(), device="cuda")
    td.all_gather_into_tensor(all_l.view(-1), lat.reshape(-1).contiguous())
    for r in range(world):
        assert torch.equal(all_l[r], all_l[0]), f"rank {r} differs"
    if rank == 0:
        single = EMOAnimationPipeline(unet=unet, scheduler=_product(name)).denoise(lat0.to("cuda"), refl, text, **kw)
        torch.cuda.synchronize()
        diff = float((lat - single).abs().max())
        # the ranks batch their UNet calls and ReferenceNet timesteps differently from one process: equal at the loop tolerance
        torch.testing.assert_close(lat.cpu(), single.cpu(), rtol=1e-3, atol=1e-4)
        print(f"SCHED_DIST_OK {name} world={world} backend={td.get_backend()} max diff to one process {diff:.3e} "
              f"bit-identical={torch.equal(lat, single)}", flush=True)
    td.barrier()
    td.destroy_process_group()


if __name__ == "__main__":
    main()
