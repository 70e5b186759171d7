"""Samples per ray of a headline batch: bench.py's pipeline, its untimed pre-training (300 steps, prune every 100), then ONE batch of
the timed region's ray count marched on its own; offsets[1:] - offsets[:-1] as a histogram.
usage: python scripts/ray_length_hist.py OUT.json [--pretrain N]"""
import json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import bench, synlego
from wisp.core import Rays
from wisp.trainers import MultiviewTrainStep

out = sys.argv[1]
args = bench.parse(sys.argv[2:])
dev = torch.device("cuda:0")
pipe = bench.build_pipeline(dev, args.hidden, args.num_steps, bench._initial_cells(args, dev, synlego.occupied_cells(7, device=dev)))
trainer = MultiviewTrainStep(pipe, lr=1e-3, eps=1e-16, weight_decay=1e-6, grid_lr_weight=500.0, rgb_loss_type='huber', prune_every=100,
                             target_sample_size=args.target_samples, max_rays=2 ** 18, enable_amp=args.precision == "bf16")
bank_o, bank_d, bank_rgb = synlego.ray_bank(args.bank_rays, seed=1000, device=dev)
gen = torch.Generator(device=dev).manual_seed(1234)


def batch(n):
    idx = torch.randint(0, bank_o.shape[0], (n,), device=dev, generator=gen)
    o, d, rgb = bench._gather_rows(idx, [bank_o, bank_d, bank_rgb])
    return Rays(o, d, dist_min=synlego.NEAR, dist_max=synlego.FAR), rgb


def size_batch():
    probe, _ = batch(4096)
    pipe.tracer.prev_num_samples = bench._probe_samples(pipe, probe, args.num_steps)
    return max(int(trainer.calc_adaptive_rays(4096)), 256)


R = size_batch()
for _ in range(args.pretrain):
    rays, gts = batch(R)
    trainer.step(rays, gts)
    R = max(int(trainer.num_rays), 256)
R = size_batch()
rays, _ = batch(R)
grid = pipe.nef.grid
ridx = grid.raymarch(rays, level=grid.active_lods[-1], num_samples=args.num_steps, raymarch_type='ray').ridx
lens = torch.bincount(ridx.long(), minlength=R)
S = int(lens.sum())
hist = torch.bincount(lens).tolist()
share = lambda n: float((lens > n).double().mean())
weight = lambda n: float(lens[lens > n].sum()) / max(S, 1)
res = {"rays": R, "samples": S, "mean": S / R, "max": int(lens.max()), "pretrain_steps": args.pretrain, "candidates_per_ray": args.num_steps,
       "share_of_rays_above": {str(n): share(n) for n in (0, 64, 128, 256, 512)},
       "share_of_samples_on_rays_above": {str(n): weight(n) for n in (64, 128, 256, 512)},
       "histogram_rays_by_length": hist}
with open(out, "w") as f:
    json.dump(res, f)
print({k: v for k, v in res.items() if k != "histogram_rays_by_length"})
