"""Train the nerf_hash.yaml pipeline on a NeRF-synthetic style dataset on disk (transforms*.json + images): the flow of
app/nerf/main_nerf.py:74-116 with this package's classes - NeRFSyntheticDataset + SampleRays, create_split for validation, the
nerf_hash.yaml pipeline, MultiviewTrainer, validation PSNR.

    python scripts/train_nerf_synthetic.py DATASET_DIR [--epochs N] [--mip M] [--valid-split val] [--valid-metrics psnr [ssim]]
    python scripts/train_nerf_synthetic.py --write-synlego DIR [--views 100] [--res 800]

With --write-synlego DIR a SynLego scene (synlego.py's analytic brick assembly) is first written to DIR in the NeRF-synthetic
layout - transforms_{train,val,test}.json + RGBA PNGs, Blender's z-up world - and then trained on, so the script runs where no
dataset exists.  `write_synlego_scene` is also what the tests build their fixtures with."""
import argparse
import json
import logging
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd")]


@torch.no_grad()
def _render_alpha(origins, dirs, steps=768, chunk=1 << 16):
    """sum of the quadrature weights of synlego.render_gt (same nodes, same weights): the opacity of every ray."""
    import synlego
    out = []
    for s in range(0, origins.shape[0], chunk):
        o, d = origins[s:s + chunk], dirs[s:s + chunk]
        t = torch.linspace(synlego.NEAR, synlego.FAR, steps + 1, device=o.device)
        tm = 0.5 * (t[1:] + t[:-1])
        tau = synlego.density(o[:, None, :] + d[:, None, :] * tm[None, :, None]) * (t[1] - t[0])
        T = torch.exp(-(torch.cumsum(tau, 1) - tau))
        out.append((T * (1 - torch.exp(-tau))).sum(1))
    return torch.cat(out, 0)


def write_synlego_scene(root, views=(100, 8, 8), res=800, seed=0, device='cpu', rgba=True, steps=768):
    """Write SynLego to `root` as NeRF-synthetic files: transforms_train / _val / _test.json with `views` = (train, val, test)
    frames each and <split>/r_<i>.png (RGBA: straight colour + opacity; rgba=False: RGB over black).  The files use Blender's
    world (z up) and camera (looks down -z, y up) like the original data; camera positions are stored times 1.25 because the
    loader divides translations by aabb_scale = 1.25.  Returns the list of transform files."""
    import synlego
    from wisp.ops.image import save_u8
    os.makedirs(root, exist_ok=True)
    to_file = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])       # (x, y, z) y-up -> (x, -z, y) z-up
    py, px = torch.meshgrid(torch.arange(res), torch.arange(res), indexing='ij')
    py, px = py.reshape(-1).to(device), px.reshape(-1).to(device)
    written = []
    for k, (split, count) in enumerate(zip(('train', 'val', 'test'), views)):
        rot, pos = synlego.cameras(count, seed=seed + 7 * k)
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i in range(count):
            vi = torch.full((res * res,), i, dtype=torch.long, device=device)
            o, d = synlego.pixel_rays(rot.to(device), pos.to(device), vi, px, py, res)
            rgb = synlego.render_gt(o, d, steps=steps)
            if rgba:
                a = _render_alpha(o, d, steps=steps).clamp(0.0, 1.0)[:, None]
                straight = torch.where(a > 1e-6, rgb / a.clamp_min(1e-6), torch.zeros_like(rgb)).clamp(0.0, 1.0)
                img = torch.cat([straight, a], 1)
            else:
                img = rgb.clamp(0.0, 1.0)
            img = (img * 255.0).round().to(torch.uint8).reshape(res, res, -1).cpu().numpy()
            save_u8(os.path.join(root, split, f"r_{i}.png"), img)
            c2w = np.eye(4)
            r = rot[i].double().numpy()
            c2w[:3, :3] = to_file @ np.stack([r[:, 0], r[:, 1], -r[:, 2]], 1)      # OpenGL camera: right, up, backward
            c2w[:3, 3] = to_file @ (pos[i].double().numpy() * 1.25)
            frames.append(dict(file_path=f"./{split}/r_{i}", transform_matrix=c2w.tolist()))
        path = os.path.join(root, f"transforms_{split}.json")
        with open(path, "w") as f:
            json.dump(dict(camera_angle_x=synlego.CAMERA_ANGLE_X, frames=frames), f)
        written.append(path)
    return written


def build_pipeline(device, num_steps=2048, bg_color=(0.0, 0.0, 0.0)):
    """nerf_hash.yaml: dense level-7 OctreeAS, 16-level 'cat' HashGrid, NeuralRadianceField, PackedRFTracer."""
    from wisp.accelstructs import OctreeAS
    from wisp.models import Pipeline
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralRadianceField
    from wisp.tracers import PackedRFTracer
    blas = OctreeAS.make_dense(level=7)
    grid = HashGrid.from_geometric(blas, feature_dim=2, num_lods=16, multiscale_type='cat', feature_std=1e-9, codebook_bitwidth=19,
                                   min_grid_res=16, max_grid_res=512)
    nef = NeuralRadianceField(grid, pos_embedder='none', view_embedder='positional', view_multires=4, activation_type='relu',
                              layer_type='linear', hidden_dim=64, num_layers=1, bias=True, prune_density_decay=0.95,
                              prune_min_density=(0.01 * 512) / (2 * math.sqrt(3))).to(device)
    return Pipeline(nef, PackedRFTracer(raymarch_type='ray', num_steps=num_steps, step_size=1.0, bg_color=tuple(bg_color)))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dataset_dir", nargs="?", help="dataset root (transforms*.json + images)")
    ap.add_argument("--write-synlego", metavar="DIR", default=None, help="write a SynLego scene to DIR first and train on it")
    ap.add_argument("--views", type=int, default=100, help="--write-synlego: training views (8 more each for val and test)")
    ap.add_argument("--res", type=int, default=800, help="--write-synlego: image side in pixels")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--mip", type=int, default=0)
    ap.add_argument("--num-workers", type=int, default=-1, help="image decoding processes (dataset_num_workers)")
    ap.add_argument("--num-samples", type=int, default=4096, help="rays per batch before the adaptive count takes over")
    ap.add_argument("--num-steps", type=int, default=2048, help="raymarch steps (nerf_hash.yaml: 2048)")
    ap.add_argument("--valid-split", default="val")
    ap.add_argument("--bg", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--valid-metrics", nargs="+", choices=("psnr", "ssim"), default=["psnr"],
                    help="validation metrics (nerf_hash.yaml: psnr); with ssim the record carries the views' mean SSIM too")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if "psnr" not in args.valid_metrics:
        ap.error("--valid-metrics must name psnr (the record's psnr comes from it)")
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    assert torch.cuda.is_available(), "train_nerf_synthetic.py trains on the GPU"
    dev = "cuda:0"
    root = args.dataset_dir
    if args.write_synlego:
        root = args.write_synlego
        t0 = time.perf_counter()
        write_synlego_scene(root, views=(args.views, 8, 8), res=args.res, device=dev)
        print(f"wrote SynLego ({args.views} + 8 + 8 views of {args.res} x {args.res}) to {root} in {time.perf_counter() - t0:.1f}s")
    if not root:
        ap.error("give DATASET_DIR or --write-synlego DIR")
    from wisp.datasets import SampleRays, load_multiview_dataset
    from wisp.trainers import ConfigAdamW, ConfigMultiviewTrainer, MultiviewTrainer
    t0 = time.perf_counter()
    train = load_multiview_dataset(root, split='train', transform=SampleRays(args.num_samples), bg_color=tuple(args.bg), mip=args.mip,
                                   dataset_num_workers=args.num_workers)
    print(f"{type(train).__name__}: {len(train)} views of {tuple(train.img_shape)}, {train.device_bytes() / 2 ** 20:.1f} MiB on the "
          f"device, loaded in {time.perf_counter() - t0:.1f}s")
    valid = train.create_split(split=args.valid_split, transform=None)
    torch.manual_seed(0)
    pipeline = build_pipeline(dev, args.num_steps, args.bg)
    cfg = ConfigMultiviewTrainer(optimizer=ConfigAdamW(lr=1e-3, eps=1e-16, weight_decay=1e-6), grid_lr_weight=500.0, enable_amp=True,
                                 prune_every=100, rgb_loss_type='huber', rgb_loss_denom='rays', max_epochs=args.epochs, scheduler=True,
                                 valid_every=-1, save_every=-1, profile_nvtx=False, valid_metrics=tuple(args.valid_metrics))
    trainer = MultiviewTrainer(cfg, pipeline, train, validation_dataset=valid, device=dev)
    t0 = time.perf_counter()
    trainer.train()
    torch.cuda.synchronize()
    print(f"trained {args.epochs} epochs ({trainer.total_iterations} iterations) in {time.perf_counter() - t0:.1f}s")
    result = trainer.validate()
    extra = dict(ssim=float(result["ssim"])) if "ssim" in result else {}
    print(json.dumps(dict(metric="train_nerf_synthetic", views=len(train), epochs=args.epochs, psnr=float(result["psnr"]), **extra)))


if __name__ == "__main__":
    main()
