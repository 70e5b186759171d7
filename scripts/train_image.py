"""Fit one image with the image_hash.yaml field: the flow of app/image/main_image.py:53-100 with this package's classes -
ImageDataset (u8 bank on the GPU, fused sampling), HashGrid.from_geometric(blas=None), ImageNeuralField(hidden 64), ImageTrainer with
Adam (lr 1e-3, eps 1e-16, weight decay 1e-6), grid lr x 500 and the MultiStepLR schedule, validation (whole-image render, PSNR,
img_pred.png / img_gts.png) at the end.

    python scripts/train_image.py IMAGE [--epochs N] [--fused-step] [--fused-kernel] [--valid-metrics psnr [ssim]] [--log-dir DIR]
    python scripts/train_image.py --write-test-image PATH [--size H W] ...

--write-test-image PATH first writes a procedural RGB PNG to PATH and then fits it, so the script runs where no image exists.
--fused-step trains with ImageTrainStep (flat parameter buffer, single-launch optimizer, forward + backward replayed as a HIP
graph) instead of ImageTrainer's torch.optim loop; validation is ImageTrainer's in both cases.
--fused-kernel (implies --fused-step) builds ImageTrainStep(..., fused=True): forward + loss + backward run through
wisp_image_field_train_step (csrc/image_field_train.hip, two launches) instead of the modular ops under autograd.
The last line printed is one JSON record: PSNR after the first epoch and after training, seconds, ms per step, and
fused_image_step - whether the steps went through that kernel.  --valid-metrics psnr ssim also computes the structural
similarity of the final image (wisp.ops.image.ssim, on the GPU) and adds `ssim` to the record."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd")]


def procedural_image(h, w):
    """u8 [h, w, 3]: smooth waves, a disc with a hard edge and a fine checker band - low and high frequencies to fit."""
    ys, xs = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing='ij')
    img = np.stack([0.5 + 0.5 * np.sin(6 * xs + 2 * ys), 0.5 + 0.5 * np.cos(4 * ys), 0.5 + 0.5 * np.sin(5 * xs * ys)], -1)
    disc = (xs - 0.3) ** 2 + (ys + 0.2) ** 2 < 0.15
    img[disc] = img[disc] * 0.3 + np.array([0.7, 0.1, 0.1])
    band = np.abs(ys - 0.7) < 0.08
    checker = ((np.floor(xs * 24) + np.floor(ys * 24)) % 2).astype(bool)
    img[band & checker] = 1.0 - img[band & checker]
    return np.clip(img * 255.0, 0, 255).astype(np.uint8)


def build(image_path, device, num_pixels=4096, hidden_dim=64, codebook_bitwidth=19, num_lods=16, scaling_factor=2.0):
    """(dataset, pipeline) as main_image.py:57-71 builds them from image_hash.yaml."""
    from wisp.datasets import ImageDataset
    from wisp.models import Pipeline
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import ImageNeuralField
    ds = ImageDataset(image_path, num_pixels_per_image=num_pixels, device=device)
    max_grid_res = int(max(ds.h, ds.w) // scaling_factor)
    grid = HashGrid.from_geometric(blas=None, feature_dim=2, num_lods=num_lods, multiscale_type='cat', feature_std=1.0e-9,
                                   feature_bias=0.0, codebook_bitwidth=codebook_bitwidth, min_grid_res=16, max_grid_res=max_grid_res)
    nef = ImageNeuralField(grid, activation_type='relu', layer_type='linear', hidden_dim=hidden_dim, num_layers=1)
    return ds, Pipeline(nef=nef)


def trainer_config(epochs, enable_amp=True, valid_every=-1, valid_metrics=('psnr',)):
    from wisp.trainers import ConfigAdam, ConfigBaseTrainer
    return ConfigBaseTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-16, weight_decay=1e-6), exp_name='image-hash', max_epochs=epochs,
                             valid_every=valid_every, enable_amp=enable_amp, profile_nvtx=False, grid_lr_weight=500.0, scheduler=True,
                             valid_metrics=tuple(valid_metrics))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("image", nargs="?")
    ap.add_argument("--write-test-image", metavar="PATH")
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512), metavar=("H", "W"))
    ap.add_argument("--epochs", type=int, default=100, help="image_hash.yaml: 100 (of 100 steps each)")
    ap.add_argument("--num-pixels", type=int, default=4096)
    ap.add_argument("--hidden-dim", type=int, default=64)
    ap.add_argument("--codebook-bitwidth", type=int, default=19)
    ap.add_argument("--fused-step", action="store_true")
    ap.add_argument("--fused-kernel", action="store_true", help="ImageTrainStep(fused=True): the two-launch training kernel; implies --fused-step")
    ap.add_argument("--no-amp", action="store_true")
    ap.add_argument("--log-dir", default=os.path.join("_results", "logs", "runs", "image-hash"))
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--valid-metrics", nargs="+", choices=("psnr", "ssim"), default=["psnr"],
                    help="validation metrics (image_hash.yaml: psnr); ssim needs --device cuda")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if "psnr" not in args.valid_metrics:
        ap.error("--valid-metrics must name psnr (the record's psnr fields come from it)")
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    from wisp.ops.image import save_u8
    from wisp.trainers import ImageTrainer, ImageTrainStep
    from wisp.trainers.base_trainer import _Tracker
    path = args.image
    if args.write_test_image:
        path = args.write_test_image
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        save_u8(path, procedural_image(*args.size))
    if not path:
        ap.error("give an IMAGE or --write-test-image PATH")
    torch.manual_seed(args.seed)
    ds, pipeline = build(path, args.device, args.num_pixels, args.hidden_dim, args.codebook_bitwidth)
    trainer = ImageTrainer(trainer_config(args.epochs, enable_amp=not args.no_amp, valid_metrics=args.valid_metrics), pipeline, ds, tracker=_Tracker(args.log_dir),
                           device=args.device)
    steps_per_epoch = trainer.iterations_per_epoch
    total = steps_per_epoch * args.epochs
    t0 = time.time()
    fused_image_step = False
    if args.fused_step or args.fused_kernel:
        oc = trainer.cfg.optimizer
        step = ImageTrainStep(pipeline.nef, lr=oc.lr, eps=oc.eps, weight_decay=oc.weight_decay, grid_lr_weight=trainer.cfg.grid_lr_weight,
                              betas=oc.betas, optimizer='adam', fused=args.fused_kernel)
        fused_image_step = bool(args.fused_kernel and step._fused_field() is not None)
        step.set_schedule([total * x for x in trainer.cfg.scheduler_milestones], trainer.cfg.scheduler_gamma)
        step.capture(args.num_pixels)
        first = None
        for epoch in range(1, args.epochs + 1):
            running = torch.zeros((), device=args.device)
            for _ in range(steps_per_epoch):
                running += step.step(*ds[0])
            logging.info('EPOCH {}/{} | total loss: {:>.3E}'.format(epoch, args.epochs, float(running) / steps_per_epoch))
            if epoch == 1:
                torch.cuda.synchronize()
                t1 = time.time()
                first = trainer.validate()['psnr']
                t0 += time.time() - t1
    else:
        trainer.is_optimization_running = True
        first = None
        while trainer.is_optimization_running:
            trainer.iterate()
            if first is None and trainer.epoch >= 2 or (first is None and not trainer.is_optimization_running):
                torch.cuda.synchronize() if torch.cuda.is_available() else None
                t1 = time.time()
                first = trainer.validate()['psnr']
                t0 += time.time() - t1
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    seconds = time.time() - t0
    last = trainer.validate()
    final = last['psnr']
    extra = dict(ssim=float(last['ssim'])) if 'ssim' in last else {}
    print(json.dumps(dict(image=os.path.abspath(path), h=ds.h, w=ds.w, step="ImageTrainStep" if args.fused_step or args.fused_kernel else "ImageTrainer",
                          fused_image_step=fused_image_step,
                          epochs=args.epochs, steps=total, psnr_first_epoch=first, psnr=final, seconds=round(seconds, 3),
                          ms_per_step=round(1e3 * seconds / total, 4), log_dir=os.path.abspath(args.log_dir), **extra)))
    return final


if __name__ == "__main__":
    main()
