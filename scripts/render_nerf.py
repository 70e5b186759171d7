"""Render a trained radiance field to pictures: an orbit of look-at cameras on the training hemisphere, one rgb / depth / alpha PNG
per view, one JSON line with the timing.

    python scripts/render_nerf.py --checkpoint PATH [--views 8] [--res 800 800] [--render-batch 10000] --out DIR [--no-fused]
    python scripts/render_nerf.py --write-synlego DIR --steps K [--grid hash|octree|codebook|triplanar] [...] --out DIR

--checkpoint PATH is a file written by wisp.trainers.validation.save_pipeline: a 'full' checkpoint is the pipeline itself, a
state_dict checkpoint is loaded into the nerf_hash.yaml pipeline of scripts/train_nerf_synthetic.py (with --grid triplanar: into the
nerf_triplanar.yaml pipeline).  With --write-synlego DIR a
SynLego scene is written to DIR and fitted for K iterations first (the flow of train_nerf_synthetic.py), so the script runs where
neither a dataset nor a checkpoint exists.

The views are traced through wisp.trainers.validation.render with the tracer's `fused_query` on - lookup + decoder of every chunk
in one launch (csrc/nerf_query.hip), the same bits as the modular ops - unless --no-fused is given or the field is not one the
kernel covers (the JSON line reports which).

--grid octree / codebook (with --write-synlego) builds the field of nerf_octree.yaml / nerf_codebook.yaml instead - OctreeGrid or
4-bit CodebookOctreeGrid, 5 features, 4 LODs, 'sum', bias-free decoders, 'voxel' march with 16 steps - on an octree built from the
scene's surface point cloud; its views go through the one-launch query of csrc/nerf_octree_query.hip (`fused_octree_query` in the
JSON line).

--grid triplanar (with --write-synlego) builds the field of nerf_triplanar.yaml - an AxisAlignedBBoxAS, a TriplanarGrid of 4
features per plane, 4 LODs from 33 x 33 texels, 'sum', feature_std 0.01, hidden-64 decoders, 'voxel' march with 512 steps, white
background - and fits it with RMSprop at 1e-3 and grid_lr_weight 100 through the MultiviewTrainer the other grids use (it accepts
a triplanar field: the grid keeps its own `interpolate` inside the step).  Its views go through the one-launch query of
csrc/nerf_triplane_query.hip where WISP_NERF_TRIPLANE_QUERY_FUSED allows it.  `fused_query_route` in the JSON line names the route a
view took - "hash", "octree", "triplanar" or "modular" - next to the booleans `fused_query` (the hash route), `fused_octree_query`
and `fused_triplane_query`."""
import argparse
import json
import logging
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "scripts")]


def orbit_cameras(views, width, height, elevation_cos=0.5):
    """`views` LookAtCameras evenly spaced on the circle of the training hemisphere (synlego.cameras: radius CAMERA_RADIUS, y up)
    whose polar angle from +y has the cosine `elevation_cos`, looking at the origin with the training field of view."""
    import synlego
    from wisp.ops.raygen import LookAtCamera
    sin_phi = math.sqrt(1.0 - elevation_cos ** 2)
    cams = []
    for k in range(views):
        theta = 2.0 * math.pi * k / max(views, 1)
        eye = [synlego.CAMERA_RADIUS * sin_phi * math.cos(theta), synlego.CAMERA_RADIUS * elevation_cos,
               synlego.CAMERA_RADIUS * sin_phi * math.sin(theta)]
        cams.append(LookAtCamera(eye=eye, at=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0], fov=synlego.CAMERA_ANGLE_X, width=width,
                                 height=height, near=synlego.NEAR, far=synlego.FAR))
    return cams


def build_octree_pipeline(dev, kind, level, cloud_rays, bg_color=(0.0, 0.0, 0.0)):
    """nerf_octree.yaml (kind 'octree') / nerf_codebook.yaml (kind 'codebook'): the octree of the scene's surface point cloud (as
    bench_configs.vqad_scene builds it), F = 5, 4 LODs, 'sum', bias-free hidden-64 decoders, 'voxel' march with 16 steps."""
    import synlego
    from wisp.accelstructs import OctreeAS
    from wisp.models import Pipeline
    from wisp.models.grids import CodebookOctreeGrid, OctreeGrid
    from wisp.models.nefs import NeuralRadianceField
    from wisp.tracers import PackedRFTracer
    blas = OctreeAS.from_pointcloud(synlego.v8_pointcloud(cloud_rays, res=400, device=dev), level)
    shape = dict(feature_dim=5, num_lods=4, interpolation_type='linear', multiscale_type='sum', feature_std=0.01, feature_bias=0.0)
    grid = CodebookOctreeGrid(blas, codebook_bitwidth=4, **shape) if kind == "codebook" else OctreeGrid(blas, **shape)
    nef = NeuralRadianceField(grid, pos_embedder='none', view_embedder='positional', view_multires=4, activation_type='relu',
                              layer_type='linear', hidden_dim=64, num_layers=1, bias=False, prune_density_decay=None,
                              prune_min_density=None).to(dev)
    return Pipeline(nef, PackedRFTracer(raymarch_type='voxel', num_steps=16, step_size=1.0, bg_color=tuple(bg_color)))


def build_triplanar_pipeline(dev, num_steps=512, bg_color=(1.0, 1.0, 1.0)):
    """nerf_triplanar.yaml: an AABB, TriplanarGrid(4 features per plane, 4 LODs from 2^5 + 1 texels a side, 'sum', std 0.01), hidden-64
    decoders with the positional view embedding of 4 octaves, 'voxel' march with 512 steps, white background."""
    from wisp.accelstructs import AxisAlignedBBoxAS
    from wisp.models import Pipeline
    from wisp.models.grids import TriplanarGrid
    from wisp.models.nefs import NeuralRadianceField
    from wisp.tracers import PackedRFTracer
    grid = TriplanarGrid(AxisAlignedBBoxAS(), feature_dim=4, log_base_resolution=5, num_lods=4, interpolation_type='linear',
                         multiscale_type='sum', feature_std=0.01, feature_bias=0.0)
    nef = NeuralRadianceField(grid, pos_embedder='none', view_embedder='positional', view_multires=4, activation_type='relu',
                              layer_type='linear', hidden_dim=64, num_layers=1, prune_density_decay=None,
                              prune_min_density=None).to(dev)
    return Pipeline(nef, PackedRFTracer(raymarch_type='voxel', num_steps=num_steps, step_size=1.0, bg_color=tuple(bg_color)))


def fit_synlego(root, steps, dev, views=8, res=64, num_steps=512, num_samples=1024, grid="hash", octree_level=8,
                cloud_rays=1 << 21):
    """write a small SynLego scene to `root` and fit the nerf_hash.yaml pipeline (grid 'hash'), or the nerf_octree.yaml /
    nerf_codebook.yaml / nerf_triplanar.yaml one, to it for `steps` iterations"""
    from train_nerf_synthetic import build_pipeline, write_synlego_scene
    from wisp.datasets import SampleRays, load_multiview_dataset
    from wisp.trainers import ConfigAdamW, ConfigMultiviewTrainer, ConfigRMSprop, MultiviewTrainer
    write_synlego_scene(root, views=(views, 1, 1), res=res, device=dev)
    bg = (1.0, 1.0, 1.0) if grid == "triplanar" else (0.0, 0.0, 0.0)
    train = load_multiview_dataset(root, split='train', transform=SampleRays(num_samples), bg_color=bg, mip=0,
                                   dataset_num_workers=-1)
    torch.manual_seed(0)
    pipeline = (build_pipeline(dev, num_steps, (0.0, 0.0, 0.0)) if grid == "hash" else
                build_triplanar_pipeline(dev, num_steps) if grid == "triplanar" else
                build_octree_pipeline(dev, grid, octree_level, cloud_rays))
    epochs = max(1, -(-(steps + 1) // len(train)))                      # (the first iteration only sizes the batch)
    optimizer = (ConfigRMSprop(lr=1e-3) if grid == "triplanar" else ConfigAdamW(lr=1e-3, eps=1e-16, weight_decay=1e-6))
    cfg = ConfigMultiviewTrainer(optimizer=optimizer, grid_lr_weight=100.0 if grid == "triplanar" else 500.0, enable_amp=True,
                                 prune_every=100 if grid == "hash" else -1, rgb_loss_type='huber', rgb_loss_denom='rays', max_epochs=epochs, scheduler=True,
                                 valid_every=-1, save_every=-1, profile_nvtx=False)
    trainer = MultiviewTrainer(cfg, pipeline, train, device=dev)
    trainer.is_optimization_running = True
    while trainer.is_optimization_running and trainer.total_iterations <= steps:
        trainer.iterate()
    return pipeline


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", metavar="PATH", default=None, help="a file written by save_pipeline")
    ap.add_argument("--write-synlego", metavar="DIR", default=None, help="write a SynLego scene to DIR and fit it first")
    ap.add_argument("--steps", type=int, default=200, help="--write-synlego: training iterations")
    ap.add_argument("--train-views", type=int, default=8, help="--write-synlego: training views")
    ap.add_argument("--train-res", type=int, default=64, help="--write-synlego: side of the training images in pixels")
    ap.add_argument("--num-steps", type=int, default=512, help="raymarch steps of the pipeline this script builds")
    ap.add_argument("--views", type=int, default=8, help="frames to render")
    ap.add_argument("--res", type=int, nargs=2, default=(800, 800), metavar=("H", "W"))
    ap.add_argument("--render-batch", type=int, default=10000, help="rays per chunk")
    ap.add_argument("--out", metavar="DIR", required=True)
    ap.add_argument("--no-fused", action="store_true", help="leave the tracer's fused_query off (the modular ops)")
    ap.add_argument("--grid", choices=("hash", "octree", "codebook", "triplanar"), default="hash",
                    help="--write-synlego: the field to fit - nerf_hash.yaml, nerf_octree.yaml, nerf_codebook.yaml or nerf_triplanar.yaml")
    ap.add_argument("--octree-level", type=int, default=8, help="--grid octree / codebook: depth of the scene's octree")
    ap.add_argument("--cloud-rays", type=int, default=1 << 21, help="--grid octree / codebook: rays of the surface point cloud")
    args = ap.parse_args(argv)
    if (args.checkpoint is None) == (args.write_synlego is None):
        ap.error("give exactly one of --checkpoint PATH and --write-synlego DIR")
    if args.grid in ("octree", "codebook") and args.write_synlego is None:
        ap.error("--grid octree / codebook builds its field with --write-synlego (a 'full' checkpoint carries its own grid)")
    logging.basicConfig(level=logging.WARNING, format="%(message)s")
    assert torch.cuda.is_available(), "render_nerf.py renders on the GPU"
    dev = "cuda:0"
    from wisp.core import RenderBuffer
    from wisp.ops.image import write_png
    from wisp.ops.nerf_mlp import nerf_octree_query_supported, nerf_query_supported, nerf_triplane_query_supported
    from wisp.ops.raygen import generate_centered_pixel_coords, generate_pinhole_rays
    from wisp.trainers.validation import load_pipeline, render
    if args.checkpoint is not None:
        from collections.abc import Mapping
        obj = torch.load(args.checkpoint, map_location=dev, weights_only=False)
        if isinstance(obj, Mapping):
            from train_nerf_synthetic import build_pipeline
            base = build_triplanar_pipeline(dev, args.num_steps) if args.grid == "triplanar" else build_pipeline(dev, args.num_steps)
            pipeline = load_pipeline(args.checkpoint, base, map_location=dev)
        else:
            pipeline = obj
        pipeline = pipeline.to(dev)
    else:
        pipeline = fit_synlego(args.write_synlego, args.steps, dev, views=args.train_views, res=args.train_res, num_steps=args.num_steps,
                               grid=args.grid, octree_level=args.octree_level, cloud_rays=args.cloud_rays)
    pipeline.eval()
    h, w = args.res
    fused = not args.no_fused
    os.makedirs(args.out, exist_ok=True)
    times, samples = [], []
    for k, cam in enumerate(orbit_cameras(args.views, w, h)):
        grid = generate_centered_pixel_coords(w, h, device=dev)
        rays = generate_pinhole_rays(cam, grid).reshape(-1, 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = 0
        rb = RenderBuffer()
        for pack in (rays.split(args.render_batch) if args.render_batch > 0 else [rays]):
            rb += render(pipeline, pack, render_batch=-1, channels=["rgb", "depth", "alpha"], fused_query=fused)
            count += pipeline.tracer.get_prev_num_samples()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        samples.append(count)
        img = rb.reshape(h, w, -1).cpu().image().byte()
        write_png(os.path.join(args.out, f"rgb_{k:03d}.png"), img.rgb.numpy())
        write_png(os.path.join(args.out, f"depth_{k:03d}.png"), img.depth.numpy())
        write_png(os.path.join(args.out, f"alpha_{k:03d}.png"), img.alpha.numpy())
    grid_ = pipeline.nef.grid
    with torch.no_grad():
        took_fused = bool(fused and nerf_query_supported(pipeline.nef))
        took_octree = bool(fused and not took_fused and nerf_octree_query_supported(pipeline.nef))
        took_triplane = bool(fused and not took_fused and not took_octree and nerf_triplane_query_supported(pipeline.nef))
    route = "hash" if took_fused else "octree" if took_octree else "triplanar" if took_triplane else "modular"
    print(json.dumps(dict(metric="render_nerf", frames=len(times), res=[h, w], render_batch=args.render_batch,
                          ms_per_frame=round(sum(times) / max(len(times), 1), 3),
                          samples_per_frame=int(sum(samples) / max(len(samples), 1)), fused_query=took_fused,
                          grid=args.grid, fused_octree_query=took_octree, fused_triplane_query=took_triplane,
                          fused_query_route=route,
                          field=dict(grid=type(grid_).__name__, num_lods=int(getattr(grid_, "num_lods", 0)),
                                     feature_dim=int(getattr(grid_, "feature_dim", 0)),
                                     codebook_bitwidth=int(getattr(grid_, "codebook_bitwidth", getattr(grid_, "bitwidth", 0))),
                                     multiscale_type=getattr(grid_, "multiscale_type", None),
                                     hidden_dim=int(pipeline.nef.hidden_dim)))))


if __name__ == "__main__":
    main()
