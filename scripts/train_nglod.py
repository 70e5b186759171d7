"""Fit a signed distance field to an OBJ and look at the result: the flow of app/nglod/main_nglod.py with this package's classes -
OctreeAS.from_mesh, OctreeGrid, NeuralSDF, a mesh SDF dataset, SDFTrainer with its IoU validation - then an OfflineRenderer
snapshot (render.png) and the three axis-aligned distance cross-sections (slice_x.png, slice_y.png, slice_z.png).

    python scripts/train_nglod.py OBJ [--epochs N] [--dataset octree|mesh] [--grid octree|hash|triplanar] [--fused-step]
                                  [--fused-kernel] [--all-lods] [--out-dir DIR]
    python scripts/train_nglod.py --write-test-mesh DIR ...

--write-test-mesh DIR first writes the procedural torus of scripts/train_sdf_tex.py into DIR and fits that.
--fused-step trains with SDFTrainStep (flat parameter buffer, single-launch optimizer, fused forward + loss + backward, replayed
as a HIP graph for whole batches) instead of SDFTrainer's torch.optim loop; validation is SDFTrainer.validate either way.
--grid hash fits the field of nglod_hash.yaml instead: HashGrid.from_geometric, 'cat', 4 levels x 8 features between resolutions
16 and 2048, tables of 2^19 rows (--codebook-bitwidth for smaller ones).  Validation, the snapshot and the slices then run through
the kernels of csrc/hash_sdf_eval.hip, and --fused-step trains through wisp_hash_sdf_train_step (csrc/hash_sdf_train.hip:
SDFTrainStep(..., fused_hash=True)), replayed as a HIP graph like the octree step; the JSON record's fused_hash_step says whether
the field took that branch.
--grid triplanar fits the field of nglod_triplanar.yaml: AxisAlignedBBoxAS, TriplanarGrid of one level of three 4 x 33 x 33
planes, 'sum', and the configuration's MeshSampledSDFDataset (--dataset mesh is implied).  Validation, the snapshot and the slices
run through the kernels of csrc/triplane_sdf_eval.hip; the JSON record's fused_triplane_eval says whether the field took them.
--fused-kernel (with --grid triplanar only) trains this field through wisp_triplane_sdf_train_step (csrc/triplane_sdf_train.hip:
SDFTrainStep(..., fused_triplane=True)), replayed as a HIP graph for whole batches; the JSON record's fused_triplane_step says
whether the field took that branch.  --grid triplanar --fused-step stays refused.
--all-lods takes the loss over every level of detail (only_last=False, the reference's default): the field then means something at
every lod_idx, not at the finest alone.  With --fused-step the octree field trains through wisp_sdf_lods_train_step (csrc/spc_grad.hip:
SDFTrainStep(..., only_last=False, fused_lods=True)), replayed as a HIP graph; the JSON record's fused_lods_step says whether the field
took it.  There is no all-LOD fused step over a hash or triplanar grid: --all-lods with one of them and a fused option is refused.
The record's iou_lods_before / iou_lods_after hold the IoU of every LOD, whatever the loss was taken over.
The last line printed is one JSON record with the IoU before and after training."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "scripts")]


def build(obj, device, level=6, dataset="octree", num_samples=100000, samples_per_voxel=16, num_lods=4, hidden_dim=128,
          num_samples_on_mesh=2_000_000, grid_type="octree", codebook_bitwidth=19):
    """(dataset, pipeline) as main_nglod.py builds them from nglod_octree.yaml (grid_type 'octree'), nglod_hash.yaml ('hash') or
    nglod_triplanar.yaml ('triplanar')."""
    from wisp.accelstructs import AxisAlignedBBoxAS, OctreeAS
    from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset
    from wisp.models import Pipeline
    from wisp.models.grids import HashGrid, OctreeGrid, TriplanarGrid
    from wisp.models.nefs import NeuralSDF
    from wisp.tracers import PackedSDFTracer
    if grid_type == "triplanar":
        ds = MeshSampledSDFDataset(obj, split='train', num_samples=max(num_samples // 5, 1))
        grid = TriplanarGrid(AxisAlignedBBoxAS(), feature_dim=4, log_base_resolution=5, num_lods=1, multiscale_type='sum',
                             feature_std=0.01)
        nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=hidden_dim, num_layers=1).to(device)
        return ds, Pipeline(nef, PackedSDFTracer(num_steps=128, step_size=0.8, min_dis=0.0003))
    blas = OctreeAS.from_mesh(obj, level=level, num_samples_on_mesh=num_samples_on_mesh)
    if dataset == "octree":
        ds = OctreeSampledSDFDataset(blas, split='train', num_samples=num_samples, samples_per_voxel=samples_per_voxel)
    else:
        ds = MeshSampledSDFDataset(obj, split='train', num_samples=max(num_samples // 5, 1))
    if grid_type == "hash":
        grid = HashGrid.from_geometric(blas, feature_dim=8, num_lods=num_lods, multiscale_type='cat', feature_std=0.01,
                                       codebook_bitwidth=codebook_bitwidth, min_grid_res=16, max_grid_res=2048)
    else:
        grid = OctreeGrid(blas, feature_dim=16, num_lods=num_lods, multiscale_type='sum', feature_std=0.01)
    nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=hidden_dim, num_layers=1).to(device)
    return ds, Pipeline(nef, PackedSDFTracer(num_steps=128, step_size=0.8, min_dis=0.0003))


def fit_fused(trainer, ds, cfg, device, fused_triplane=False, fused_lods=False):
    """SDFTrainer's epochs with SDFTrainStep: shuffled batches of cfg.dataloader.batch_size, resampling after every epoch.  Returns
    whether the field took its opt-in fused step (the hash one, with fused_triplane the triplanar one, with fused_lods the all-LOD
    octree one)."""
    from wisp.trainers import SDFTrainStep
    oc, bs = cfg.optimizer, cfg.dataloader.batch_size
    nef = trainer.pipeline.nef
    from wisp.models.grids import HashGrid, OctreeGrid
    step = SDFTrainStep(nef, lr=oc.lr, eps=oc.eps, grid_lr_weight=cfg.grid_lr_weight, betas=oc.betas, optimizer='adam',
                        only_last=cfg.only_last, fused_hash=type(nef.grid) is HashGrid, fused_triplane=bool(fused_triplane),
                        fused_lods=bool(fused_lods))
    on_gpu = torch.device(device).type == 'cuda'
    took_opt_in = bool(on_gpu and (step.fused_hash or fused_triplane or fused_lods) and step._fused_field() is not None)
    if fused_lods:
        took_opt_in = bool(took_opt_in and step._fused_field().get("lods_loss"))
    if on_gpu and len(ds) >= bs and (type(nef.grid) is OctreeGrid or took_opt_in):
        step.capture(bs)
    nef.train()
    for epoch in range(cfg.max_epochs):
        coords, sdf = ds.data["coords"].to(device), ds.data["sdf"].to(device)
        order = torch.randperm(coords.shape[0], device=coords.device)
        total = torch.zeros((), device=coords.device)
        for a in range(0, order.shape[0], bs):
            pick = order[a:a + bs]
            total = total + step.step(coords[pick], sdf[pick].reshape(-1, 1)) * pick.shape[0]
        logging.info('EPOCH {}/{} | l2 loss: {:>.3E}'.format(epoch + 1, cfg.max_epochs, float(total) / order.shape[0]))
        if cfg.resample:
            ds.resample()
            trainer.init_dataloader()
    nef.eval()
    return took_opt_in


def validate_every_lod(trainer):
    """SDFTrainer.validate over every LOD of the field, whatever the loss is taken over: {metric: [mean IoU per LOD]} - the last
    entry is the finest LOD's, the figure validate() gives with only_last"""
    saved = getattr(trainer, "loss_lods", None)
    trainer.loss_lods = list(range(trainer.pipeline.nef.grid.num_lods))
    try:
        return trainer.validate()
    finally:
        if saved is None:
            del trainer.loss_lods
        else:
            trainer.loss_lods = saved


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter,
                                 epilog="--grid {octree,hash} take either --dataset and --fused-step;\n"
                                        "--grid triplanar implies --dataset mesh, refuses --fused-step and takes --fused-kernel.")
    ap.add_argument("obj", nargs="?")
    ap.add_argument("--write-test-mesh", metavar="DIR")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--dataset", choices=("octree", "mesh"), default="octree")
    ap.add_argument("--grid", choices=("octree", "hash", "triplanar"), default="octree",
                    help="feature grid: nglod_octree.yaml, nglod_hash.yaml or nglod_triplanar.yaml")
    ap.add_argument("--codebook-bitwidth", type=int, default=19, help="--grid hash: the hashed levels have 2^N rows")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--num-lods", type=int, default=4)
    ap.add_argument("--num-samples", type=int, default=100000)
    ap.add_argument("--mesh-samples", type=int, default=2_000_000, help="surface samples the occupancy octree is built from")
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--fused-step", action="store_true")
    ap.add_argument("--fused-kernel", action="store_true",
                    help="--grid triplanar only: train through the kernel-fused step (wisp_triplane_sdf_train_step)")
    ap.add_argument("--all-lods", action="store_true",
                    help="loss over every level of detail (only_last=False); with --fused-step: the fused all-LOD octree step")
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("W", "H"))
    ap.add_argument("--shading-mode", choices=("rb", "normal", "matcap"), default="normal")
    ap.add_argument("--matcap-path", default=None)
    ap.add_argument("--out-dir", default=os.path.join("_results", "nglod"))
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if args.grid == "triplanar":
        if args.fused_step:
            ap.error("--grid triplanar has no fused training step: drop --fused-step")
        args.dataset = "mesh"
    elif args.fused_kernel:
        ap.error("--fused-kernel is the triplanar field's fused step: use it with --grid triplanar (--grid hash: --fused-step)")
    if args.all_lods and args.grid != "octree" and (args.fused_step or args.fused_kernel):
        ap.error(f"--all-lods has no fused step over a {args.grid} grid (the all-LOD step is the octree fields'): "
                 "drop --all-lods, or drop --fused-step / --fused-kernel to train through the modular launches")
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    from wisp.ops.image import save_u8
    from wisp.trainers import ConfigAdam, ConfigDataloader, ConfigSDFTrainer, SDFTrainer
    from wisp.trainers.tracker import OfflineRenderer
    obj = args.obj
    if args.write_test_mesh:
        from train_sdf_tex import write_test_mesh
        obj = write_test_mesh(args.write_test_mesh)
    if not obj:
        ap.error("give an OBJ or --write-test-mesh DIR")
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    ds, pipeline = build(obj, args.device, level=args.level, dataset=args.dataset, num_samples=args.num_samples,
                         num_lods=args.num_lods, num_samples_on_mesh=args.mesh_samples, grid_type=args.grid,
                         codebook_bitwidth=args.codebook_bitwidth)
    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=args.batch_size),
                           max_epochs=args.epochs, resample=True, only_last=not args.all_lods, exp_name='nglod', profile_nvtx=False,
                           valid_every=-1)
    trainer = SDFTrainer(cfg, pipeline, ds, device=args.device)
    from wisp.ops.sdf import fused_sdf_field
    fld = fused_sdf_field(pipeline.nef) if torch.device(args.device).type == 'cuda' else None
    fused_triplane_eval = bool(args.grid == "triplanar" and fld is not None and fld.get("kind") == "triplane")
    before = validate_every_lod(trainer)
    metric = next(iter(before))
    t0 = time.time()
    fused_hash_step = fused_triplane_step = fused_lods_step = False
    if args.fused_step and args.all_lods:
        fused_lods_step = fit_fused(trainer, ds, cfg, args.device, fused_lods=True)
    elif args.fused_kernel:
        fused_triplane_step = fit_fused(trainer, ds, cfg, args.device, fused_triplane=True)
    elif args.fused_step:
        fused_hash_step = fit_fused(trainer, ds, cfg, args.device)
    else:
        trainer.train()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    seconds = time.time() - t0
    pipeline.eval()
    after = validate_every_lod(trainer)
    os.makedirs(args.out_dir, exist_ok=True)
    renderer = OfflineRenderer(render_res=tuple(args.size), shading_mode=args.shading_mode,
                               matcap_path=args.matcap_path or './data/matcap/Pearl.png', device=args.device)
    rb = renderer.render_snapshot(pipeline, f=[1.4, 1.2, 1.6], t=[0, 0, 0], fov=40.0, camera_clamp=[0, 6])
    shot = rb.transpose()                                   # back to [height, width, .]
    img = torch.where(shot.hit.bool().reshape(*shot.rgb.shape[:2], 1), shot.rgb[..., :3], torch.ones_like(shot.rgb[..., :3]))
    files = dict(render=os.path.join(args.out_dir, "render.png"))
    save_u8(files["render"], (img.clamp(0, 1) * 255).round().to(torch.uint8).numpy())
    for axis, name in enumerate("xyz"):
        files[f"slice_{name}"] = os.path.join(args.out_dir, f"slice_{name}.png")
        vis = renderer.sdf_slice(pipeline.nef, dim=axis)
        save_u8(files[f"slice_{name}"], (np.clip(vis, 0, 1) * 255).round().astype(np.uint8).transpose(1, 0, 2))
    rec = dict(obj=os.path.abspath(obj), dataset=args.dataset, grid=args.grid, samples=len(ds), epochs=args.epochs, fused_step=bool(args.fused_step),
               fused_hash_step=fused_hash_step, fused_triplane_eval=fused_triplane_eval, fused_triplane_step=fused_triplane_step,
               all_lods=bool(args.all_lods), fused_lods_step=fused_lods_step, iou_lods_before=list(before[metric]),
               iou_lods_after=list(after[metric]), metric=metric, iou_before=before[metric][-1], iou_after=after[metric][-1], hits=int(shot.hit.sum()),
               seconds=round(seconds, 3), **{k: os.path.abspath(v) for k, v in files.items()})
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
