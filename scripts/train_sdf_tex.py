"""Fit a signed distance field with surface colour to a textured OBJ: the flow of app/nglod/main_nglod.py with `sample_tex: True`
and this package's classes - OctreeAS.from_mesh(sample_tex=True), OctreeGrid, NeuralSDFTex, a mesh dataset whose `rgb` comes from
wisp.ops.mesh.closest_tex, SDFTrainer (Adam, resampling every epoch).  Then one view is sphere-traced with PackedSDFTracer and
the colour of the field at the hits, nef(coords=rb.xyz[rb.hit], channels="rgb"), is written to albedo.png.

    python scripts/train_sdf_tex.py OBJ [--epochs N] [--dataset octree|mesh] [--fused-step] [--out-dir DIR]
    python scripts/train_sdf_tex.py --write-test-mesh DIR ...

--write-test-mesh DIR first writes a procedural textured torus (torus.obj + torus.mtl + stripes.png + checker.png: three materials -
a striped RGB map, a plain diffuse colour, a checker RGBA map) into DIR and then fits it, so the script runs where no asset exists.
--fused-step trains with SDFTrainStep (flat parameter buffer, single-launch optimizer, forward + loss + backward of a batch as the
fused four-launch step, replayed as a HIP graph for whole batches) instead of SDFTrainer's torch.optim loop: same batches per epoch,
same resampling, the same two per-sample means.
The last line printed is one JSON record: losses of the first and the last epoch, hit count, seconds."""
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


def write_test_mesh(folder, nu=48, nv=24, R=0.6, r=0.25):
    """Procedural textured torus -> path of torus.obj.  Quad (i, j) of the (u, v) grid gets the UV square [i/nu, (i+1)/nu] x
    [j/nv, (j+1)/nv] scaled by (2, 1), so u runs to 2 (reflection padding mirrors the map once around the ring); the material
    changes with the third of the tube the quad lies in."""
    from wisp.ops.image import save_u8
    os.makedirs(folder, exist_ok=True)
    ys, xs = np.meshgrid(np.arange(64), np.arange(128), indexing='ij')
    stripes = np.stack([128 + 120 * np.sin(xs / 128 * 8 * np.pi), 40 + 3 * ys, 255 - 1.5 * xs], -1)
    save_u8(os.path.join(folder, "stripes.png"), np.clip(stripes, 0, 255).astype(np.uint8))
    checker = (((xs[:32, :32] // 4) + (ys[:32, :32] // 4)) % 2)[..., None] * np.array([200, 180, 40]) + 30
    save_u8(os.path.join(folder, "checker.png"), np.concatenate([checker, np.full((32, 32, 1), 255)], -1).astype(np.uint8))
    with open(os.path.join(folder, "torus.mtl"), "w") as f:
        f.write("newmtl striped\nKd 1 1 1\nmap_Kd stripes.png\n\nnewmtl plain\nKd 0.2 0.4 0.8\n\nnewmtl checked\nKd 1 1 1\nmap_Kd checker.png\n")
    u, v = np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv
    with open(os.path.join(folder, "torus.obj"), "w") as f:
        f.write("mtllib torus.mtl\n")
        for a in u:
            for b in v:
                f.write(f"v {float((R + r * np.cos(b)) * np.cos(a))!r} {float((R + r * np.cos(b)) * np.sin(a))!r} {float(r * np.sin(b))!r}\n")
        for i in range(nu + 1):
            for j in range(nv + 1):
                f.write(f"vt {2.0 * i / nu!r} {j / nv!r}\n")
        names = ("striped", "plain", "checked")
        for k in range(3):
            f.write(f"usemtl {names[k]}\n")
            for i in range(nu):
                for j in range(k * nv // 3, (k + 1) * nv // 3):
                    vs = [i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv]
                    ts = [i * (nv + 1) + j, (i + 1) * (nv + 1) + j, (i + 1) * (nv + 1) + j + 1, i * (nv + 1) + j + 1]
                    f.write("f " + " ".join(f"{a + 1}/{b + 1}" for a, b in zip(vs, ts)) + "\n")
    return os.path.join(folder, "torus.obj")


def build(obj, device, level=6, dataset="octree", num_samples=100000, samples_per_voxel=16, feature_dim=16, num_lods=4, hidden_dim=128,
          num_samples_on_mesh=2_000_000):
    """(blas, dataset, pipeline) as main_nglod.py builds them from nglod_octree.yaml with sample_tex: True."""
    from wisp.accelstructs import OctreeAS
    from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset
    from wisp.models import Pipeline
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDFTex
    blas = OctreeAS.from_mesh(obj, level=level, sample_tex=True, num_samples_on_mesh=num_samples_on_mesh)
    if dataset == "octree":
        ds = OctreeSampledSDFDataset(blas, split='train', sample_tex=True, num_samples=num_samples, samples_per_voxel=samples_per_voxel)
    else:
        ds = MeshSampledSDFDataset(obj, split='train', sample_tex=True, num_samples=max(num_samples // 5, 1))
    grid = OctreeGrid(blas, feature_dim=feature_dim, num_lods=num_lods, multiscale_type='sum', feature_std=0.01)
    nef = NeuralSDFTex(grid, embedder_type='identity', hidden_dim=hidden_dim, num_layers=1).to(device)
    return blas, ds, Pipeline(nef, None)


def view_rays(h, w, device, eye=(1.1, -1.4, 1.2), fov_deg=40.0):
    """Pinhole rays of an h x w view from `eye` towards the origin (z up)."""
    from wisp.core import Rays
    eye = np.asarray(eye, dtype=np.float64)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    t = np.tan(np.radians(fov_deg) / 2)
    ys, xs = np.meshgrid((np.arange(h) + 0.5) / h * 2 - 1, (np.arange(w) + 0.5) / w * 2 - 1, indexing='ij')
    d = fwd + xs[..., None] * t * (w / h) * right - ys[..., None] * t * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(eye, d.shape)
    return Rays(torch.tensor(o.reshape(-1, 3), dtype=torch.float32, device=device),
                torch.tensor(d.reshape(-1, 3), dtype=torch.float32, device=device), dist_min=0.0, dist_max=6.0)


def render_albedo(nef, h, w, device, num_steps=64):
    """(u8 [h, w, 3] albedo over a white background, number of rays that hit)."""
    from wisp.tracers import PackedSDFTracer
    tracer = PackedSDFTracer(num_steps=num_steps, step_size=0.8, min_dis=0.0003)
    with torch.no_grad():
        rb = tracer(nef, rays=view_rays(h, w, device), channels=["depth", "hit"], lod_idx=None)
        hit = rb.hit.reshape(-1)
        img = torch.ones(h * w, 3, device=device)
        if bool(hit.any()):
            img[hit] = nef(coords=rb.xyz.reshape(-1, 3)[hit], channels="rgb")
    return (img.clamp(0, 1) * 255).round().to(torch.uint8).reshape(h, w, 3).cpu().numpy(), int(hit.sum())


def fit_fused(nef, ds, cfg, device, epochs):
    """SDFTrainer's epochs with SDFTrainStep: shuffled batches of cfg.dataloader.batch_size (the last one may be short and is
    issued eagerly), the two un-normalised sums added up on the device and read back once per epoch, resampling after it."""
    from wisp.trainers import SDFTrainStep
    oc, bs = cfg.optimizer, cfg.dataloader.batch_size
    step = SDFTrainStep(nef, lr=oc.lr, eps=oc.eps, grid_lr_weight=cfg.grid_lr_weight, betas=oc.betas, optimizer='adam',
                        only_last=cfg.only_last)
    if torch.device(device).type == 'cuda' and len(ds) >= bs:
        step.capture(bs)
    nef.train()
    for epoch in range(cfg.max_epochs):
        coords, sdf, rgb = (ds.data[k].to(device) for k in ("coords", "sdf", "rgb"))
        order = torch.randperm(coords.shape[0], device=coords.device)
        l2, col = torch.zeros((), device=coords.device), torch.zeros((), device=coords.device)
        for a in range(0, order.shape[0], bs):
            pick = order[a:a + bs]
            step.step(coords[pick], sdf[pick].reshape(-1, 1), rgb[pick][..., :3].contiguous())
            l2, col = l2 + step.last_l2, col + step.last_rgb
        epochs.append((float(l2) / order.shape[0], float(col) / order.shape[0]))
        logging.info('EPOCH {}/{} | l2 loss: {:>.3E} | rgb loss: {:>.3E}'.format(epoch + 1, cfg.max_epochs, *epochs[-1]))
        if cfg.resample:
            ds.resample()
    nef.eval()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("obj", nargs="?")
    ap.add_argument("--write-test-mesh", metavar="DIR")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--dataset", choices=("octree", "mesh"), default="octree")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--num-samples", type=int, default=100000)
    ap.add_argument("--mesh-samples", type=int, default=2_000_000, help="surface samples the occupancy octree is built from")
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--fused-step", action="store_true")
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("H", "W"))
    ap.add_argument("--out-dir", default=os.path.join("_results", "sdf-tex"))
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    from wisp.ops.image import save_u8
    from wisp.trainers import ConfigAdam, ConfigDataloader, ConfigSDFTrainer, SDFTrainer
    obj = args.obj
    if args.write_test_mesh:
        obj = write_test_mesh(args.write_test_mesh)
    if not obj:
        ap.error("give an OBJ or --write-test-mesh DIR")
    torch.manual_seed(args.seed)
    blas, ds, pipeline = build(obj, args.device, level=args.level, dataset=args.dataset, num_samples=args.num_samples,
                                num_samples_on_mesh=args.mesh_samples)
    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=args.batch_size),
                           max_epochs=args.epochs, resample=True, only_last=True, exp_name='sdf-tex', profile_nvtx=False)
    epochs = []                                             # (l2, rgb) mean per sample of every finished epoch

    class Trainer(SDFTrainer):
        def log_console(self):
            super().log_console()
            m = self.tracker.metrics
            epochs.append((m.average_metric('l2_loss'), m.average_metric('rgb_loss')))

    t0 = time.time()
    if args.fused_step:
        fit_fused(pipeline.nef, ds, cfg, args.device, epochs)
    else:
        trainer = Trainer(cfg, pipeline, ds, device=args.device)
        trainer.train()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    seconds = time.time() - t0
    os.makedirs(args.out_dir, exist_ok=True)
    img, hits = render_albedo(pipeline.nef, args.size[0], args.size[1], args.device)
    out = os.path.join(args.out_dir, "albedo.png")
    save_u8(out, img)
    rec = dict(obj=os.path.abspath(obj), dataset=args.dataset, samples=len(ds), epochs=args.epochs, hits=hits, albedo=os.path.abspath(out),
               seconds=round(seconds, 3))
    if epochs:
        rec.update(l2_first=epochs[0][0], l2_last=epochs[-1][0], rgb_first=epochs[0][1], rgb_last=epochs[-1][1])
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
