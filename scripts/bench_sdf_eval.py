"""Evaluation of an nglod field, fused against modular, on the procedural torus of scripts/train_sdf_tex.py (level 6, four LODs,
hidden 128 - nglod_octree.yaml's shape): one JSON line, also written to --out.

Three comparisons, each the one-launch kernels of csrc/sdf_eval.hip against the modular ops (WISP_SDF_FUSED=0: octree query,
multi-level trilinear launch, decoder per call) in ONE process, repetitions alternating, medians of wall time around a device
synchronisation (the host work between launches is part of what is compared):
  validate  SDFTrainer.validate() over the whole dataset in batches of 512
  normals   central-difference normals at 2^16 points near the surface
  render    OfflineRenderer.render_lookat at 512 x 512 (WISP_SDF_FUSED=0 takes the MARCH through the modular loop as well: this row is
            march + normals, not the normals kernel alone)

--grid hash measures the same three on the field of nglod_hash.yaml (HashGrid.from_geometric, 'cat', 4 levels x 8 features, 16 ..
2048, tables of 2^--codebook-bitwidth rows; csrc/hash_sdf_eval.hip) and writes profiles/bench_hash_sdf_eval.json.
--grid triplanar measures them on the field of nglod_triplanar.yaml (TriplanarGrid, 'sum', one level of three 4 x 33 x 33 planes over
an AxisAlignedBBoxAS, MeshSampledSDFDataset; csrc/triplane_sdf_eval.hip), fitted with SDFTrainer (the field has no fused training
step), and writes profiles/bench_triplanar_sdf_eval.json; every timing also carries the maximum of its repetitions.
"""
import argparse
import json
import logging
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "scripts")]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def compare(fn, reps):
    """alternating fused / modular repetitions after one warm-up of each -> dict of medians and minima in ms"""
    times = {"fused": [], "modular": []}
    for rep in range(reps + 1):
        for mode in ("fused", "modular"):
            os.environ["WISP_SDF_FUSED"] = "1" if mode == "fused" else "0"
            ms = timed(fn)
            if rep:
                times[mode].append(ms)
    os.environ["WISP_SDF_FUSED"] = "1"
    out = {f"{m}_ms_median": round(statistics.median(v), 4) for m, v in times.items()}
    out.update({f"{m}_ms_min": round(min(v), 4) for m, v in times.items()})
    out.update({f"{m}_ms_max": round(max(v), 4) for m, v in times.items()})
    out["speedup_median"] = round(out["modular_ms_median"] / out["fused_ms_median"], 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--num-samples", type=int, default=100000)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2, help="epochs of fitting before measuring (the render needs a surface)")
    ap.add_argument("--grid", choices=("octree", "hash", "triplanar"), default="octree")
    ap.add_argument("--codebook-bitwidth", type=int, default=19, help="--grid hash: the hashed levels have 2^N rows")
    ap.add_argument("--out", default=None, help="default: profiles/bench_sdf_eval.json, bench_hash_sdf_eval.json with --grid hash, "
                                               "bench_triplanar_sdf_eval.json with --grid triplanar")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"hash": "bench_hash_sdf_eval.json", "triplanar": "bench_triplanar_sdf_eval.json"}
                                .get(args.grid, "bench_sdf_eval.json"))
    logging.basicConfig(level=logging.WARNING)
    import train_nglod
    from train_sdf_tex import write_test_mesh
    from wisp.ops.differential import finitediff_gradient
    from wisp.ops.sdf import sdf_fd_gradient, fused_sdf_field
    from wisp.trainers import ConfigAdam, ConfigDataloader, ConfigSDFTrainer, SDFTrainer
    from wisp.trainers.tracker import OfflineRenderer
    dev = "cuda"
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        obj = write_test_mesh(tmp)
        ds, pipeline = train_nglod.build(obj, dev, level=args.level, num_samples=args.num_samples, grid_type=args.grid,
                                         codebook_bitwidth=args.codebook_bitwidth)
    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=512),
                           max_epochs=args.epochs, resample=False, only_last=True, profile_nvtx=False)
    trainer = SDFTrainer(cfg, pipeline, ds, device=dev)
    if args.grid == "triplanar":
        trainer.train()
        pipeline.eval()
    else:
        train_nglod.fit_fused(trainer, ds, cfg, dev)
    nef = pipeline.nef
    assert fused_sdf_field(nef, None) is not None
    rec = dict(bench={"hash": "hash_sdf_eval", "triplanar": "triplanar_sdf_eval"}.get(args.grid, "sdf_eval"), device=torch.cuda.get_device_name(0), level=args.level,
               lods=nef.grid.num_lods, hidden=128, **(dict(codebook_bitwidth=args.codebook_bitwidth) if args.grid == "hash" else {}),
               dataset_points=len(ds), batches=len(trainer.train_data_loader), reps=args.reps)
    iou = {}

    def validate():
        iou[os.environ["WISP_SDF_FUSED"]] = trainer.validate()
    rec["validate"] = compare(validate, args.reps)
    rec["validate"]["iou_fused"], rec["validate"]["iou_modular"] = (list(iou[k].values())[0][-1] for k in ("1", "0"))
    pts = ds.data["coords"].to(dev)[:1 << 16].contiguous()
    rec["normals"] = dict(points=int(pts.shape[0]), **compare(lambda: sdf_fd_gradient(nef, pts, None), args.reps))
    with torch.no_grad():
        a = sdf_fd_gradient(nef, pts, None)
        b = finitediff_gradient(pts, nef.get_forward_function("sdf"))
    rec["normals"]["max_abs_diff"] = float((a - b).abs().max())
    renderer = OfflineRenderer(render_res=(args.size, args.size), shading_mode='normal', device=dev)
    hits = {}

    def render():
        # (render() switches the tracer's fused normals on; whether they ARE fused follows WISP_SDF_FUSED, and so does the march)
        rb = renderer.render_lookat(pipeline, f=[1.4, 1.2, 1.6], t=[0, 0, 0], fov=40.0, camera_clamp=[0, 6])
        hits[os.environ["WISP_SDF_FUSED"]] = int(rb.hit.sum())
    rec["render"] = dict(size=args.size, **compare(render, args.reps))
    rec["render"]["hits_fused"], rec["render"]["hits_modular"] = hits["1"], hits["0"]
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return rec


if __name__ == "__main__":
    main()
