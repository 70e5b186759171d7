"""Render a Structured Point Cloud file with its per-cell colours to an image: Pipeline(SPCField, PackedSPCTracer), one view.

    python scripts/render_spc.py SPC.npz [--size H W] [--eye X Y Z] [--fov DEG] [--out-dir DIR] [--fused 0|1]
    python scripts/render_spc.py --write-test-mesh DIR [--level L] [--num-samples N] ...

SPC.npz holds `octree` (u8) and optionally `colors` (u8, flat RGBA) / `normals` - what scripts/mesh2spc.py and the reference's
examples/spc_browser/mesh2spc.py write; it is loaded the way the reference's SPC browser does (widget_spc_selector.py:30-42).
--write-test-mesh DIR first writes the procedural textured torus of scripts/train_sdf_tex.py into DIR, converts it with
scripts/mesh2spc.py (DIR/torus.npz) and renders that, so the script runs where no asset exists.
Writes rgb.png (RGBA: colour of the first cell every pixel's ray hits over black, alpha = hit) and depth.png (grey, nearest =
brightest, 0 = no hit) into --out-dir.  The last line printed is one JSON record: cells, rays, hit share, milliseconds of the trace."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "scripts")]


def load_pipeline(filename, device):
    """Pipeline(SPCField, PackedSPCTracer) of an SPC file."""
    from wisp.models import Pipeline
    from wisp.models.nefs import SPCField
    from wisp.tracers import PackedSPCTracer
    spc_fields = np.load(filename)
    octree = torch.from_numpy(spc_fields['octree']).to(device)
    features = {k: torch.from_numpy(v).to(device) for k, v in spc_fields.items() if k in ('colors', 'normals')}
    return Pipeline(SPCField(spc_octree=octree, features_dict=features, device=device), PackedSPCTracer())


def view_rays(h, w, device, eye=(1.1, -1.4, 1.2), fov_deg=45.0):
    """Pinhole rays of an h x w look-at view from `eye` towards the origin (z up), through wisp.ops.raygen."""
    from wisp.ops.raygen import raygen
    cam = raygen.LookAtCamera(eye=eye, at=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), fov=float(np.radians(fov_deg)), width=w, height=h,
                              near=1e-2, far=1e2)
    grid = raygen.generate_centered_pixel_coords(w, h, device=device)
    return raygen.generate_pinhole_rays(cam, grid)


def render(pipeline, rays):
    """(RenderBuffer, milliseconds of the traced call by its own events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        pipeline(rays=rays, channels=["rgb", "depth", "hit", "alpha"])          # first call: lazy allocations
        e0.record()
        rb = pipeline(rays=rays, channels=["rgb", "depth", "hit", "alpha"])
        e1.record()
    torch.cuda.synchronize()
    return rb, e0.elapsed_time(e1)


def write_images(rb, h, w, out_dir):
    from wisp.ops.image import write_png
    os.makedirs(out_dir, exist_ok=True)
    hit = rb.hit.reshape(h, w)
    rgba = torch.cat([rb.rgb.reshape(h, w, 3).clamp(0, 1), hit[..., None].float()], dim=-1)
    write_png(os.path.join(out_dir, "rgb.png"), (rgba * 255).round().to(torch.uint8).cpu().numpy())
    d = rb.depth.reshape(h, w)
    if bool(hit.any()):
        lo, hi = d[hit].min(), d[hit].max()
        grey = torch.where(hit, 255.0 - 254.0 * (d - lo) / (hi - lo).clamp(min=1e-12), torch.zeros_like(d))
    else:
        grey = torch.zeros_like(d)
    write_png(os.path.join(out_dir, "depth.png"), grey.round().to(torch.uint8).cpu().numpy())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("spc", nargs="?")
    ap.add_argument("--write-test-mesh", metavar="DIR")
    ap.add_argument("--level", type=int, default=7, help="with --write-test-mesh: octree depth")
    ap.add_argument("--num-samples", type=int, default=1000000, help="with --write-test-mesh: surface samples")
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512), metavar=("H", "W"))
    ap.add_argument("--eye", type=float, nargs=3, default=(1.1, -1.4, 1.2))
    ap.add_argument("--fov", type=float, default=45.0, help="horizontal field of view, degrees")
    ap.add_argument("--fused", type=int, choices=(0, 1), default=None, help="force the tracer's path (default: the tracer's own)")
    ap.add_argument("--out-dir", default=os.path.join("_results", "spc"))
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    torch.manual_seed(args.seed)
    spc = args.spc
    if args.write_test_mesh:
        import mesh2spc
        from train_sdf_tex import write_test_mesh
        obj = write_test_mesh(args.write_test_mesh)
        spc = mesh2spc.convert_mesh_to_spc(obj, args.level, os.path.join(args.write_test_mesh, "torus.npz"), args.num_samples,
                                           'none', args.device)
    if not spc:
        ap.error("give an SPC .npz or --write-test-mesh DIR")
    h, w = args.size
    pipeline = load_pipeline(spc, args.device)
    if args.fused is not None:
        pipeline.tracer.fused = bool(args.fused)
    rays = view_rays(h, w, args.device, tuple(args.eye), args.fov)
    rb, ms = render(pipeline, rays)
    write_images(rb, h, w, args.out_dir)
    blas = pipeline.nef.grid.blas
    record = dict(spc=spc, level=int(blas.max_level), cells=int(blas.pyramid[0, blas.max_level]), rays=h * w,
                  hit_share=round(float(rb.hit.float().mean()), 6), ms=round(ms, 4), fused=bool(pipeline.tracer.fused),
                  out_dir=args.out_dir)
    print(json.dumps(record))
    return record


if __name__ == "__main__":
    main()
