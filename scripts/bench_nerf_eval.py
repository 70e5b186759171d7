"""Inference on the nerf_hash.yaml field, fused query against modular ops: one JSON line, also written to --out
(default profiles/bench_nerf_eval.json).

Two comparisons, each the one-launch query of csrc/nerf_query.hip against the modular path (WISP_NERF_QUERY_FUSED=0: the hash-grid
lookup launch into a feature tensor, then the exact-fp32 decoder launch) in ONE process, repetitions alternating, medians of wall
time around a device synchronisation:
  query   lookup + decoder alone at 2^18 and 2^21 random sample positions with per-sample view directions
  view    a whole 800 x 800 view through wisp.trainers.validation.render at render_batch 10 000 and 2^17 (march, the
          index_select of the ray directions, query, compositing)
The field is the untrained nerf_hash.yaml pipeline with tables drawn at std 0.1 and a dense level-7 octree: the cost of the query
does not depend on what the field has learned, and every ray that meets the cube carries samples.

--grid octree | codebook measures the query of csrc/nerf_octree_query.hip the same way on the nerf_octree.yaml / nerf_codebook.yaml
field (scripts/render_nerf.py: build_octree_pipeline - level-8 octree of the scene's surface point cloud, F = 5, 4 LODs, 'sum',
'voxel' march with 16 steps; tables and logits drawn at std 0.1), against WISP_NERF_OCTREE_QUERY_FUSED=0.  The query positions are
the 'voxel' march's own samples of the measured view (16 consecutive samples share a cell), not uniform draws, which would fall
into empty space.  Each row carries the median, the minimum and the maximum of its repetitions; `fused_max_below_modular_min` is
the claim the row is read for.  Written to profiles/bench_nerf_octree_eval.json.

--grid triplanar: the same plan on the nerf_triplanar.yaml field (scripts/render_nerf.py: build_triplanar_pipeline - planes of 33^2
to 257^2 texels, 4 features each, 'sum', 'voxel' march of the AABB with 512 steps; planes drawn at std 0.1) and the query of
csrc/nerf_triplane_query.hip, against WISP_NERF_TRIPLANE_QUERY_FUSED=0 - the modular ops: index_select of the directions, one
wisp_triplane_fwd launch, the decoder.  The two lookups agree to rounding, not to bits: every row carries the largest colour
difference.  Written to profiles/bench_nerf_triplanar_eval.json."""
import argparse
import json
import logging
import os
import statistics
import sys
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


def compare(fns, reps):
    """fns: dict mode -> callable; alternating repetitions after one warm-up of each -> medians, minima and the spread (max - min)"""
    times = {m: [] for m in fns}
    for rep in range(reps + 1):
        for mode, fn in fns.items():
            ms = timed(fn)
            if rep:
                times[mode].append(ms)
    out = {}
    for m, v in times.items():
        out[f"{m}_ms_median"] = round(statistics.median(v), 4)
        out[f"{m}_ms_min"] = round(min(v), 4)
        out[f"{m}_ms_spread"] = round(max(v) - min(v), 4)
        out[f"{m}_ms_max"] = round(max(v), 4)
    out["speedup_median"] = round(out["modular_ms_median"] / out["fused_ms_median"], 3)
    out["fused_max_below_modular_min"] = bool(out["fused_ms_max"] < out["modular_ms_min"])
    return out


def octree_main(args):
    """--grid octree | codebook: the same plan on the octree family's query"""
    from render_nerf import build_octree_pipeline, orbit_cameras
    from wisp.ops.nerf_mlp import fused_nerf_octree_query, nerf_octree_query_supported
    from wisp.ops.raygen import generate_centered_pixel_coords, generate_pinhole_rays
    from wisp.trainers.validation import render
    dev = "cuda:0"
    switch = "WISP_NERF_OCTREE_QUERY_FUSED"
    out_path = args.out or os.path.join(ROOT, "profiles", "bench_nerf_octree_eval.json")
    torch.manual_seed(0)
    pipeline = build_octree_pipeline(dev, args.grid, args.octree_level, args.cloud_rays, bg_color=(1.0, 1.0, 1.0))
    nef = pipeline.nef
    with torch.no_grad():
        for p in nef.grid.parameters():
            p.normal_(0.0, 0.1)
    pipeline.eval()
    os.environ[switch] = "1"
    with torch.no_grad():
        assert nerf_octree_query_supported(nef)
    cam = orbit_cameras(1, args.res, args.res)[0]
    rays = generate_pinhole_rays(cam, generate_centered_pixel_coords(args.res, args.res, device=dev)).reshape(-1, 3)
    with torch.no_grad():
        rm = nef.grid.raymarch(rays, level=nef.grid.active_lods[-1], num_samples=pipeline.tracer.num_steps, raymarch_type='voxel')
    total = int(rm.samples.shape[0])
    rec = dict(bench="nerf_octree_eval", grid=args.grid, device=torch.cuda.get_device_name(0), reps=args.reps,
               octree_level=args.octree_level, occupied_cells=int(nef.grid.blas.pyramid[0, args.octree_level]),
               view_samples=total, query={}, view={})
    for log2n in (18, 21):
        n = 1 << log2n
        pick = torch.arange(n, device=dev) % total                                  # the march's samples in order, repeated if short
        coords = rm.samples.index_select(0, pick).contiguous()
        dirs = rays.dirs.index_select(0, rm.ridx.long().index_select(0, pick)).contiguous()

        def fused():
            with torch.no_grad():
                fused_nerf_octree_query(nef, coords, ray_d=dirs)

        def modular():
            with torch.no_grad():
                nef(coords=coords, ray_d=dirs, channels=["rgb", "density"])
        with torch.no_grad():
            a = fused_nerf_octree_query(nef, coords, ray_d=dirs)
            b = nef(coords=coords, ray_d=dirs, channels=["rgb", "density"])
        row = compare(dict(fused=fused, modular=modular), args.reps)
        row["equal_bits"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].reshape(-1), b[1].reshape(-1)))
        row["max_abs_diff_rgb"] = float((a[0] - b[0]).abs().max())
        rec["query"][f"2^{log2n}"] = row
    for batch in (10000, 1 << 17):
        out = {}

        def view(flag, key):
            os.environ[switch] = "1" if flag else "0"
            torch.manual_seed(1)
            out[key] = render(pipeline, rays, render_batch=batch, channels=["rgb"], fused_query=True).rgb
        row = compare(dict(fused=lambda: view(True, "f"), modular=lambda: view(False, "m")), args.reps)
        os.environ[switch] = "1"
        row["equal_bits"] = bool(torch.equal(out["f"], out["m"]))
        row["max_abs_diff_rgb"] = float((out["f"] - out["m"]).abs().max())
        rec["view"][f"render_batch_{batch}"] = dict(res=args.res, **row)
    line = json.dumps(rec)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        kept = []
        if os.path.exists(out_path):                                                # one line per grid: replace this grid's
            kept = [l for l in open(out_path).read().splitlines() if l.strip() and json.loads(l).get("grid") != args.grid]
        with open(out_path, "w") as f:
            f.write("\n".join(kept + [line]) + "\n")
    print(line)
    return rec


def triplanar_main(args):
    """--grid triplanar: the plan of octree_main on the triplanar field's query"""
    from render_nerf import build_triplanar_pipeline, orbit_cameras
    from wisp.ops.nerf_mlp import fused_nerf_triplane_query, nerf_triplane_query_supported
    from wisp.ops.raygen import generate_centered_pixel_coords, generate_pinhole_rays
    from wisp.trainers.validation import render
    dev = "cuda:0"
    switch = "WISP_NERF_TRIPLANE_QUERY_FUSED"
    out_path = args.out or os.path.join(ROOT, "profiles", "bench_nerf_triplanar_eval.json")
    torch.manual_seed(0)
    pipeline = build_triplanar_pipeline(dev, args.num_steps)
    nef = pipeline.nef
    with torch.no_grad():
        for p in nef.grid.parameters():
            p.normal_(0.0, 0.1)
    pipeline.eval()
    os.environ[switch] = "1"
    with torch.no_grad():
        assert nerf_triplane_query_supported(nef)
    cam = orbit_cameras(1, args.res, args.res)[0]
    rays = generate_pinhole_rays(cam, generate_centered_pixel_coords(args.res, args.res, device=dev)).reshape(-1, 3)
    # the query rows take their positions from the tracer's own 'voxel' march of the AABB: a band of rows through the image centre
    # (the whole view's samples would be hundreds of millions)
    band = rays[(args.res // 2) * args.res:][:max(1, -(-(1 << 21) // args.num_steps) * 2)]
    with torch.no_grad():
        rm = nef.grid.raymarch(band, level=nef.grid.active_lods[-1], num_samples=pipeline.tracer.num_steps, raymarch_type='voxel')
    total = int(rm.samples.shape[0])
    assert total > 0
    sizes = [int(v.fsize) + 1 for v in nef.grid.features]
    rec = dict(bench="nerf_triplanar_eval", grid=args.grid, device=torch.cuda.get_device_name(0), reps=args.reps,
               num_steps=args.num_steps, plane_sizes=sizes, band_samples=total, query={}, view={})
    for log2n in (18, 21):
        n = 1 << log2n
        pick = torch.arange(n, device=dev) % total                                  # the march's samples in order, repeated if short
        coords = rm.samples.index_select(0, pick).contiguous()
        dirs = band.dirs.index_select(0, rm.ridx.long().index_select(0, pick)).contiguous()

        def fused():
            with torch.no_grad():
                fused_nerf_triplane_query(nef, coords, ray_d=dirs)

        def modular():
            with torch.no_grad():
                nef(coords=coords, ray_d=dirs, channels=["rgb", "density"])
        with torch.no_grad():
            a = fused_nerf_triplane_query(nef, coords, ray_d=dirs)
            b = nef(coords=coords, ray_d=dirs, channels=["rgb", "density"])
        row = compare(dict(fused=fused, modular=modular), args.reps)
        row["equal_bits"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].reshape(-1), b[1].reshape(-1)))
        row["max_abs_diff_rgb"] = float((a[0] - b[0]).abs().max())
        rec["query"][f"2^{log2n}"] = row
    for batch in (10000, 1 << 17):
        out = {}

        def view(flag, key):
            os.environ[switch] = "1" if flag else "0"
            torch.manual_seed(1)
            out[key] = render(pipeline, rays, render_batch=batch, channels=["rgb"], fused_query=True).rgb
        row = compare(dict(fused=lambda: view(True, "f"), modular=lambda: view(False, "m")), args.reps)
        os.environ[switch] = "1"
        row["equal_bits"] = bool(torch.equal(out["f"], out["m"]))
        row["max_abs_diff_rgb"] = float((out["f"] - out["m"]).abs().max())
        rec["view"][f"render_batch_{batch}"] = dict(res=args.res, reps=args.reps, **row)
    line = json.dumps(rec)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")
    print(line)
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--num-steps", type=int, default=512)
    ap.add_argument("--out", default=None, help="default: profiles/bench_nerf_eval.json, or profiles/bench_nerf_octree_eval.json "
                                                "(one line per grid) with --grid octree / codebook, or "
                                                "profiles/bench_nerf_triplanar_eval.json with --grid triplanar")
    ap.add_argument("--grid", choices=("hash", "octree", "codebook", "triplanar"), default="hash")
    ap.add_argument("--octree-level", type=int, default=8, help="--grid octree / codebook: depth of the scene's octree")
    ap.add_argument("--cloud-rays", type=int, default=1 << 21, help="--grid octree / codebook: rays of the surface point cloud")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.WARNING)
    if args.grid == "triplanar":
        return triplanar_main(args)
    if args.grid != "hash":
        return octree_main(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "bench_nerf_eval.json")
    from render_nerf import orbit_cameras
    from train_nerf_synthetic import build_pipeline
    from wisp.ops.nerf_mlp import fused_nerf_query, nerf_query_supported
    from wisp.ops.raygen import generate_centered_pixel_coords, generate_pinhole_rays
    from wisp.trainers.validation import render
    dev = "cuda:0"
    torch.manual_seed(0)
    pipeline = build_pipeline(dev, args.num_steps)
    nef = pipeline.nef
    with torch.no_grad():
        nef.grid.codebook.feats.normal_(0.0, 0.1)
    pipeline.eval()
    os.environ["WISP_NERF_QUERY_FUSED"] = "1"
    with torch.no_grad():
        assert nerf_query_supported(nef)
    rec = dict(bench="nerf_eval", device=torch.cuda.get_device_name(0), reps=args.reps, num_steps=args.num_steps, query={}, view={})
    for log2n in (18, 21):
        n = 1 << log2n
        g = torch.Generator(device=dev).manual_seed(log2n)
        coords = torch.rand(n, 3, device=dev, generator=g) * 2.0 - 1.0
        dirs = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)

        def fused():
            with torch.no_grad():
                fused_nerf_query(nef, coords, ray_d=dirs)

        def modular():
            with torch.no_grad():
                nef(coords=coords, ray_d=dirs, channels=["rgb", "density"])
        with torch.no_grad():
            a = fused_nerf_query(nef, coords, ray_d=dirs)
            b = nef(coords=coords, ray_d=dirs, channels=["rgb", "density"])
        row = compare(dict(fused=fused, modular=modular), args.reps)
        row["equal_bits"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].reshape(-1), b[1].reshape(-1)))
        rec["query"][f"2^{log2n}"] = row
    cam = orbit_cameras(1, args.res, args.res)[0]
    rays = generate_pinhole_rays(cam, generate_centered_pixel_coords(args.res, args.res, device=dev)).reshape(-1, 3)
    for batch in (10000, 1 << 17):
        out = {}

        def view(flag, key):
            torch.manual_seed(1)                                    # (the march's jitter seeds follow torch's CPU generator)
            out[key] = render(pipeline, rays, render_batch=batch, channels=["rgb"], fused_query=flag).rgb
        row = compare(dict(fused=lambda: view(True, "f"), modular=lambda: view(False, "m")), args.reps)
        row["equal_bits"] = bool(torch.equal(out["f"], out["m"]))
        rec["view"][f"render_batch_{batch}"] = dict(res=args.res, **row)
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return rec


if __name__ == "__main__":
    main()
