"""Mesh -> SDF kernel throughput (csrc/mesh_sdf.hip) on procedural bumpy spheres, one JSON line.

Per (F triangles, N points) shape: kernel time from device events around wisp._C.mesh_to_sdf (prep + main + finalize launches,
after a warm-up call), pairs/s, the fp64 operations per pair as counted below, and the fraction of the fp64 vector peak.  The peak
is AMD's specification for the MI355X (78.6 TFLOPS vector fp64), not a measurement.  Also: seconds to build an
OctreeSampledSDFDataset pool at level 7 with 32 samples per voxel (the wait of an nglod_octree user), on the 80 K-triangle mesh.

fp64 operations per (point, triangle) pair, an FMA counted as 2, following ms_pair:
  p - a, p - b, p - c                        9
  three (e x n) . (p - v) sign dots          15
  edge case: 3 x (dot 5 + scale 1 + |e c - p|^2 11)   51
  face case: n . (p - a) 5, squared and scaled 2       7
  q = (p - a) x e1 9, e2 . q 5                14
  13 directions: u = (p - a) . pvec * inv 6, v = d . q * inv (1..5 + 1), t 1, u + v 1 -> 129
  total                                      225
Comparisons, selects and float conversions are not counted.

Usage: python scripts/bench_mesh_sdf.py [--quick] [--stage scalar|lds] [--no-pool]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "tests")]

FLOPS_PER_PAIR = 9 + 15 + 51 + 7 + 14 + 129
PEAK_FP64 = 78.6e12            # AMD specification, vector fp64, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--stage", choices=["scalar", "lds"], default=None)
    ap.add_argument("--no-pool", action="store_true")
    args = ap.parse_args()
    if args.stage:
        os.environ["WISP_MESH_SDF_STAGE"] = args.stage
    assert torch.cuda.is_available(), "bench_mesh_sdf.py measures on the GPU"
    import mesh_sdf_oracle as meshes
    import wisp._C as C
    dev = "cuda:0"
    shapes = [(5, 100_000), (6, 1_000_000), (7, 3_000_000)] if not args.quick else [(5, 100_000), (6, 300_000)]
    rows = []
    built = {}
    for sub, n in shapes:
        V, F = built.setdefault(sub, meshes.bumpy_sphere(sub))
        T = torch.as_tensor(V[F], device=dev)
        P = (torch.rand(n, 3, device=dev, dtype=torch.float64) * 2 - 1)
        C.mesh_to_sdf(P[:1024], T)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = C.mesh_to_sdf(P, T)
        b.record()
        torch.cuda.synchronize()
        s = a.elapsed_time(b) / 1e3
        pairs = n * F.shape[0]
        rows.append(dict(triangles=int(F.shape[0]), points=n, kernel_s=round(s, 4), pairs_per_s=float(f"{pairs / s:.4g}"),
                         fp64_ops_per_pair=FLOPS_PER_PAIR,
                         fraction_of_fp64_peak=round(pairs * FLOPS_PER_PAIR / s / PEAK_FP64, 4),
                         inside_fraction=round(float((out < 0).double().mean()), 4)))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    pool = None
    if not args.no_pool:
        from wisp.accelstructs import OctreeAS
        from wisp.datasets import OctreeSampledSDFDataset
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            obj = meshes.write_obj(os.path.join(d, "bumpy.obj"), *built.setdefault(6, meshes.bumpy_sphere(6)))
            torch.manual_seed(0)
            blas = OctreeAS.from_mesh(obj, level=7, num_samples_on_mesh=10_000_000)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = OctreeSampledSDFDataset(blas, split='train', samples_per_voxel=32)
            torch.cuda.synchronize()
            pool = dict(triangles=81920, level=7, samples_per_voxel=32, pool_size=ds.pool_size,
                        seconds=round(time.perf_counter() - t0, 3))
    print(json.dumps(dict(metric="mesh_sdf", stage=os.environ.get("WISP_MESH_SDF_STAGE", "scalar"), device=torch.cuda.get_device_name(0),
                          peak_fp64_source="AMD specification 78.6 TFLOPS vector fp64 (not measured)", shapes=rows,
                          octree_pool=pool)))


if __name__ == "__main__":
    main()
