"""SPC rendering, the fused first-hit launch against the modular raytrace path of PackedSPCTracer: a coloured torus shell (R 0.6,
r 0.25) as an SPC of levels 8 and 10, one 800 x 800 look-at view; one JSON line, also written to --out
(profiles/bench_spc_render.json).  Needs a GPU.

Per level, in ONE process: both paths warmed up, then --reps repetitions ALTERNATING fused / modular; a repetition is --inner
consecutive Pipeline calls bracketed by its own pair of device events (the modular path reads the nugget count back to the host
in every call; that wait is part of what it costs and lies between the events).  Reported per path: median, minimum, maximum and
interquartile range of milliseconds per call; the median ratio; nuggets per hitting ray of the full raytrace (what the modular
path generates and the fused one does not); and that the four buffers of the two paths are bitwise equal."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "scripts")]


def torus_cloud(level, device, R=0.6, r=0.25):
    """Points of the torus on a lattice over its two angles, fine enough that no cell of `level` the surface crosses is skipped
    (spacing below 0.4 of a cell along both circles)."""
    cell = 2.0 / 2 ** level
    na = int(np.ceil(2 * np.pi * (R + r) / (0.4 * cell)))
    nb = int(np.ceil(2 * np.pi * r / (0.4 * cell)))
    a = torch.arange(na, device=device, dtype=torch.float32) * (2 * np.pi / na)
    b = torch.arange(nb, device=device, dtype=torch.float32) * (2 * np.pi / nb)
    a, b = a[:, None], b[None, :]
    ring = R + r * torch.cos(b)
    return torch.stack([ring * torch.cos(a), ring * torch.sin(a), (r * torch.sin(b)).expand(na, nb)], dim=-1).reshape(-1, 3)


def build_pipeline(level, device, seed=0):
    from wisp.models import Pipeline
    from wisp.models.nefs import SPCField
    from wisp.ops.spc import pointcloud_to_octree
    from wisp.tracers import PackedSPCTracer
    octree = pointcloud_to_octree(torus_cloud(level, device), level)
    nef = SPCField(octree, None, device=device)
    cells = int(nef.grid.blas.pyramid[0, level])
    g = torch.Generator(device=device).manual_seed(seed)
    colors = torch.randint(0, 256, (cells * 4,), device=device, generator=g, dtype=torch.uint8)
    nef.colors = colors.reshape(-1, 4) / 255.0                               # what SPCField makes of a file's u8 RGBA
    return Pipeline(nef, PackedSPCTracer())


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4), iqr=round(q[2] - q[0], 4))


def measure(pipeline, rays, reps, inner):
    channels = ["rgb", "depth", "hit", "alpha"]
    tracer = pipeline.tracer
    out, times = {}, {"fused": [], "modular": []}
    with torch.no_grad():
        for rep in range(reps + 2):                                          # two warm-up rounds of both paths
            for mode in ("fused", "modular"):
                tracer.fused = mode == "fused"
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    rb = pipeline(rays=rays, channels=channels)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[mode].append(e0.elapsed_time(e1) / inner)
                out[mode] = rb
    same = all(torch.equal(getattr(out["fused"], k), getattr(out["modular"], k)) for k in ("rgb", "depth", "hit", "alpha"))
    return times, same, out["fused"]


def main(argv=None):
    import render_spc
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--levels", type=int, nargs="+", default=[8, 10])
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_spc_render.json"))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_spc_render.py measures on a GPU"
    record = dict(bench="spc_render", gpu=torch.cuda.get_device_name(0), size=args.size, reps=args.reps, calls_per_rep=args.inner,
                  unit="ms per Pipeline call, device events around each repetition", levels={})
    rays = render_spc.view_rays(args.size, args.size, args.device)
    for level in args.levels:
        pipeline = build_pipeline(level, args.device)
        blas = pipeline.nef.grid.blas
        times, same, rb = measure(pipeline, rays, args.reps, args.inner)
        rt = blas.raytrace(rays, level)
        hitting = int(rb.hit.sum())
        f, m = stats(times["fused"]), stats(times["modular"])
        record["levels"][str(level)] = dict(
            cells=int(blas.pyramid[0, level]), rays=int(rays.origins.shape[0]), hitting_rays=hitting,
            nuggets=int(rt.ridx.shape[0]), nuggets_per_hitting_ray=round(rt.ridx.shape[0] / max(hitting, 1), 3),
            fused_ms=f, modular_ms=m, modular_over_fused_median=round(m["median"] / f["median"], 3), buffers_bitwise_equal=bool(same))
        del pipeline, rt, rb
        torch.cuda.empty_cache()
    ahead = {lvl: ("fused" if r["modular_over_fused_median"] > 1.0 else "modular") for lvl, r in record["levels"].items()}
    record["ahead"] = ahead
    line = json.dumps(record)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    return record


if __name__ == "__main__":
    main()
