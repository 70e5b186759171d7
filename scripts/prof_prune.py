"""Where one occupancy prune of the benchmark's model spends its time.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o prune -- python scripts/prof_prune.py [--steps 300] [--prunes 5]
    python scripts/prof_prune.py --table DIR > profiles/prune_timeline_<tag>.txt

The first form builds bench.py's model (bench.build_pipeline on the dense level-7 octree, the bf16 trainer of
bench.py::make_trainer), trains it for --steps steps (prune every 100, adaptive ray count) so that the occupancy is a learned
one, and then runs --prunes prunes between two synchronisations, each bracketed by a float64 fill launch of SENTINEL_ELEMS
elements.  Without a profiler it still prints the wall-clock milliseconds per prune.  WISP_PRUNE_FUSED=0 selects the modular
prune.  The second form cuts the kernel trace at the sentinels and prints the per-launch table of the LAST prune (kernel,
duration, idle gap in front of it), the same launches summed per kernel, and the window of every prune."""
import argparse
import collections
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kaolin-wisp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SENTINEL_ELEMS = 1_000_003
SENTINEL_KERNEL = "FillFunctor<double>"


def run(args):
    import torch
    import bench
    import synlego
    from wisp.accelstructs import OctreeAS
    from wisp.core import Rays
    from wisp.trainers import MultiviewTrainStep
    import wisp._C as C
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cells = OctreeAS.make_dense(level=7).points[-(128 ** 3):].to(dev)
    pipe = bench.build_pipeline(dev, 64, 2048, cells)
    trainer = MultiviewTrainStep(pipe, lr=1e-3, eps=1e-16, weight_decay=1e-6, grid_lr_weight=500.0, rgb_loss_type='huber',
                                 prune_every=100, target_sample_size=2 ** 18, max_rays=2 ** 18, enable_amp=True)
    bank_o, bank_d, bank_rgb = synlego.ray_bank(2 ** 21, seed=1000, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1234)

    def batch(n):
        idx = torch.randint(0, bank_o.shape[0], (n,), device=dev, generator=gen)
        o, d, rgb = C.gather_rows(idx, [bank_o, bank_d, bank_rgb])
        return Rays(o, d, dist_min=synlego.NEAR, dist_max=synlego.FAR), rgb

    probe, _ = batch(4096)
    grid = pipe.nef.grid
    pipe.tracer.prev_num_samples = grid.raymarch(probe, level=grid.active_lods[-1], num_samples=2048,
                                                 raymarch_type='ray').samples.shape[0]
    R = max(256, trainer.calc_adaptive_rays(4096))
    for _ in range(args.steps):
        rays, gts = batch(R)
        trainer.step(rays, gts)
        R = max(256, trainer.num_rays)
    trainer.sync_master()
    trainer.prune()                                    # one outside the window: allocations of the first call of a path
    sentinel = torch.empty(SENTINEL_ELEMS, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.prunes):
        sentinel.fill_(0.0)
        trainer.prune()
        sentinel.fill_(0.0)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / args.prunes
    blas = grid.blas
    print(f"prune: {ms:.3f} ms each (wall clock, {args.prunes} prunes between two synchronisations, after {args.steps} steps); "
          f"fused={os.environ.get('WISP_PRUNE_FUSED', '1') != '0'}; leaf cells {int(blas.pyramid[0, blas.max_level])} of {cells.shape[0]}")


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    head = name.split("(")[0].strip()
    return (head if len(head) > 12 else name)[-96:]


def table(root):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if SENTINEL_KERNEL in r[2]]
    if len(marks) < 2 or len(marks) % 2:
        sys.exit(f"{len(marks)} sentinel launches under {root}: expected one pair per prune")
    windows = [(marks[k], marks[k + 1]) for k in range(0, len(marks), 2)]
    print(f"{len(windows)} prunes; window = end of the opening sentinel to start of the closing one")
    for k, (a, b) in enumerate(windows):
        busy = sum(e - s for s, e, _ in rows[a + 1:b])
        print(f"  prune {k}: window {1e-3 * (rows[b][0] - rows[a][1]):9.1f} us   launches {b - a - 1:3d}   busy {1e-3 * busy:9.1f} us")
    a, b = windows[-1]
    print("\nlast prune, launch by launch")
    print(f"{'#':>3} {'gap us':>9} {'us':>9}  kernel")
    prev = rows[a][1]
    per = collections.OrderedDict()
    gaps = 0
    for i, (s, e, kn) in enumerate(rows[a + 1:b]):
        gap = s - prev
        gaps += max(gap, 0)
        print(f"{i:3d} {1e-3 * gap:9.1f} {1e-3 * (e - s):9.1f}  {short(kn)}")
        c = per.setdefault(short(kn), [0, 0])
        c[0] += 1
        c[1] += e - s
        prev = max(prev, e)
    gaps += max(rows[b][0] - prev, 0)
    print(f"\nlast prune, per kernel (idle gaps between launches, closing gap included: {1e-3 * gaps:.1f} us)")
    print(f"{'calls':>5} {'us':>9}  kernel")
    for kn, (n, t) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        print(f"{n:5d} {1e-3 * t:9.1f}  {kn}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--prunes", type=int, default=5)
    ap.add_argument("--table", metavar="DIR", default=None)
    a = ap.parse_args()
    table(a.table) if a.table else run(a)
