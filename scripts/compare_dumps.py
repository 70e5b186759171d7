"""Table of a `bench.py --dump-outputs` comparison: usage  python scripts/compare_dumps.py --parent DIR DIR [DIR ...] --change DIR [DIR ...]
For every array: the largest difference between any two runs of the parent (max |diff| over max |a|), the largest difference between
any run of the change and any run of the parent, and whether the latter stays inside the former.  (The hash-grid backward sums its
coarse levels with float atomics, so two runs of one build agree bit for bit only by chance; how far they drift varies from pair to pair.)"""
import glob
import itertools
import os
import sys

import numpy as np

args = sys.argv[1:]
parents = args[args.index("--parent") + 1:args.index("--change")]
changes = args[args.index("--change") + 1:]
print(f"{len(parents)} parent runs ({len(parents) * (len(parents) - 1) // 2} pairs), {len(changes)} runs of the change "
      f"({len(parents) * len(changes)} change-parent pairs)")
print(f"{'array':20s} {'max|a|':>11s}   parent vs parent: max / pairs bit-equal      change vs parent: max / pairs bit-equal     inside")
ok = True
for f in sorted(glob.glob(os.path.join(parents[0], "*.npy"))):
    name = os.path.basename(f)[:-4]
    load = lambda d: np.load(os.path.join(d, name + ".npy")).astype(np.float64)
    P, C = [load(d) for d in parents], [load(d) for d in changes]
    scale = float(np.abs(P[0]).max()) or 1.0
    pp = [float(np.abs(a - b).max()) for a, b in itertools.combinations(P, 2)]
    cp = [float(np.abs(c - a).max()) for c in C for a in P]
    inside = max(cp) <= max(pp)
    ok = ok and inside
    print(f"{name:20s} {scale:11.4e}   {max(pp):.4e} = {max(pp) / scale:.3e} rel / {sum(d == 0 for d in pp)} of {len(pp)}"
          f"      {max(cp):.4e} = {max(cp) / scale:.3e} rel / {sum(d == 0 for d in cp)} of {len(cp)}     {inside}")
print("every array of the change inside the parent's own run-to-run difference:", ok)
