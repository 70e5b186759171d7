"""ms per optimisation step of an octree SDF field trained with the loss over EVERY level of detail (only_last=False; 512
coordinates per step, 6 LODs, hidden 128) on the procedural torus of scripts/train_sdf_tex.py, for the plain field (NeuralSDF) and the
textured one (NeuralSDFTex), five ways each: one JSON line.

  * modular_eager      SDFTrainStep(only_last=False).step: one field query + decoder per LOD through autograd, and all of it backwards;
  * modular_captured   the same launches replayed as a HIP graph;
  * fused_eager        SDFTrainStep(only_last=False, fused_lods=True).step: wisp_sdf_lods_train_step (four launches) + the optimizer;
  * fused_captured     the same, forward + loss + backward replayed as a HIP graph;
  * one_lod_captured   the existing one-LOD fused step (only_last=True) as a HIP graph: what the finest LOD alone costs.
Every figure is the median (with min and max) of `--reps` (at least 5) repetitions of `--steps` steps each between two HIP events,
the variants taking turns inside one process; every variant trains its own copy of the same initial field on the same batches.

    python scripts/bench_sdf_lods_step.py [--reps 7] [--steps 200] [--out profiles/bench_sdf_lods_step.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "scripts")]

ROWS = ("modular_eager", "modular_captured", "fused_eager", "fused_captured", "one_lod_captured")


def _time(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner                                   # ms


def _alternate(cases, reps, inner):
    """cases: {name: fn}.  Ten warm-up steps each, then `reps` rounds in which the cases take turns.  -> {name: [ms per step]}"""
    for fn in cases.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            times[k].append(_time(fn, inner))
    return times


def _steps(nef, B, batches):
    """the five variants over copies of `nef` -> {'<row>': fn}"""
    from wisp.trainers import SDFTrainStep
    nefs = [copy.deepcopy(nef) for _ in ROWS]
    turn = {}

    def nxt(name):
        turn[name] = (turn.get(name, -1) + 1) % len(batches)
        return batches[turn[name]]

    kw = dict(lr=1e-3, eps=1e-15)
    modular_eager = SDFTrainStep(nefs[0], only_last=False, **kw)
    modular_captured = SDFTrainStep(nefs[1], only_last=False, **kw).capture(B)
    assert modular_eager._fused_field() is None and modular_captured._fused_field() is None
    fused_eager = SDFTrainStep(nefs[2], only_last=False, fused_lods=True, **kw)
    fused_captured = SDFTrainStep(nefs[3], only_last=False, fused_lods=True, **kw).capture(B)
    for s in (fused_eager, fused_captured):
        assert (s._fused_field() or {}).get("lods_loss"), "the field did not take the all-LOD fused step"
    one_lod = SDFTrainStep(nefs[4], only_last=True, **kw).capture(B)
    assert one_lod._fused_field() is not None
    steps = dict(zip(ROWS, (modular_eager, modular_captured, fused_eager, fused_captured, one_lod)))
    return {k: (lambda s=s, k=k: s.step(*nxt(k))) for k, s in steps.items()}, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200, help="steps between the two events of one repetition")
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--num-lods", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sdf_lods_step.py measures on the GPU"
    import train_sdf_tex
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDF
    dev, B = "cuda:0", args.batch_size
    reps = max(args.reps, 5)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        obj = train_sdf_tex.write_test_mesh(tmp)
        blas, ds, pipe = train_sdf_tex.build(obj, dev, level=args.level, num_samples=50000, num_samples_on_mesh=500_000,
                                             num_lods=args.num_lods, hidden_dim=args.hidden)
    grid = OctreeGrid(blas, feature_dim=16, num_lods=args.num_lods, multiscale_type='sum', feature_std=0.01)
    plain = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=args.hidden, num_layers=1).to(dev)
    coords, sdf, rgb = (ds.data[k].to(dev) for k in ("coords", "sdf", "rgb"))
    n_batches = coords.shape[0] // B
    cut = lambda t, i: t[i * B:(i + 1) * B]
    batches = dict(plain=[(cut(coords, i).contiguous(), cut(sdf, i).reshape(-1, 1).contiguous()) for i in range(n_batches)],
                   textured=[(cut(coords, i).contiguous(), cut(sdf, i).reshape(-1, 1).contiguous(), cut(rgb, i)[:, :3].contiguous())
                             for i in range(n_batches)])
    cases, steps = {}, {}
    for field, nef in (("plain", plain), ("textured", pipe.nef)):
        fns, st = _steps(nef, B, batches[field])
        cases.update({f"{field}_{k}": fn for k, fn in fns.items()})
        steps.update({f"{field}_{k}": s for k, s in st.items()})
    times = _alternate(cases, reps, args.steps)
    result = dict(metric="sdf_lods_step", source=f"HIP events around {args.steps} steps, median [min, max] of {reps} alternating "
                                                 "repetitions in one process",
                  device=torch.cuda.get_device_name(0), batch=B, level=args.level, num_lods=args.num_lods, hidden=args.hidden)
    for k, v in times.items():
        result[k + "_ms"] = round(statistics.median(v), 4)
        result[k + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
    for field in ("plain", "textured"):
        med = lambda row: statistics.median(times[f"{field}_{row}"])
        result[f"{field}_captured_modular_over_captured_fused"] = round(med("modular_captured") / med("fused_captured"), 2)
        result[f"{field}_eager_modular_over_eager_fused"] = round(med("modular_eager") / med("fused_eager"), 2)
        result[f"{field}_captured_fused_over_one_lod"] = round(med("fused_captured") / med("one_lod_captured"), 2)
        result[f"{field}_fused_captured_wholly_below_modular_captured"] = bool(
            max(times[f"{field}_fused_captured"]) < min(times[f"{field}_modular_captured"]))
        result[f"{field}_final_losses"] = {row: float(steps[f"{field}_{row}"].step(*batches[field][0])) for row in ROWS}
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
