"""ms per optimisation step of the hash-grid SDF application (NeuralSDF over a HashGrid, nglod_hash.yaml: 'cat', 4 levels x 8
features, resolutions 16 .. 2048, tables of 2^19 rows, hidden 128) on the procedural torus of scripts/train_sdf_tex.py, four ways, at
512 coordinates per step (the config's batch) and at 2^16: one JSON line.

  * train_step_eager_modular     SDFTrainStep.step as a trainer built without fused_hash runs it: autograd over the modular launches
                                 + the single-launch optimizer - the only way to fit this field before the fused step;
  * train_step_eager_fused       SDFTrainStep(fused_hash=True).step: wisp_hash_sdf_train_step (two launches) + the optimizer;
  * train_step_captured_fused    the same, forward + loss + backward replayed as a HIP graph;
  * train_step_captured_modular  the graph of the modular launches.
Every figure is the median of `--reps` (at least 5) repetitions of `--steps` steps each between two HIP events, the four variants
taking turns inside one process; every variant trains its own copy of the same initial field on the same batches.

    python scripts/bench_hash_sdf_step.py [--reps 7] [--steps 200] [--out profiles/bench_hash_sdf_step.json]

--grid triplanar measures the field of nglod_triplanar.yaml instead (NeuralSDF over a TriplanarGrid: 'sum', one level of three
4 x 33 x 33 planes, hidden 128; the fused variants are SDFTrainStep(fused_triplane=True): wisp_triplane_sdf_train_step), the same
four variants at the same two batch sizes, and reports the largest repetition beside the median and the smallest:

    python scripts/bench_hash_sdf_step.py --grid triplanar [--out profiles/bench_triplanar_sdf_step.json]
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

from bench_sdf_tex_step import _time                                     # noqa: E402


def _alternate_spread(cases, reps, inner):
    """bench_sdf_tex_step._alternate, keeping the spread: ten warm-up steps each, then `reps` rounds in which the cases take turns
    -> median, min and max ms per step"""
    for fn in cases.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            times[k].append(_time(fn, inner))
    return ({k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()},
            {k: max(v) for k, v in times.items()})


def measure(nef, coords, sdf, B, reps, inner, opt_in="fused_hash"):
    """the four variants at batch size B -> (median ms, min ms, max ms, final losses); opt_in: SDFTrainStep's keyword of the fused step"""
    from wisp.trainers import SDFTrainStep
    n_batches = max(coords.shape[0] // B, 1)
    batches = [(coords[i * B:(i + 1) * B].contiguous(), sdf[i * B:(i + 1) * B].reshape(-1, 1).contiguous()) for i in range(n_batches)]
    assert batches[0][0].shape[0] == B, "the dataset is smaller than one batch"
    turn = {}

    def nxt(name):
        turn[name] = (turn.get(name, -1) + 1) % n_batches
        return batches[turn[name]]

    nefs = [copy.deepcopy(nef) for _ in range(4)]
    eager_modular = SDFTrainStep(nefs[0], lr=1e-3, eps=1e-15)
    assert eager_modular._fused_field() is None
    eager = SDFTrainStep(nefs[1], lr=1e-3, eps=1e-15, **{opt_in: True})
    assert eager._fused_field() is not None
    graph_fused = SDFTrainStep(nefs[2], lr=1e-3, eps=1e-15, **{opt_in: True}).capture(B)
    assert graph_fused._fused_field() is not None
    graph_modular = SDFTrainStep(nefs[3], lr=1e-3, eps=1e-15).capture(B)
    assert graph_modular._fused_field() is None
    cases = {"train_step_eager_modular": lambda: eager_modular.step(*nxt("m")),
             "train_step_eager_fused": lambda: eager.step(*nxt("e")),
             "train_step_captured_fused": lambda: graph_fused.step(*nxt("gf")),
             "train_step_captured_modular": lambda: graph_modular.step(*nxt("gm"))}
    med, low, high = _alternate_spread(cases, reps, inner)
    final = {k: float(v) for k, v in (("eager_modular", eager_modular.step(*batches[0])), ("eager_fused", eager.step(*batches[0])),
                                      ("captured_fused", graph_fused.step(*batches[0])),
                                      ("captured_modular", graph_modular.step(*batches[0])))}
    return med, low, high, final


def main_triplanar(args):
    """--grid triplanar: the same measurement on the field of nglod_triplanar.yaml"""
    import train_nglod
    import train_sdf_tex
    dev = "cuda:0"
    reps = max(args.reps, 5)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        obj = train_sdf_tex.write_test_mesh(tmp)
        ds, pipe = train_nglod.build(obj, dev, num_samples=5 << 17, grid_type="triplanar")       # (a fifth of it is sampled)
    nef = pipe.nef
    coords, sdf = ds.data["coords"].to(dev), ds.data["sdf"].to(dev)
    vol = nef.grid.features[0]
    result = dict(metric="triplanar_sdf_step",
                  source=f"HIP events around {args.steps} steps ({max(args.steps // 4, 1)} at 2^16), median, min and max of {reps} "
                         f"alternating repetitions in one process",
                  device=torch.cuda.get_device_name(0), num_lods=nef.grid.num_lods, feature_dim=vol.fdim, plane_size=vol.fsize + 1,
                  multiscale=nef.grid.multiscale_type, hidden=nef.decoder.layers[0].out_features, samples=int(coords.shape[0]))
    for B, inner in ((512, args.steps), (1 << 16, max(args.steps // 4, 1))):
        med, low, high, final = measure(nef, coords, sdf, B, reps, inner, opt_in="fused_triplane")
        result[f"batch_{B}"] = dict(**{k + "_ms": round(v, 4) for k, v in med.items()},
                                    **{"min_" + k + "_ms": round(v, 4) for k, v in low.items()},
                                    **{"max_" + k + "_ms": round(v, 4) for k, v in high.items()},
                                    eager_modular_over_eager_fused=round(med["train_step_eager_modular"] / med["train_step_eager_fused"], 2),
                                    eager_modular_over_captured_fused=round(med["train_step_eager_modular"] / med["train_step_captured_fused"], 2),
                                    captured_modular_over_captured_fused=round(med["train_step_captured_modular"] /
                                                                               med["train_step_captured_fused"], 2),
                                    final_losses=final)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", choices=("hash", "triplanar"), default="hash", help="nglod_hash.yaml or nglod_triplanar.yaml")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200, help="steps between the two events of one repetition (a quarter of it at 2^16)")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--codebook-bitwidth", type=int, default=19)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hash_sdf_step.py measures on the GPU"
    if args.grid == "triplanar":
        return _emit(main_triplanar(args), args.out)
    import train_nglod
    import train_sdf_tex
    dev = "cuda:0"
    reps = max(args.reps, 5)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        obj = train_sdf_tex.write_test_mesh(tmp)
        ds, pipe = train_nglod.build(obj, dev, level=args.level, num_samples=1 << 18, num_samples_on_mesh=500_000, grid_type="hash",
                                     codebook_bitwidth=args.codebook_bitwidth)
    nef = pipe.nef
    coords, sdf = ds.data["coords"].to(dev), ds.data["sdf"].to(dev)
    result = dict(metric="hash_sdf_step",
                  source=f"HIP events around {args.steps} steps ({max(args.steps // 4, 1)} at 2^16), median of {reps} alternating "
                         f"repetitions in one process",
                  device=torch.cuda.get_device_name(0), level=args.level, num_lods=nef.grid.num_lods, feature_dim=nef.grid.feature_dim,
                  codebook_bitwidth=args.codebook_bitwidth, hidden=nef.decoder.layers[0].out_features, samples=int(coords.shape[0]))
    for B, inner in ((512, args.steps), (1 << 16, max(args.steps // 4, 1))):
        med, low, _, final = measure(nef, coords, sdf, B, reps, inner)
        result[f"batch_{B}"] = dict(**{k + "_ms": round(v, 4) for k, v in med.items()},
                                    **{"min_" + k + "_ms": round(v, 4) for k, v in low.items()},
                                    eager_modular_over_eager_fused=round(med["train_step_eager_modular"] / med["train_step_eager_fused"], 2),
                                    eager_modular_over_captured_fused=round(med["train_step_eager_modular"] / med["train_step_captured_fused"], 2),
                                    captured_modular_over_captured_fused=round(med["train_step_captured_modular"] /
                                                                               med["train_step_captured_fused"], 2),
                                    final_losses=final)
    _emit(result, args.out)


def _emit(result, out):
    text = json.dumps(result)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
