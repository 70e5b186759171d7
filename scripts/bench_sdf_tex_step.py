"""ms per optimisation step of the textured SDF application (NeuralSDFTex over an OctreeGrid, nglod_octree.yaml with sample_tex:
512 coordinates per step) on the procedural torus of scripts/train_sdf_tex.py, four ways: one JSON line.

  * sdf_trainer_modular        SDFTrainer.step - autograd over the field, torch.optim.Adam, three metric read-backs: the only way
                               to fit a textured field before the fused step (and unchanged by it);
  * train_step_eager_fused     SDFTrainStep.step: wisp_sdf_tex_train_step (four launches) + the single-launch optimizer;
  * train_step_captured_fused  the same, forward + loss + backward replayed as a HIP graph;
  * train_step_captured_modular  the graph of the modular launches (WISP_SDF_TRAIN_FUSED=0 while capturing).
Every figure is the median of `--reps` (at least 5) repetitions of `--steps` steps each between two HIP events, the four variants
taking turns inside one process; every variant trains its own copy of the same initial field on the same batches.

    python scripts/bench_sdf_tex_step.py [--reps 7] [--steps 200] [--out profiles/bench_sdf_tex_step.json]
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
    """cases: {name: fn}.  Ten warm-up steps each, then `reps` rounds in which the cases take turns.  -> median and min ms per step"""
    for fn in cases.values():
        for _ in range(10):
            fn()
    times = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            times[k].append(_time(fn, inner))
    return {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200, help="steps between the two events of one repetition")
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sdf_tex_step.py measures on the GPU"
    import train_sdf_tex
    from wisp.models import Pipeline
    from wisp.trainers import ConfigAdam, ConfigDataloader, ConfigSDFTrainer, SDFTrainer, SDFTrainStep
    dev, B = "cuda:0", args.batch_size
    reps = max(args.reps, 5)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        obj = train_sdf_tex.write_test_mesh(tmp)
        blas, ds, pipe = train_sdf_tex.build(obj, dev, level=args.level, num_samples=50000, num_samples_on_mesh=500_000)
    nefs = [pipe.nef] + [copy.deepcopy(pipe.nef) for _ in range(3)]
    coords, sdf, rgb = (ds.data[k].to(dev) for k in ("coords", "sdf", "rgb"))
    n_batches = coords.shape[0] // B
    batches = [(coords[i * B:(i + 1) * B].contiguous(), sdf[i * B:(i + 1) * B].reshape(-1, 1).contiguous(),
                rgb[i * B:(i + 1) * B, :3].contiguous()) for i in range(n_batches)]
    turn = {}

    def nxt(name):
        turn[name] = (turn.get(name, -1) + 1) % n_batches
        return batches[turn[name]]

    cfg = ConfigSDFTrainer(optimizer=ConfigAdam(lr=1e-3, eps=1e-15), dataloader=ConfigDataloader(batch_size=B), max_epochs=1,
                           resample=False, only_last=True, exp_name='bench-sdf-tex', profile_nvtx=False)
    trainer = SDFTrainer(cfg, Pipeline(nefs[0], None), ds, device=dev)
    trainer.pre_training()
    trainer.pre_epoch()

    def modular():
        c, s, r = nxt("m")
        trainer.step(dict(coords=c, sdf=s, rgb=r))
    eager = SDFTrainStep(nefs[1], lr=1e-3, eps=1e-15)
    assert eager._fused_field() is not None
    graph_fused = SDFTrainStep(nefs[2], lr=1e-3, eps=1e-15).capture(B)
    assert graph_fused._fused_field() is not None
    os.environ["WISP_SDF_TRAIN_FUSED"] = "0"
    graph_modular = SDFTrainStep(nefs[3], lr=1e-3, eps=1e-15).capture(B)
    assert graph_modular._fused_field() is None
    os.environ.pop("WISP_SDF_TRAIN_FUSED")
    cases = {"sdf_trainer_modular": modular,
             "train_step_eager_fused": lambda: eager.step(*nxt("e")),
             "train_step_captured_fused": lambda: graph_fused.step(*nxt("gf")),
             "train_step_captured_modular": lambda: graph_modular.step(*nxt("gm"))}
    med, low = _alternate(cases, reps, args.steps)
    result = dict(metric="sdf_tex_step", source=f"HIP events around {args.steps} steps, median of {reps} alternating repetitions in one process",
                  device=torch.cuda.get_device_name(0), batch=B, level=args.level, num_lods=nefs[0].grid.num_lods,
                  hidden=nefs[0].hidden_dim, **{k + "_ms": round(v, 4) for k, v in med.items()},
                  **{"min_" + k + "_ms": round(v, 4) for k, v in low.items()},
                  modular_over_eager_fused=round(med["sdf_trainer_modular"] / med["train_step_eager_fused"], 2),
                  modular_over_captured_fused=round(med["sdf_trainer_modular"] / med["train_step_captured_fused"], 2),
                  captured_modular_over_captured_fused=round(med["train_step_captured_modular"] / med["train_step_captured_fused"], 2),
                  final_losses={k: float(v) for k, v in (("eager_fused", eager.step(*batches[0])),
                                                         ("captured_fused", graph_fused.step(*batches[0])),
                                                         ("captured_modular", graph_modular.step(*batches[0])))})
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
