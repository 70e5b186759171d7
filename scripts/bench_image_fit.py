"""The image application's data path, whole-image render and training step on the GPU: one JSON line.

  * resident bytes: the u8 bank (3 B per pixel) against the reference layout of ImageDataset (32 B per pixel), at 4096^2 and 16384^2;
  * wisp_image_sample against wisp_gather_rows over resident fp32 coordinates and pixels (the parent layout's item), at 4 096 and
    2^18 indices of a 4096^2 image;
  * whole-image validation render (u8 image + squared error against the bank) at 4096^2 and 16384^2 on the same trained field:
    the fused launch of csrc/image_field.hip against 1 M-pixel chunks of nef.rgb - the path that exists without it;
  * ms per step at 4 096 pixels: ImageTrainer (torch.optim, fp16 autocast) against ImageTrainStep eager and captured, modular
    (autograd over the ops) and fused (ImageTrainStep(fused=True): wisp_image_field_train_step, csrc/image_field_train.hip) -
    five rows, with the spread (max - min over the repetitions) of every row.
Every figure is the median of `--reps` (at least 5) repetitions, the alternatives alternating inside one process; times are HIP
events around the launches (`inner` launches per repetition for the microsecond cases).  The fused render's fraction of the fp32
vector peak counts 2 x (46 x hidden + 3 x hidden) flops per pixel against 157.3 TFLOP/s.

    python scripts/bench_image_fit.py [--reps 5] [--big 16384] [--out profiles/bench_image_fit.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "scripts")]
PEAK_FP32_VECTOR = 157.3e12


def _time(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner                                   # ms


def _alternate(cases, reps, inner=1, with_max=False):
    """cases: {name: fn}.  One warm-up each, then `reps` rounds in which the cases take turns.  -> ({name: median ms}, {name: min ms})
    and, with_max, {name: max ms} as a third member"""
    for fn in cases.values():
        fn()
    times = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            times[k].append(_time(fn, inner))
    out = {k: statistics.median(v) for k, v in times.items()}, {k: min(v) for k, v in times.items()}
    return out + ({k: max(v) for k, v in times.items()},) if with_max else out


def _bank(side, dev):
    """u8 [side, side, 3]: train_image.py's procedural picture at 2048^2, tiled."""
    import train_image
    tile = torch.from_numpy(train_image.procedural_image(2048, 2048)).to(dev)
    k = side // 2048
    return tile.repeat(k, k, 1).contiguous() if k > 1 else tile[:side, :side].contiguous()


def _field(side, hidden, dev):
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import ImageNeuralField
    torch.manual_seed(0)
    grid = HashGrid.from_geometric(blas=None, feature_dim=2, num_lods=16, multiscale_type='cat', feature_std=1e-4, codebook_bitwidth=19,
                                   min_grid_res=16, max_grid_res=side // 2)
    return ImageNeuralField(grid, hidden_dim=hidden).to(dev)


def bench_sample(bank, reps):
    import wisp._C as C
    h, w = bank.shape[:2]
    idx_all = torch.arange(h * w, device=bank.device)
    res = C.image_sample(bank, idx_all)
    coords, pixels = res["coords"], res["rgb"]                          # the resident fp32 tensors of the parent layout
    out = []
    for n, inner in ((4096, 200), (1 << 18, 50)):
        sets = [torch.randint(0, h * w, (n,), device=bank.device) for _ in range(8)]
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % len(sets)
            return sets[turn[0]]
        med, low = _alternate({"gather_rows": lambda: C.gather_rows(nxt(), [coords, pixels]),
                               "image_sample": lambda: C.image_sample(bank, nxt())}, reps, inner)
        out.append(dict(indices=n, launches_per_rep=inner, gather_rows_us=round(1e3 * med["gather_rows"], 3),
                        image_sample_us=round(1e3 * med["image_sample"], 3), min_gather_rows_us=round(1e3 * low["gather_rows"], 3),
                        min_image_sample_us=round(1e3 * low["image_sample"], 3),
                        new_over_old=round(med["image_sample"] / med["gather_rows"], 3)))
    del coords, pixels
    return out


def bench_render(side, hidden, reps, train_steps, dev):
    import wisp._C as C
    from wisp.models.nefs import fused_render_shape, render_image
    from wisp.trainers import ImageTrainStep
    bank = _bank(side, dev)
    nef = _field(side, hidden, dev)
    step = ImageTrainStep(nef, lr=1e-3, eps=1e-16, weight_decay=1e-6, grid_lr_weight=500.0)
    for _ in range(train_steps):
        s = C.image_sample(bank, torch.randint(0, side * side, (4096,), device=dev))
        step.step(s["coords"], s["rgb"])
    assert fused_render_shape(nef) is not None
    got = {}

    def fused():
        os.environ["WISP_IMAGE_RENDER_FUSED"] = "1"
        got["fused"] = render_image(nef, side, side, out='u8', gts_u8=bank)[1]

    def chunked():
        os.environ["WISP_IMAGE_RENDER_FUSED"] = "0"
        got["chunked"] = render_image(nef, side, side, out='u8', gts_u8=bank)[1]
    med, low = _alternate({"chunked": chunked, "fused": fused}, reps)
    os.environ.pop("WISP_IMAGE_RENDER_FUSED", None)
    # the kernel alone (no weight packing, no partial sum): what the roofline fraction is taken from
    grid, l1, lout = nef.grid, nef.decoder.layers[0], nef.decoder.lout
    packed, hp = C.image_field_pack_weights(l1.weight, l1.bias, lout.weight, lout.bias, grid.num_lods)
    args = (grid.codebook.feats.detach(), grid.codebook.begin_idxes, grid.codebook.resolutions.reshape(-1).tolist(), grid.codebook_bitwidth,
            grid.num_lods - 1, packed, hp)
    kern = [_time(lambda: C.image_field_render(side, side, 0, side * side, *args, gts_u8=bank, want_f32=False, want_u8=True, want_err=True))
            for _ in range(reps + 1)][1:]
    kernel_ms = statistics.median(kern)
    flops = 2.0 * (46 * hidden + 3 * hidden) * side * side
    mse_f, mse_c = float(got["fused"]) / (3 * side * side), float(got["chunked"]) / (3 * side * side)
    return dict(side=side, pixels=side * side, hidden=hidden, train_steps=train_steps, chunked_ms=round(med["chunked"], 3),
                fused_ms=round(med["fused"], 3), min_chunked_ms=round(low["chunked"], 3), min_fused_ms=round(low["fused"], 3),
                fused_kernel_ms=round(kernel_ms, 3), speedup=round(med["chunked"] / med["fused"], 2),
                fused_kernel_gpixels_per_s=round(side * side / kernel_ms / 1e6, 3),
                fused_kernel_fraction_of_fp32_vector_peak=round(flops / (kernel_ms * 1e-3) / PEAK_FP32_VECTOR, 4),
                psnr_fused=round(10 * np.log10(1 / mse_f), 4), psnr_chunked=round(10 * np.log10(1 / mse_c), 4))


def bench_step(reps, dev, steps=100):
    from train_image import build, trainer_config
    import tempfile
    from wisp.ops.image import save_u8
    import train_image
    from wisp.trainers import ImageTrainer, ImageTrainStep
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.png")
        save_u8(path, train_image.procedural_image(1024, 1024))
        made = [build(path, dev) for _ in range(5)]
    ds = made[0][0]
    for _, pipeline in made[1:]:                                       # (ImageTrainer moves its own pipeline)
        pipeline.nef.to(dev)
    trainer = ImageTrainer(trainer_config(100), made[0][1], ds, device=dev)
    trainer.pre_training()
    eager = ImageTrainStep(made[1][1].nef, lr=1e-3, eps=1e-16, weight_decay=1e-6, grid_lr_weight=500.0)
    graph = ImageTrainStep(made[2][1].nef, lr=1e-3, eps=1e-16, weight_decay=1e-6, grid_lr_weight=500.0).capture(4096)

    fused = ImageTrainStep(made[3][1].nef, lr=1e-3, eps=1e-16, weight_decay=1e-6, grid_lr_weight=500.0, fused=True)
    fused_graph = ImageTrainStep(made[4][1].nef, lr=1e-3, eps=1e-16, weight_decay=1e-6, grid_lr_weight=500.0, fused=True).capture(4096)
    assert fused._fused_field() is not None and fused_graph._fused_field() is not None

    def dropin():
        c, p = ds[0]
        trainer.step([c[None], p[None]])
    cases = {"image_trainer": dropin, "train_step_eager": lambda: eager.step(*ds[0]),
             "train_step_captured": lambda: graph.step(*ds[0]), "train_step_fused": lambda: fused.step(*ds[0]),
             "train_step_fused_captured": lambda: fused_graph.step(*ds[0])}
    med, low, high = _alternate(cases, reps, inner=steps, with_max=True)
    return dict(pixels_per_step=4096, steps_per_rep=steps, **{k + "_ms": round(v, 4) for k, v in med.items()},
                **{"min_" + k + "_ms": round(v, 4) for k, v in low.items()},
                **{"spread_" + k + "_ms": round(high[k] - low[k], 4) for k in med})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=16384, help="side of the large image (0: skip it)")
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--accuracy", default=None, help="JSON-lines file of tests/gpu_helpers.margin records to carry into the result")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_image_fit.py measures on the GPU"
    reps = max(args.reps, 5)
    dev = "cuda:0"
    sides = [4096] + ([args.big] if args.big else [])
    result = dict(metric="image_fit", source=f"HIP events, median of {reps} alternating repetitions in one process",
                  device=torch.cuda.get_device_name(0),
                  resident_bytes=[dict(side=s, u8_bank=3 * s * s, reference_layout=32 * s * s) for s in (4096, 16384)])
    result["sample"] = bench_sample(_bank(4096, dev), reps)
    torch.cuda.empty_cache()
    result["render"] = []
    for side in sides:
        for hidden in (64, 128) if side == 4096 else (64,):
            result["render"].append(bench_render(side, hidden, reps, args.train_steps, dev))
            torch.cuda.empty_cache()
    result["step"] = bench_step(reps, dev)
    if args.accuracy and os.path.exists(args.accuracy):
        result["render_error_vs_oracle"] = [json.loads(l) for l in open(args.accuracy) if "render vs oracle" in l]
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
