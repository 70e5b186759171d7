"""SSIM of one 800 x 800 x 3 pair, three ways; one JSON line, also written to --out (profiles/bench_ssim.json).  Needs a GPU.

  kernel   wisp.ops.image.structural_similarity: the two launches of csrc/ssim.hip, fp64 arithmetic on the fp32 images, nothing read back;
  torch    the same definition restated with torch in fp64 on the device: reflect padding, five quantities filtered by two
           separable conv2d passes, the statistic elementwise, the cropped mean - what a user would write without the kernel;
  host     the reference's route (wisp/ops/image/metrics.py:70-90): both images copied to the host, then the float64
           restatement over scipy.ndimage.gaussian_filter (tests/ssim_ref.py), on at most 16 threads.

In ONE process: all three warmed up, then --reps repetitions ALTERNATING kernel / torch / host.  A repetition of a device path is
--inner consecutive calls between a pair of device events; a repetition of the host path is one call on the host clock, from
device tensors to a Python float.  Reported per path: median, minimum, maximum and interquartile range of milliseconds per call,
the median ratios, the kernel's bytes and fp64 operations per call counted from the shape, and how far the three values lie
apart."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "tests")]


def torch_ssim(x, y, weights, cov_norm, c1, c2):
    """[H, W, C] fp32 images on the device -> 0-d float64 tensor; every step a torch op in float64"""
    r = (weights.numel() - 1) // 2
    a, b = x.permute(2, 0, 1)[:, None].double(), y.permute(2, 0, 1)[:, None].double()              # [C, 1, H, W]
    stack = torch.cat([a, b, a * a, b * b, a * b])                                                   # [5 C, 1, H, W]
    # (torch's 'reflect' mirrors about the edge pixel, scipy's about the edge: they differ on the border of the map only, which the
    # cropped mean never sees - one pad launch instead of four flips)
    stack = torch.nn.functional.pad(stack, (r, r, r, r), mode='reflect')
    f = torch.nn.functional.conv2d(stack, weights.reshape(1, 1, 1, -1))
    f = torch.nn.functional.conv2d(f, weights.reshape(1, 1, -1, 1))
    ux, uy, uxx, uyy, uxy = f.reshape(5, -1, *f.shape[2:])
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s[:, r:s.shape[1] - r, r:s.shape[2] - r].mean(dim=(1, 2)).mean()


def host_ssim(x, y):
    import ssim_ref
    return float(ssim_ref.ssim(x[..., :3].cpu().numpy(), y[..., :3].cpu().numpy())[0])


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return dict(median=round(statistics.median(ms), 5), min=round(min(ms), 5), max=round(max(ms), 5), iqr=round(q[2] - q[0], 5))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, nargs=2, default=(800, 800), metavar=("H", "W"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ssim.json"))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_ssim.py measures on a GPU"
    from wisp.ops.image import gaussian_window, structural_similarity
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    h, w = args.size
    g = torch.Generator(device=args.device).manual_seed(0)
    gts = torch.rand(h, w, 3, device=args.device, generator=g)
    gts[: h // 2] = 1.0                                                      # a flat background, as rendered views have
    pred = (gts + 0.02 * torch.randn(h, w, 3, device=args.device, generator=g)).clamp(0, 1)
    weights = torch.from_numpy(gaussian_window()).to(args.device)
    r = (weights.numel() - 1) // 2
    cov_norm, c1, c2 = weights.numel() ** 2 / (weights.numel() ** 2 - 1.0), 1e-4, 9e-4
    paths = dict(kernel=lambda: structural_similarity(pred, gts), torch=lambda: torch_ssim(pred, gts, weights, cov_norm, c1, c2))
    values, times = {}, dict(kernel=[], torch=[], host=[])
    for rep in range(args.reps + 2):                                         # two warm-up rounds of all three
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(e0.elapsed_time(e1) / args.inner)
            values[name] = float(out)
        t0 = time.perf_counter()
        values["host"] = host_ssim(pred, gts)
        if rep >= 2:
            times["host"].append(1e3 * (time.perf_counter() - t0))
    tiles, halo = -(-h // 16) * -(-w // 16), 16 + 2 * r
    record = dict(bench="ssim", gpu=torch.cuda.get_device_name(0), size=[h, w, 3], reps=args.reps, calls_per_rep=args.inner,
                  unit="ms per call; device paths: device events around each repetition; host: wall clock of one call, copies included",
                  host_threads=int(os.environ.get("OMP_NUM_THREADS", 0)) or torch.get_num_threads(),
                  kernel_ms=stats(times["kernel"]), torch_fp64_ms=stats(times["torch"]), host_scipy_ms=stats(times["host"]),
                  kernel_counts=dict(bytes_read_from_memory=2 * 4 * h * w * 3, bytes_requested_with_halo=2 * 4 * 3 * tiles * halo * halo,
                                     fp64_fma=3 * tiles * (halo * 16 + 256) * (2 * r + 1) * 5),
                  ssim=values, kernel_minus_host=values["kernel"] - values["host"], torch_minus_host=values["torch"] - values["host"])
    record["torch_over_kernel_median"] = round(record["torch_fp64_ms"]["median"] / record["kernel_ms"]["median"], 2)
    record["host_over_kernel_median"] = round(record["host_scipy_ms"]["median"] / record["kernel_ms"]["median"], 1)
    record["ahead"] = min(("kernel", "torch_fp64", "host_scipy"), key=lambda k: record[k + "_ms"]["median"])
    line = json.dumps(record)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    return record


if __name__ == "__main__":
    main()
