"""Per-step data path of a multiview dataset, resident fp32 tensors against the u8 bank: kernel times, one JSON line.

For 100 views of 800 x 800 (random texels and poses: the kernels' time does not depend on the picture) the script launches, at
least 1 000 times each after a warm-up,
  (a) wisp_gather_rows over the fp32 origins / directions / colours - the parent layout's SampleRays: 4 096 rays out of one view's
      [H*W, 3] tensors, and 2^18 rays out of the flattened all-view bank;
  (b) wisp_multiview_sample (csrc/dataset.hip) at the same counts, in one-view and in per-ray-view mode;
  (c) NeRFSyntheticDataset.view(i): a whole 800 x 800 view,
under `rocprofv3 --kernel-trace --stats` in a child process of its own, and reports the MEAN kernel time of every case from the
trace (cases are told apart by kernel name and grid size; single launches of a few microseconds jitter by more than 3 %).  (a)
copies 36 bytes per ray (the resident layout of MultiviewTensorDataset has no masks), (b) and (c) write 37.  Views rotate from
launch to launch and eight index sets alternate, so no case re-reads what the previous launch left in cache more than a training
loop would.  Also reported: the bytes both layouts keep on the device.

    python scripts/bench_nerf_synthetic.py [--launches 1000] [--views 100] [--res 800] [--out profiles/bench_nerf_synthetic.json]
    python scripts/bench_nerf_synthetic.py --load-timing [--views 100] [--res 800]     # host only: PIL against the built-in reader
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd")]
WARMUP = 20


def _random_poses(views, rng):
    poses = []
    for _ in range(views):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = q, rng.uniform(-4, 4, 3)
        poses.append(m)
    return poses


def child(args):
    """The launches themselves (run under rocprofv3).  Prints the case table the parent matches the trace against."""
    import torch
    import wisp._C as C
    from wisp.datasets import NeRFSyntheticDataset
    assert torch.cuda.is_available(), "bench_nerf_synthetic.py measures on the GPU"
    dev = "cuda:0"
    V, R, L = args.views, args.res, args.launches + WARMUP
    rng = np.random.default_rng(0)
    bank = rng.integers(0, 256, (V, R, R, 4), dtype=np.uint8)
    ds = NeRFSyntheticDataset.from_arrays(bank, _random_poses(V, rng), dict(camera_angle_x=0.6911112), device=dev)
    del bank
    new_bytes = ds.device_bytes()
    data = ds.data                                             # the resident layout: rays [V, H*W, 3] x 2, rgb, masks
    o, d, rgb = data["rays"].origins, data["rays"].dirs, data["rgb"]
    old_bytes = sum(t.numel() * t.element_size() for t in (o, d, rgb, data["masks"]))
    flat = [t.reshape(-1, 3) for t in (o, d, rgb)]
    torch.manual_seed(0)
    sets = 8
    small, large = 4096, 1 << 18
    pix_s = [torch.randint(0, R * R, [small], device=dev) for _ in range(sets)]
    pix_l = [torch.randint(0, R * R, [large], device=dev) for _ in range(sets)]
    view_s = [torch.randint(0, V, [small], device=dev) for _ in range(sets)]
    view_l = [torch.randint(0, V, [large], device=dev) for _ in range(sets)]
    row_l = [v * (R * R) + p for v, p in zip(view_l, pix_l)]
    whole = torch.arange(R * R, dtype=torch.int64, device=dev)
    cases = []

    def run(name, kernel, rays, fn):
        for k in range(L):
            fn(k)
        torch.cuda.synchronize()
        cases.append(dict(case=name, kernel=kernel, rays=rays, threads=-(-rays // 256) * 256))

    run("gather_rows_one_view_4096", "gather_rows_kernel", small,
        lambda k: C.gather_rows(pix_s[k % sets], [o[k % V], d[k % V], rgb[k % V]]))
    run("gather_rows_all_views_2p18", "gather_rows_kernel", large, lambda k: C.gather_rows(row_l[k % sets], flat))
    run("multiview_sample_one_view_4096", "multiview_sample_kernel<false>", small,
        lambda k: ds._launch(pix_s[k % sets], view_index=k % V))
    run("multiview_sample_per_ray_view_4096", "multiview_sample_kernel<true>", small,
        lambda k: ds._launch(pix_s[k % sets], view=view_s[k % sets]))
    run("multiview_sample_one_view_2p18", "multiview_sample_kernel<false>", large,
        lambda k: ds._launch(pix_l[k % sets], view_index=k % V))
    run("multiview_sample_per_ray_view_2p18", "multiview_sample_kernel<true>", large,
        lambda k: ds._launch(pix_l[k % sets], view=view_l[k % sets]))
    run("whole_view", "multiview_sample_kernel<false>", R * R, lambda k: ds._launch(whole, view_index=k % V))
    print("BENCH_CASES " + json.dumps(dict(device=torch.cuda.get_device_name(0), views=V, height=R, width=R, launches=args.launches,
                                           resident_bytes_fp32_layout=old_bytes, resident_bytes_u8_bank=new_bytes, cases=cases)))


def _trace_means(root, cases):
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], grid))
    rows.sort()
    if not rows:
        sys.exit("no *kernel_trace.csv under " + root)
    out = []
    for c in cases:
        # (a bool template argument is spelled <false> / <true> or <0> / <1> depending on the demangler)
        names = {c["kernel"], c["kernel"].replace("<false>", "<0>").replace("<true>", "<1>")}
        durs = [e - s for s, e, name, grid in rows if grid == c["threads"] and any(n in name for n in names)]
        durs = durs[WARMUP:]
        if not durs:
            sys.exit(f"no launches of {c['kernel']} with {c['threads']} threads in the trace")
        mean = sum(durs) / len(durs)
        out.append(dict(case=c["case"], rays=c["rays"], launches=len(durs), mean_kernel_us=round(mean / 1e3, 3),
                        min_kernel_us=round(min(durs) / 1e3, 3), rays_per_s=float(f"{c['rays'] / (mean * 1e-9):.4g}")))
    return out


def _smooth_rgba(res, k):
    """A picture with structure (ramps, discs, noise): PIL's encoder then uses all of PNG's filters, like rendered data."""
    yy, xx = np.mgrid[0:res, 0:res].astype(np.float32)
    rng = np.random.default_rng(k)
    img = np.zeros((res, res, 4), np.float32)
    for c in range(3):
        img[..., c] = 0.5 + 0.5 * np.sin(xx * (0.01 + 0.003 * c) + yy * 0.007 * (k % 5 + 1) + c)
    cx, cy, rad = rng.uniform(0.3, 0.7, 2).tolist() + [rng.uniform(0.15, 0.35)]
    dist = np.sqrt((xx / res - cx) ** 2 + (yy / res - cy) ** 2)
    img[..., 3] = np.clip((rad - dist) * 40.0, 0.0, 1.0)
    img[..., :3] += rng.normal(0, 0.02, (res, res, 3)).astype(np.float32)
    return (np.clip(img, 0, 1) * 255).round().astype(np.uint8)


def load_timing(args):
    """Wall time of NeRFSyntheticDataset(...) on the host (device='cpu') with PIL and with the built-in PNG reader."""
    import wisp.ops.image.io as io
    from wisp.datasets import NeRFSyntheticDataset
    if not io._have_pil():
        sys.exit("--load-timing compares against PIL, which does not import here")
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "images"))
        frames = []
        for k, pose in enumerate(_random_poses(args.views, rng)):
            io.save_u8(os.path.join(root, "images", f"r_{k}.png"), _smooth_rgba(args.res, k), use_pil=True)
            frames.append(dict(file_path=f"./images/r_{k}", transform_matrix=pose.tolist()))
        with open(os.path.join(root, "transforms.json"), "w") as f:
            json.dump(dict(camera_angle_x=0.6911112, frames=frames), f)
        file_bytes = sum(os.path.getsize(os.path.join(root, "images", n)) for n in os.listdir(os.path.join(root, "images")))
        out = dict(metric="nerf_synthetic_load", views=args.views, height=args.res, width=args.res, png_bytes=file_bytes)
        have = io._have_pil
        try:
            for name, pil, workers in (("pil", True, -1), ("builtin", False, -1), ("builtin_16_workers", False, 16)):
                io._have_pil = (lambda: True) if pil else (lambda: False)
                t0 = time.perf_counter()
                ds = NeRFSyntheticDataset(root, split='train', device='cpu', dataset_num_workers=workers)
                out[f"{name}_seconds"] = round(time.perf_counter() - t0, 2)
                assert len(ds) == args.views
        finally:
            io._have_pil = have
        # the built-in reader's worst case: files whose every row uses the Paeth filter (a Python loop per byte); PIL's own
        # encoder, which wrote the files above, mostly picks the filters numpy undoes a row at a time
        worst = os.path.join(root, "paeth.png")
        io.write_png(worst, _smooth_rgba(args.res, 0), filter_type=4)
        t0 = time.perf_counter()
        io.read_png(worst)
        out["builtin_all_paeth_seconds_per_view"] = round(time.perf_counter() - t0, 2)
        t0 = time.perf_counter()
        io.load_u8(worst, use_pil=True)
        out["pil_all_paeth_seconds_per_view"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--load-timing", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.load_timing:
        return load_timing(args)
    with tempfile.TemporaryDirectory() as trace:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "-o", "nerf_synthetic", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches), "--views", str(args.views),
               "--res", str(args.res)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = next((l for l in done.stdout.splitlines() if l.startswith("BENCH_CASES ")), None)
        if done.returncode != 0 or line is None:
            sys.stderr.write(done.stdout[-4000:])
            sys.exit(f"the profiled child failed (exit {done.returncode})")
        info = json.loads(line[len("BENCH_CASES "):])
        cases = _trace_means(trace, info.pop("cases"))
    by = {c["case"]: c["mean_kernel_us"] for c in cases}
    result = dict(metric="nerf_synthetic_data_path", source="rocprofv3 --kernel-trace, mean over the launches after a warm-up of "
                  f"{WARMUP}", **info, cases=cases,
                  new_over_old_4096=round(by["multiview_sample_one_view_4096"] / by["gather_rows_one_view_4096"], 3),
                  new_over_old_2p18=round(by["multiview_sample_per_ray_view_2p18"] / by["gather_rows_all_views_2p18"], 3))
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
