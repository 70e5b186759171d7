"""wisp_composite_loss on a batch whose ray lengths are exactly profiles/ray_length_hist_2p18.json's histogram (shuffled, fixed
seed): WISP_COMPOSITE_SPLIT = 0 (one wave per ray) against the default (long rays over the four waves of their workgroup), rounds
interleaved.  The measurement runs in a child process under a time limit.  The C entry point is called directly on preallocated
buffers, CALLS times back to back between two events, so that a figure is device time per call and not the host's.
(profiles/long_rays_ab.txt also keeps the figures of two variants that were measured with this script and dropped: K = 8 chunks
per wave, and raymarch_ray_count with 2 / 4 / 8 active chunks of a ray in flight.)"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, CALLS = 30, 20


def report(title, ts):
    print(title)
    for name, v in ts.items():
        v = sorted(v)
        print(f"  {name:10s} min {v[0]:7.2f}  median {v[len(v) // 2]:7.2f}  max {v[-1]:7.2f}", flush=True)


def timed(fns):
    import torch
    ts = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(5): fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS): fn()
            b.record(); torch.cuda.synchronize(); ts[name].append(a.elapsed_time(b) * 1e3 / CALLS)
    return ts


def composite():
    import numpy as np, torch
    import wisp._C as C
    dev = "cuda:0"
    hist = json.load(open(os.path.join(ROOT, "profiles", "ray_length_hist_2p18.json")))["histogram_rays_by_length"]
    rng = np.random.default_rng(0)
    lens = rng.permutation(np.repeat(np.arange(len(hist)), hist))
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    R, S = len(lens), int(lens.sum())
    g = torch.Generator(device=dev).manual_seed(0)
    color = torch.rand(S, 3, device=dev, generator=g)
    dens = torch.rand(S, 1, device=dev, generator=g) * 30 * (torch.rand(S, 1, device=dev, generator=g) < 0.6)
    delt = torch.rand(S, 1, device=dev, generator=g) * 2e-3 + 1e-3
    gts = torch.rand(R, 3, device=dev, generator=g)
    gc, gd, loss, ws = torch.empty(S, 3, device=dev), torch.empty(S, 1, device=dev), torch.empty(1, device=dev), torch.empty(2 * R, device=dev)
    bg_arr, bg_ptr = C._host_f32((1.0, 1.0, 1.0))
    stream = C._stream()

    def call(split):
        def fn():
            os.environ["WISP_COMPOSITE_SPLIT"] = split
            C._check(C.lib.wisp_composite_loss(C._p(color), C._p(dens), C._p(delt), C._p(offs), R, S, bg_ptr, C._p(gts), 0, C._p(gc),
                                               C._p(gd), None, C._p(loss), C._p(ws), ws.numel(), stream), "composite_loss")
        return fn
    fns = {"split off": call("0"), "split on": call("1")}
    out = {}
    for name, fn in fns.items():
        fn(); torch.cuda.synchronize()
        out[name] = (gc.clone(), gd.clone(), loss.clone())
    for name in ("split on",):
        same = [torch.equal(a, b) for a, b in zip(out[name], out["split off"])]
        print(f"{name} against off: grad_color equal {same[0]}, grad_density equal {same[1]} "
              f"(max diff {float((out[name][1] - out['split off'][1]).abs().max()):.2e}), loss equal {same[2]}")
    report(f"composite_loss + loss_sum, {R} rays, {S} samples, longest {int(lens.max())} (us per call, {ROUNDS} interleaved rounds of {CALLS} calls)",
           timed(fns))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd")]
        {"composite": composite}[sys.argv[1]]()
    else:
        for part in ("composite",):
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), part], timeout=240).returncode
            if rc != 0:
                sys.exit(f"{part}: exit status {rc}; nothing more is started")
