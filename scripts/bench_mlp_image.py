"""Decoder forward / backward (hidden 64, bf16, per-ray view codes): the kernels that stage and convert the parameters in every
workgroup against the kernels that copy a prebuilt operand image, rounds interleaved in one process, at 1 024 samples (the part of a
launch that does not shrink with the batch) and at the headline's 2^18."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd")]
import torch
import wisp._C as C
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(0)
n = int(C.lib.wisp_nerf_mlp_param_count(32, 64, 4))
params = torch.randn(n, device=dev, generator=g) * 0.1
gp = torch.zeros_like(params)
image = C.nerf_mlp_operand_image(params, 32)
ROUNDS = 40
for S in (1024, 262144):
    R = max(64, S // 54)
    feats = (torch.randn(S, 32, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, device=dev, generator=g), dim=1)
    ridx = torch.sort(torch.randint(0, R, (S,), device=dev, generator=g)).values
    code = C.nerf_mlp_dir_code(dirs, 4)
    g_rgb = torch.randn(S, 3, device=dev, generator=g) * 1e-3
    g_den = torch.randn(S, 1, device=dev, generator=g) * 1e-3
    fns = {
        "fwd staged": lambda: C.nerf_mlp_forward(feats, None, params, 32, 64, 4, True, ray_code=(ridx, code)),
        "fwd image ": lambda: C.nerf_mlp_forward(feats, None, params, 32, 64, 4, True, ray_code=(ridx, code, image)),
        "bwd staged": lambda: C.nerf_mlp_backward(feats, None, params, g_rgb, g_den, 32, 64, 4, True, grad_params=gp, ray_code=(ridx, code)),
        "bwd image ": lambda: C.nerf_mlp_backward(feats, None, params, g_rgb, g_den, 32, 64, 4, True, grad_params=gp, ray_code=(ridx, code, image)),
        "build image": lambda: C.nerf_mlp_operand_image(params, 32),
    }
    ts = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(5): fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize(); ts[name].append(a.elapsed_time(b) * 1e3)
    print(f"S = {S} (us per call incl. launch, {ROUNDS} interleaved rounds; bwd = kernel + reduce launch)")
    for name, v in ts.items():
        v = sorted(v)
        print(f"  {name:12s} min {v[0]:7.1f}  median {v[len(v) // 2]:7.1f}  max {v[-1]:7.1f}", flush=True)
