"""Kernel time of wisp_mesh_closest_tex (csrc/mesh_tex.hip) against the same result composed from the reference's torch steps on
the device, one JSON line.

Scene: the procedural textured torus of scripts/train_sdf_tex.py (4608 triangles, three materials, two maps); N points near its
surface with the nearest triangle found once, outside the timed region (both sides start from the same `tidx`).
  * hip:   one wisp_mesh_closest_tex launch (closest point, barycentric weights, UV, colour);
  * torch: what wisp/ops/mesh/closest_tex.py:43-64 runs behind the search - closest_point_on_triangle over [N,3,3] fp64
           (wisp.ops.mesh's, the reference's arithmetic), barycentric_coordinates, the UV gather + weighted sum, and sample_tex's
           loop of one grid_sample per material with its TM.max() / mask.sum() read-backs.
Times come from device events around each side, alternating hip / torch for `--reps` repetitions after one warm-up each; the
medians are reported, with the largest colour difference between the two.

Usage: python scripts/bench_mesh_tex.py [--points N] [--reps R] [--out profiles/bench_mesh_tex.json]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd"), os.path.join(ROOT, "scripts")]


def torch_chain(mesh, points, tidx, texv, texf, mats):
    """The reference's steps behind the nearest-triangle search, on the device."""
    import torch.nn.functional as F
    from wisp.ops.mesh import barycentric_coordinates, closest_point_on_triangle
    tri = mesh.index_select(0, tidx)
    hit = closest_point_on_triangle(tri, points)
    bc = barycentric_coordinates(hit, tri[:, 0], tri[:, 1], tri[:, 2])
    tf = texf[tidx]
    tm = tf[..., 3]
    uv = (texv[tf[..., :3]] * bc.unsqueeze(-1)).sum(1)
    max_idx = tm.max()
    assert max_idx > -1
    rgb = torch.zeros(uv.shape[0], 3, device=uv.device)
    uv = uv * 2.0 - 1.0
    uv[..., 1] *= -1
    for i in range(int(max_idx) + 1):
        mask = tm == i
        if mask.sum() == 0:
            continue
        if 'diffuse_texname' not in mats[i]:
            if 'diffuse' in mats[i]:
                rgb[mask] = mats[i]['diffuse']
            continue
        grid = uv[mask]
        out = F.grid_sample(mats[i]['diffuse_texname'], grid.reshape(1, grid.shape[0], 1, 2), mode='bilinear',
                            padding_mode='reflection', align_corners=True)
        rgb[mask] = out[0, :, :, 0].permute(1, 0)
    return hit, rgb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_tex.py measures on the GPU"
    import train_sdf_tex
    import wisp._C as C
    from wisp.ops import mesh as mesh_ops
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as d:
        V, Fc, texv, texf, mats = mesh_ops.load_obj(train_sdf_tex.write_test_mesh(d), load_materials=True)
    V, Fc = mesh_ops.normalize(V, Fc, 'sphere')
    V, Fc, texv, texf = V.to(dev), Fc.to(dev), texv.to(dev), texf.to(dev)
    torch.manual_seed(0)
    points = mesh_ops.sample_near_surface(V, Fc, args.points, variance=0.02).double().contiguous()
    mesh = V.double()[Fc].contiguous()
    n = points.shape[0]
    tidx_f64 = C.mesh_to_sdf(points, mesh, with_triangle=True)[n:].contiguous()
    tidx = tidx_f64.long()
    bank = mesh_ops.TextureBank(mats)
    texels, records = bank.to(dev)
    dev_mats = {i: {k: (v[..., :3].permute(2, 0, 1)[None].contiguous().to(dev) if k == 'diffuse_texname' else v.to(dev))
                    for k, v in m.items()} for i, m in mats.items()}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    hip = lambda: C.mesh_closest_tex(points, mesh, tidx_f64, texv, texf, texels, records)      # noqa: E731
    ref = lambda: torch_chain(mesh, points, tidx, texv, texf, dev_mats)                        # noqa: E731
    timed(hip), timed(ref)
    t_hip, t_ref = [], []
    for _ in range(args.reps):
        ms, (hit_h, rgb_h) = timed(hip)
        t_hip.append(ms)
        ms, (hit_t, rgb_t) = timed(ref)
        t_ref.append(ms)
    rec = dict(metric="mesh_closest_tex", device=torch.cuda.get_device_name(0), points=n, triangles=int(Fc.shape[0]),
               materials=len(mats), reps=args.reps, hip_ms_median=round(float(np.median(t_hip)), 4),
               torch_chain_ms_median=round(float(np.median(t_ref)), 4), hip_ms_min=round(min(t_hip), 4),
               torch_chain_ms_min=round(min(t_ref), 4), speedup_of_medians=round(float(np.median(t_ref) / np.median(t_hip)), 2),
               max_rgb_difference=float((rgb_h - rgb_t).abs().max()), max_hit_difference=float((hit_h - hit_t).abs().max()))
    line = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
