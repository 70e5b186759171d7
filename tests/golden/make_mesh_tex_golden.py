"""Writes tests/golden/mesh_tex_ref.npz: the reference's closest_tex chain (wisp/ops/mesh/closest_tex.py, closest_point.py,
barycentric_coordinates.py, sample_tex.py), executed where it lies on the CPU over the textured torus of tests/mesh_tex_ref.py.
Nearest triangle and signed distance come from tests/mesh_sdf_oracle.py in place of the CUDA extension.  Data only: the scene
(vertices, faces, texture vertices / faces, the two maps and three Kd), 2000 points whose nearest triangle is unique, 37 points
with a forced triangle covering every Voronoi region, and for all 2037 the reference's tidx, dist, hit and rgb.  The GPU tests
have no reference tree; this file holds them to its output.

    python tests/golden/make_mesh_tex_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mesh_sdf_oracle as oracle                                       # noqa: E402
import mesh_tex_ref as ref                                             # noqa: E402


def main():
    V, F, texv, texf, mats = ref.scene()
    P = ref.unique_points(V, F)
    prep = oracle.Prepared(V[F])
    d = np.sqrt(np.sort(oracle.triangle_distsq(P, prep), axis=1)[:, :2])
    gap = (d[:, 1] - d[:, 0]) / np.maximum(d[:, 1], 1e-30)
    unique = gap > 1e-3
    print(f"unique nearest triangle (relative gap > 1e-3): {unique.sum()} of {len(P)}")
    assert unique.mean() >= 0.99
    Pf, tf = ref.forced_points(V, F)
    _, region = ref.closest_point_and_region(torch.from_numpy(V[F][tf]), torch.from_numpy(Pf))
    assert sorted(set(region.tolist())) == list(range(7)), region
    assert all(sorted(region[7 * k:7 * k + 7].tolist()) == list(range(7)) for k in range(5))
    pts = np.concatenate([P, Pf])
    rgb, hit, dist, tidx = ref.reference_closest_tex(torch.from_numpy(V.astype(np.float32)), torch.from_numpy(F),
                                                     torch.from_numpy(texv), torch.from_numpy(texf), mats,
                                                     torch.from_numpy(pts.astype(np.float32)), forced_tidx=tf)
    assert rgb.dtype == torch.float32 and hit.dtype == torch.float64 and np.array_equal(tidx.numpy()[-37:], tf)
    used = set(texf[tidx.numpy(), 3].tolist())
    assert used == {-1, 0, 1, 2}, used
    out = os.path.join(HERE, "mesh_tex_ref.npz")
    np.savez_compressed(out, vertices=V.astype(np.float32), faces=F.astype(np.int32), texv=texv, texf=texf.astype(np.int32),
                        map0=mats[0]['diffuse_texname'].numpy(), map2=mats[2]['diffuse_texname'].numpy(),
                        kd0=mats[0]['diffuse'].numpy(), kd1=mats[1]['diffuse'].numpy(), kd2=mats[2]['diffuse'].numpy(),
                        points=pts.astype(np.float32), unique=np.concatenate([unique, np.zeros(37, dtype=bool)]),
                        tidx=tidx.numpy().astype(np.int32), dist=dist.numpy(), hit=hit.numpy(), rgb=rgb.numpy())
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 300 * 1024


if __name__ == "__main__":
    main()
