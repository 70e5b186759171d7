"""Convert a textured OBJ to a coloured Structured Point Cloud file: the flow of examples/spc_browser/mesh2spc.py with this
package's pieces.

    python scripts/mesh2spc.py --obj_path OBJ [--output_path OUT.npz] [--level 8] [--num_samples 1000000] [--normalize none|sphere|aabb]

Steps: load_obj(load_materials=True); `num_samples` area-weighted surface samples that carry their face index and barycentric
weights (wisp.ops.mesh.sample_surface_barycentric); the per-corner texture coordinates interpolated with those weights; colours
from wisp.ops.mesh.sample_tex (one launch for all materials); octree and per-cell mean colour from
pointcloud_to_octree(points, level, attributes=rgba); an .npz with `octree` (u8) and `colors` (u8, flat RGBA, one quadruple
per cell of the finest level in point-hierarchy order) - the reference's file format, which scripts/render_spc.py and the
reference's SPC browser read.

Where this differs from the reference script: that one samples through Kaolin's `sample_points` and looks colours up with
Kaolin's nearest-texel `texture_mapping` in the first material's map only; their source is not part of the reference tree.  This
script looks colours up BILINEARLY through sample_tex (reflection padding, v up, every material, plain diffuse colours
included).  The lookup is therefore unpinned against Kaolin, like the other Kaolin leaves (oracle/__init__.py).
--normalize defaults to `none`: the reference does not normalise, a mesh is expected to lie inside [-1, 1]^3 already.
"""
import argparse
import os
import pathlib
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaolin-wisp_amd")]


def sample_colored_points(vertices, faces, texv, texf, mats, num_samples, device):
    """(points f32 [N,3], rgba f32 [N,4] in [0,1]) over the surface of the mesh, on `device`."""
    from wisp.ops import mesh as mesh_ops
    V, F = vertices.to(device), faces.to(device)
    points, fidx, w = mesh_ops.sample_surface_barycentric(V, F, num_samples)
    tf = texf.to(device)[fidx]                                           # [N,4]: three texture-vertex indices, material id
    if texv.shape[0]:
        corner_uv = texv.to(device)[tf[:, :3].clamp(min=0)]             # [N,3,2]; faces without coordinates have no map either
        uv = (w[:, :, None] * corner_uv).sum(dim=1)
    else:
        uv = torch.zeros(num_samples, 2, device=device)
    rgb = mesh_ops.sample_tex(uv.contiguous(), tf[:, 3].contiguous(), mats)
    return points, torch.cat([rgb, torch.ones_like(rgb[:, :1])], dim=1)


def convert_mesh_to_spc(mesh_path, level, output_path=None, num_samples=1000000, normalize='none', device='cuda'):
    """Writes the .npz and returns its path."""
    from wisp.ops import mesh as mesh_ops
    from wisp.ops.spc import pointcloud_to_octree
    vertices, faces, texv, texf, mats = mesh_ops.load_obj(mesh_path, load_materials=True)
    if not mats:
        raise NotImplementedError(f"mesh2spc: {mesh_path} defines no materials")
    print(f'Loaded mesh with {len(vertices)} vertices, {len(faces)} faces and {len(mats)} materials.')
    vertices, faces = mesh_ops.normalize(vertices, faces, normalize)
    points, rgba = sample_colored_points(vertices, faces, texv, texf, mats, num_samples, device)
    print(f'Sampled {points.shape[0]} points over the mesh surface.')
    octree, colors = pointcloud_to_octree(points, level, attributes=rgba)
    print(f'SPC generated with {colors.shape[0]} cells at level {level}.')
    record = dict(octree=octree.cpu().numpy().astype(np.uint8),
                  colors=(255 * colors.reshape(-1)).cpu().numpy().astype(np.uint8))
    if output_path is None:
        output_path = f'{pathlib.Path(mesh_path).stem}.npz'
    np.savez(output_path, **record)
    return output_path


def main(argv=None):
    ap = argparse.ArgumentParser(description='Converts a textured OBJ to an SPC (.npz with `octree` and `colors`).')
    ap.add_argument('--obj_path', type=str, required=True, help='input .obj; its .mtl gives diffuse colours / map_Kd textures')
    ap.add_argument('--output_path', type=str, default=None, help='output .npz (default: the obj file name in the working directory)')
    ap.add_argument('--level', type=int, default=8, help='octree depth: the SPC resolution is 2^level')
    ap.add_argument('--num_samples', type=int, default=1000000, help='surface samples that populate the SPC')
    ap.add_argument('--normalize', choices=('none', 'sphere', 'aabb'), default='none')
    ap.add_argument('--device', default='cuda')
    ap.add_argument('--seed', type=int, default=None)
    args = ap.parse_args(argv)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    out = convert_mesh_to_spc(args.obj_path, args.level, args.output_path, args.num_samples, args.normalize, args.device)
    print(f'mesh2spc finished successfully, output resides in {out}')
    return out


if __name__ == "__main__":
    main()
