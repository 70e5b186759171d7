"""Wavefront OBJ + MTL with texture coordinates and diffuse materials: what wisp/ops/mesh/load_obj.py:85-115 takes from
tinyobjloader.  Only what the colour path reads is parsed - `vt`, the `v/vt/vn` face tokens, `mtllib`, `usemtl`, and from the
.mtl `newmtl`, `Kd` and `map_Kd`.  tinyobjloader itself is not a dependency, so the parse is held to hand-written expectations
(tests/test_mesh_tex_host.py), not to the reference's output."""
import os

import numpy as np
import torch

from wisp.ops.image.io import load_u8


def _load_map(path):
    """f32 [H,W,C] = u8 / 255 with the file's own channel count, as load_mat (load_obj.py:43-50)."""
    img = load_u8(path)
    if img.shape[2] < 3:
        raise ValueError(f"{path}: a diffuse map needs 3 or 4 channels, this one has {img.shape[2]} (a grey map's width would be "
                         f"sliced as if it were the channels)")
    return torch.from_numpy(img.astype(np.float32) / np.float32(255.0))


def load_mtl(path, folder=None):
    """[(name, {'diffuse': f32[3], 'diffuse_texname': f32[H,W,3|4]})] in file order.  Kd defaults to (0, 0, 0) (tinyobjloader
    always has a diffuse); map_Kd paths are relative to `folder` (the OBJ's, as the reference joins them; default:
    the .mtl's); map_Kd options (-s, -o, ...) raise ValueError."""
    mats, cur = [], None
    folder = os.path.dirname(path) if folder is None else folder
    with open(path) as f:
        for line in f:
            p = line.split()
            if not p or p[0].startswith("#"):
                continue
            if p[0] == "newmtl":
                cur = {'diffuse': torch.zeros(3, dtype=torch.float32)}
                mats.append((" ".join(p[1:]), cur))
            elif cur is None:
                continue
            elif p[0] == "Kd":
                if len(p) < 4:
                    raise ValueError(f"{path}: Kd needs three values: {line.strip()!r}")
                cur['diffuse'] = torch.tensor([float(p[1]), float(p[2]), float(p[3])], dtype=torch.float32)
            elif p[0] == "map_Kd":
                if len(p) < 2:
                    raise ValueError(f"{path}: map_Kd without a file name")
                if any(tok.startswith("-") for tok in p[1:]):
                    raise ValueError(f"{path}: map_Kd options are not supported: {line.strip()!r}")
                name = line.strip()[len("map_Kd"):].strip()
                cur['diffuse_texname'] = _load_map(os.path.join(folder, name.replace("\\", "/")))
    return mats


def load_obj_with_materials(fname: str):
    """(vertices f32 [V,3], faces i64 [F,3], texv f32 [TV,2], texf i64 [F,4], mats): texf holds three texture-vertex indices (-1
    where the face token has none) and the material id (position of the `usemtl` name in `mtllib` order, -1 before any
    `usemtl`); polygons are fan-triangulated and every triangle keeps its polygon's material; negative indices are relative
    to the records read so far.  mats: {id: {'diffuse': ..., 'diffuse_texname': ...}}."""
    verts, texv, faces, texf = [], [], [], []
    names, mats, material = {}, {}, -1
    folder = os.path.dirname(fname)
    with open(fname) as f:
        for lineno, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                verts.append((float(p[1]), float(p[2]), float(p[3])))
            elif p[0] == "vt":
                texv.append((float(p[1]), float(p[2]) if len(p) > 2 else 0.0))
            elif p[0] == "mtllib":
                for lib in p[1:]:
                    for name, mat in load_mtl(os.path.join(folder, lib), folder):
                        if name not in names:
                            names[name] = len(names)
                        mats[names[name]] = mat
            elif p[0] == "usemtl":
                name = " ".join(p[1:])
                if name not in names:
                    raise ValueError(f"{fname}:{lineno}: usemtl {name!r} is not defined by any mtllib read so far")
                material = names[name]
            elif p[0] == "f":
                vi, ti = [], []
                for tok in p[1:]:
                    parts = tok.split("/")
                    i = int(parts[0])
                    vi.append(i - 1 if i > 0 else len(verts) + i)
                    if len(parts) > 1 and parts[1] != "":
                        t = int(parts[1])
                        ti.append(t - 1 if t > 0 else len(texv) + t)
                    else:
                        ti.append(-1)
                for k in range(1, len(vi) - 1):
                    faces.append((vi[0], vi[k], vi[k + 1]))
                    texf.append((ti[0], ti[k], ti[k + 1], material))
    if not verts or not faces:
        raise ValueError(f"{fname}: no geometry (need 'v' and 'f' records)")
    texv = torch.tensor(texv, dtype=torch.float32).reshape(-1, 2)
    texf = torch.tensor(texf, dtype=torch.int64).reshape(-1, 4)
    for i, mat in mats.items():                           # a lookup in a map needs all three texture coordinates
        rows = texf[texf[:, 3] == i, :3]
        if 'diffuse_texname' in mat and bool(((rows < 0) | (rows >= texv.shape[0])).any()):
            raise ValueError(f"{fname}: a face of material {i}, which has a diffuse map, lacks a (valid) texture coordinate")
    return torch.tensor(verts, dtype=torch.float32), torch.tensor(faces, dtype=torch.int64), texv, texf, mats
