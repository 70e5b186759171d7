"""Surface colour of a textured mesh: TextureBank, sample_tex and closest_tex (wisp/ops/mesh/sample_tex.py:12-58,
closest_tex.py:16-64).  The reference chains the closest point on the chosen triangle, barycentric coordinates, the UV
interpolation and one grid_sample per material in torch, with two host read-backs per material; here everything behind the
nearest-triangle search is one HIP launch (csrc/mesh_tex.hip; include/wisp_hip.h spells its arithmetic out)."""
import numpy as np
import torch


class TextureBank:
    """The diffuse maps and colours of a reference-format materials dict `{i: {'diffuse': f32[3], 'diffuse_texname':
    f32[H,W,3|4]}}` as the two device buffers the kernels read: `texels` f32 [T,3], all maps row-major one after another, and
    `records` (one wisp_tex_material per id 0 .. max id: offset, height, width, Kd, has-map flag).  An id the dict does not
    hold, and a material with neither entry, gets Kd = 0 and no map.  Built once; `to(device)` copies once per device."""

    def __init__(self, materials: dict):
        from wisp._C import TexMaterial
        ids = sorted(int(k) for k in materials)
        if ids and ids[0] < 0:
            raise ValueError(f"TextureBank: material ids must be >= 0, got {ids[0]}")
        recs = (TexMaterial * (ids[-1] + 1 if ids else 0))()
        maps, offset = [], 0
        for i in ids:
            mat = materials[i]
            if 'diffuse' in mat:
                kd = torch.as_tensor(mat['diffuse'], dtype=torch.float32).reshape(-1)
                if kd.numel() != 3:
                    raise ValueError(f"TextureBank: material {i}: 'diffuse' must hold 3 values, got {kd.numel()}")
                recs[i].kd[:] = [float(v) for v in kd]
            if 'diffuse_texname' in mat:
                img = torch.as_tensor(mat['diffuse_texname'], dtype=torch.float32)
                if img.ndim != 3 or img.shape[2] < 3 or img.shape[0] < 1 or img.shape[1] < 1:
                    raise ValueError(f"TextureBank: material {i}: the diffuse map must be [H>=1, W>=1, 3|4], got {tuple(img.shape)}")
                recs[i].offset, recs[i].height, recs[i].width, recs[i].has_map = offset, img.shape[0], img.shape[1], 1
                maps.append(img[..., :3].reshape(-1, 3).cpu())
                offset += img.shape[0] * img.shape[1]
        self.num_materials = len(recs)
        self.texels = torch.cat(maps).contiguous() if maps else torch.zeros(0, 3, dtype=torch.float32)
        self.records = torch.from_numpy(np.frombuffer(bytes(recs), dtype=np.uint8).copy())
        self._on = {}

    def to(self, device):
        """(texels, records) on `device`."""
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = (self.texels.to(device), self.records.to(device))
        return self._on[device]

    def __getstate__(self):
        state = self.__dict__.copy()
        state['_on'] = {}
        return state


def as_bank(materials) -> TextureBank:
    return materials if isinstance(materials, TextureBank) else TextureBank(materials)


def sample_tex(Tp: torch.Tensor, TM: torch.Tensor, materials):
    """RGB f32 [N,3] of the UV coordinates `Tp` [N,2] in the materials `TM` [N] (sample_tex.py:12-58): the material's diffuse
    colour, or its diffuse map looked up bilinearly under reflection padding with v pointing up; zero for an id < 0 or without
    a record.  `materials`: the materials dict or a TextureBank.  One launch for all materials."""
    import wisp._C as _C
    Tp = _C._need(Tp, torch.float32, "Tp")
    texels, records = as_bank(materials).to(Tp.device)
    return _C.mesh_sample_tex(Tp.reshape(-1, 2), TM.to(Tp.device).reshape(-1), texels, records)


def closest_tex(V: torch.Tensor, F: torch.Tensor, TV: torch.Tensor, TF: torch.Tensor, materials, points: torch.Tensor,
                split_size: int = 10 ** 6):
    """(rgb f32 [N,3], closest point on the mesh f64 [N,3], signed distance f64 [N]) of `points` against the textured mesh
    (V [#V,3] on the GPU, F [#F,3], TV f32 [#TV,2], TF i64 [#F,4] = three texture-vertex indices and a material id); the other
    inputs are moved to V's device, as the reference does (closest_tex.py:16-64).  Each split runs the nearest-triangle kernel,
    then one launch for the rest; how the points are split does not change a bit of the result.  `materials`: the materials dict or a TextureBank."""
    import wisp._C as _C
    dev = _C._need(V, name="V").device
    mesh = V.to(torch.float64)[F.to(dev, torch.int64)].contiguous()
    points = points.to(dev, torch.float64).reshape(-1, 3)
    texv = TV.to(dev, torch.float32).reshape(-1, 2).contiguous()
    texf = TF.to(dev, torch.int64).contiguous()
    texels, records = as_bank(materials).to(dev)
    rgbs, hits, dists = [], [], []
    for p in (torch.split(points, max(int(split_size), 1)) if points.shape[0] else ()):
        p = p.contiguous()
        n = p.shape[0]
        out = _C.external.mesh_to_sdf_triangle_cuda(p, mesh)[0]
        hit, rgb = _C.mesh_closest_tex(p, mesh, out[n:], texv, texf, texels, records)
        rgbs.append(rgb)
        hits.append(hit)
        dists.append(out[:n])
    if not rgbs:
        return (torch.zeros(0, 3, dtype=torch.float32, device=dev), points.new_zeros(0, 3), points.new_zeros(0))
    return torch.cat(rgbs), torch.cat(hits), torch.cat(dists)
