"""Matcap shading (wisp/ops/shaders/matcap.py:20-72) with the texture fetch on the device: the reference builds a scipy
RegularGridInterpolator over the image and takes the texture coordinates through the host; here the bilinear lookup over the same
knots - linspace(0, 1, size) per axis of the transposed image, i.e. align_corners=True - is F.grid_sample.
pointlight_shadow_shader (the reference's second shader) is not provided."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from wisp.ops.geometric import spherical_envmap

_textures = {}


def matcap_sampler(path, device='cpu'):
    """The matcap image as a float tensor [1, C, A, B] on `device` with the first two image axes swapped (A = image width), as
    the reference transposes it; values 0 .. 255.  Cached per (path, modification time, device)."""
    from PIL import Image
    key = (os.path.abspath(path), os.path.getmtime(path), str(device))
    if key not in _textures:
        img = np.array(Image.open(path))
        if img.ndim == 2:
            img = img[..., None]
        tex = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 0, 2))).to(device)          # u8 [A, B, C]
        _textures[key] = tex.permute(2, 0, 1)[None].float().contiguous()
    return _textures[key]


def matcap_lookup(tex, uv):
    """bilinear texture values [N, C] (0 .. 255) at uv [N, 2] in [0, 1]: uv[:, 0] runs along A, uv[:, 1] along B of tex [1,C,A,B]"""
    # grid_sample's x indexes the LAST dimension (B), y the one before (A); align_corners: -1 / 1 are the first / last knot
    grid = torch.stack([uv[:, 1], uv[:, 0]], dim=-1).to(tex.dtype) * 2.0 - 1.0
    out = F.grid_sample(tex, grid[None, :, None, :], mode='bilinear', padding_mode='border', align_corners=True)
    return out[0, :, :, 0].T


def matcap_shader(rb, rays, matcap_path, mm=None):
    """rb.rgb <- the matcap texture at the sphere-map coordinates of (view direction, normal); mm: 3x3 rotation applied to the
    view directions.  Returns rb."""
    if not os.path.exists(matcap_path):
        raise Exception(f"The path [{matcap_path}] does not exist. Check your working directory or use an absolute path to "
                        "the matcap with --matcap-path")
    normal = rb.normal.clone()
    view = rays.dirs.clone()
    if mm is not None:
        shape = view.shape
        view = torch.mm(view.reshape(-1, 3), mm.to(normal.device).transpose(1, 0)).reshape(*shape)
    uv = spherical_envmap(view, normal)
    tex = matcap_sampler(matcap_path, device=normal.device)
    rb.rgb = (matcap_lookup(tex, uv)[..., :3] / 255.0).reshape(*view.shape)
    return rb
