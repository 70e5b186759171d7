"""Geometric helpers (wisp/ops/geometric.py): the depth-bound search of the SDF tracer (:15-22) and the sphere samplers the
radiance field's prune draws its view directions from (:25-62), and the pixel-coordinate grid of the image application (:65-99)."""
import numpy as np
import torch


def find_depth_bound(query, nug_depth, info, curr_idxes=None):
    """For every ray, the nugget that contains (or first lies beyond) the query depth, searched forward from the
    ray's current nugget; -1 if none.  query [P,1], nug_depth [M,2], info = first-hit flags [M], curr_idxes int32 [P]."""
    import wisp._C as _C
    if curr_idxes is None:
        curr_idxes = torch.nonzero(info)[..., 0].int()
    return _C.find_depth_bound(query.reshape(-1).contiguous(), curr_idxes.contiguous(), nug_depth.contiguous())


def sample_unif_sphere(n):
    """n points uniformly on the unit sphere, float64 [n, 3] from numpy's global generator (wisp/ops/geometric.py:25-39):
    z uniform in [-1, 1], azimuth uniform in [0, 2 pi) - two draws per point, all z first."""
    u = np.random.rand(2, n)
    z = 1 - 2 * u[0, :]
    r = np.sqrt(1. - z * z)
    phi = 2 * np.pi * u[1, :]
    return np.array([r * np.cos(phi), r * np.sin(phi), z]).transpose()


def sample_fib_sphere(n):
    """n points spread evenly over the unit sphere by the golden-ratio spiral, in spiral order (wisp/ops/geometric.py:42-62)."""
    k = np.arange(0, n, dtype=float) + 0.5
    polar = np.arccos(1 - 2 * k / n)
    azimuth = 2. * np.pi * k / ((1 + 5 ** 0.5) / 2)
    return np.array([np.cos(azimuth) * np.sin(polar), np.sin(azimuth) * np.sin(polar), np.cos(polar)]).transpose()


def normalized_grid(height, width, jitter=False, device='cuda', use_aspect=True):
    """grid[row, col] -> (x, y) of a normalized window, [height, width, 2] (wisp/ops/geometric.py:65-99): x runs -1 .. 1 along the
    width, y runs 1 .. -1 down the height; `jitter` moves every line by up to half a pixel (x drawn before y), `use_aspect`
    stretches the longer side by the aspect ratio."""
    lines = {'x': torch.linspace(-1, 1, steps=width, device=device), 'y': torch.linspace(1, -1, steps=height, device=device)}
    if jitter:
        for axis, count in (('x', width), ('y', height)):
            lines[axis] += (2.0 * torch.rand(count, device=device) - 1.0) * (1. / count)
    if use_aspect and width != height:
        longer, ratio = ('x', width / height) if width > height else ('y', height / width)
        lines[longer] = lines[longer] * ratio
    # every row repeats the x line, every column the y line
    return torch.stack([lines['x'][None, :].expand(height, width), lines['y'][:, None].expand(height, width)], dim=-1)


def normalized_slice(height, width, dim=0, depth=0.0, device='cuda'):
    """3D points of an axis-aligned cutting plane, [height, width, 3] (wisp/ops/geometric.py:102-127): the normalized window's
    (x, y) fill the two axes other than `dim` in ascending order, `dim` holds `depth`, and the y AXIS OF SPACE is mirrored at the
    end.  Like the reference it hands `device` to normalized_grid positionally, i.e. as its `jitter` flag: every device string
    jitters the window by up to half a pixel and the window lands on normalized_grid's default device ('cuda'), while the
    `depth` column is made on `device` - reproduced, because the reference's slices look the way they do through it."""
    window = normalized_grid(height, width, device)
    if dim not in (0, 1, 2):
        raise ValueError("dim is invalid!")
    plane = torch.ones(height, width, 1, device=device) * depth
    parts = [window[..., 0:1], window[..., 1:2]]
    parts.insert(dim, plane)
    pts = torch.cat(parts, dim=-1)
    pts[..., 1] *= -1
    return pts


def spherical_envmap(ray_dir, normal):
    """Matcap (sphere-map) texture coordinates [N, 2] in [0, 1] from viewing directions and normals [..., 3]
    (wisp/ops/geometric.py:130-155): reflect the screen-space direction (z flipped) about the normal, r = d - 2 (d . n) n, shift
    z by -1, uv = 1 - (r_xy / (2 |r|) + 0.5), clipped; NaN (a zero-length r) becomes 0."""
    d = ray_dir.clone()
    d[..., 2] *= -1
    r = d - 2.0 * torch.sum(normal * d, dim=-1, keepdim=True) * normal
    r[..., 2] -= 1.0
    m = 2.0 * torch.sqrt(torch.sum(r ** 2, dim=-1, keepdim=True))
    uv = 1.0 - ((r[..., :2] / m) + 0.5)
    uv = torch.clip(uv[..., :2].reshape(-1, 2), 0.0, 1.0)
    uv[torch.isnan(uv)] = 0
    return uv
