"""Point-cloud normalisation (wisp/ops/pointcloud/processing.py:12-38).  Torch code on the input's device."""
import torch


def normalize_pointcloud(coords, return_scale=False):
    """Centre the cloud's bounding box on the origin and scale by 1 / max over the centred COORDINATES (the largest positive
    coordinate, not the largest distance - as the reference does), which puts the cloud inside [-1, 1]^3.
    Returns the coordinates [N, 3], and with `return_scale` also the centre [3] and the scale (0-d tensor)."""
    coords_max, _ = torch.max(coords, dim=0)
    coords_min, _ = torch.min(coords, dim=0)
    coords_center = (coords_max + coords_min) / 2.0
    coords = coords - coords_center
    max_dist = torch.max(coords)
    coords_scale = 1.0 / max_dist
    coords *= coords_scale
    if return_scale:
        return coords, coords_center, coords_scale
    return coords
