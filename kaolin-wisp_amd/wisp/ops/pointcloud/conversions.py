"""Depth images -> coloured point cloud (wisp/ops/pointcloud/conversions.py:12-42).  Torch code on the inputs' device."""
import torch


def create_pointcloud_from_images(rgbs, masks, rays, depths):
    """Per view i: the pixels where masks[i] is set, lifted to origins + dirs * depth, with their colours.

    rgbs: list of [H, W, >=3]; masks: list of [H, W, 1] (or [H, W]); rays: list of wisp.core.Rays with [H, W, 3] origins and
    dirs; depths: list of [H, W, 1].  Returns (coordinates [M, 3], colours [M, 3]), views concatenated in order."""
    cloud_coords = []
    cloud_colors = []
    for i in range(len(rgbs)):
        mask = masks[i].bool()
        h, w = mask.shape[:2]
        mask = mask.reshape(h, w)
        depth = depths[i].reshape(h, w, 1)
        coords = rays[i].origins[mask] + rays[i].dirs[mask] * depth[mask]
        colors = rgbs[i][mask]
        cloud_coords.append(coords.reshape(-1, 3))
        cloud_colors.append(colors[..., :3].reshape(-1, 3))
    return torch.cat(cloud_coords, dim=0), torch.cat(cloud_colors, dim=0)
