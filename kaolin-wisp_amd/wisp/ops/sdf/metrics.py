"""Metrics of signed-distance fields (wisp/ops/sdf/metrics.py:12-29).  The reference's compute_sparse_sdf_iou (:32-57) is left
out: nothing calls it, and it queries the grid with the ground-truth distances where it means the coordinates."""
import torch


def sdf_iou_counts(pred, gts):
    """(intersection, union) of the sets pred < 0 and gts < 0, as an int64 tensor [2] on pred's device (no host read-back)."""
    inside_pred, inside_gts = pred < 0, gts < 0
    return torch.stack([(inside_pred & inside_gts).sum(), (inside_pred | inside_gts).sum()]).to(torch.int64)


def compute_sdf_iou(pred, gts):
    """Intersection over union of the interiors (distance < 0) of a predicted and a ground-truth field, 0 .. 100, as a Python
    float.  Both sums are taken in float32, as the reference takes them (exact below 2^24 points); an empty union divides by
    zero, as it does there."""
    inside_pred, inside_gts = pred < 0, gts < 0
    area_union = torch.sum((inside_pred | inside_gts).float()).item()
    area_intersect = torch.sum((inside_pred & inside_gts).float()).item()
    return 100.0 * (area_intersect / area_union)
