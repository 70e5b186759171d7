"""Evaluation of signed-distance fields: the IoU metric of the reference (wisp/ops/sdf/metrics.py) and one-launch queries of an
nglod-shaped field (csrc/sdf_eval.hip over an OctreeGrid, csrc/hash_sdf_eval.hip over a HashGrid, csrc/triplane_sdf_eval.hip over a
TriplanarGrid) with the modular path as the fallback for every other shape."""
import torch

from wisp.ops.differential import finitediff_gradient
from .metrics import compute_sdf_iou, sdf_iou_counts

__all__ = ["compute_sdf_iou", "sdf_iou_counts", "fused_sdf_field", "is_textured", "sdf_query", "sdf_fd_gradient"]


def is_textured(nef):
    """does the field answer 'rgb' and 'sdf' from one forward function (NeuralSDFTex)?"""
    return any({"rgb", "sdf"} <= set(ch) for ch in getattr(nef, "_forward_functions", {}).values())


def fused_sdf_field(nef, lod_idx=None):
    """The tensors wisp_sdf_query / wisp_sdf_fd_gradient need for `nef` at `lod_idx`, or None when the field is not the shape
    they are built for.  The shape rules are those of the fused march (PackedSDFTracer._fused_field / _fused_field_tex): a plain
    NeuralSDF or NeuralSDFTex on the GPU over an OctreeGrid with 16 'sum'-med channels and linear interpolation, the raw position
    (or, textured, nothing) in front of the features, one hidden relu layer of at most 256 units with biases, lod_idx >= 1.
    WISP_SDF_FUSED=0 switches the kernels off.  A textured field keeps all four output rows in module order (rgb logits, then
    the distance).  A plain NeuralSDF over a 3-D HashGrid (nglod_hash.yaml) yields a dict of kind 'hash' for
    wisp_hash_sdf_query / wisp_hash_sdf_fd_gradient (PackedSDFTracer._fused_field_hash: feature_dim 2 / 4 / 8, at most 32
    feature columns, the same decoder shape); there every lod_idx of the grid is served, 0 included.  A plain NeuralSDF over a
    TriplanarGrid (nglod_triplanar.yaml) yields a dict of kind 'triplane' for wisp_triplane_sdf_query /
    wisp_triplane_sdf_fd_gradient (PackedSDFTracer._fused_field_triplane: f32 planes, at most 48 feature columns, the same decoder
    shape; 'sum' at every lod_idx, 'cat' at the last one)."""
    from wisp.tracers.packed_sdf_tracer import PackedSDFTracer
    grid = getattr(nef, "grid", None)
    if grid is None or not hasattr(grid, "num_lods"):
        return None
    if lod_idx is None:
        lod_idx = grid.num_lods - 1
    fld = PackedSDFTracer._fused_field(nef, lod_idx)
    if fld is None:
        return None
    lout = nef.decoder.lout
    if lout.out_features == 4:
        fld = dict(fld, w2=lout.weight.detach().float().contiguous(), b2=lout.bias.detach().float().contiguous())
    return fld


def _distance_rows(fld):
    """the same field with the distance row alone (the last one): what the gradient differences"""
    if fld["b2"].numel() == 1:
        return fld
    hidden = fld["w1"].shape[0]
    return dict(fld, w2=fld["w2"].reshape(-1, hidden)[-1].contiguous(), b2=fld["b2"][-1:].contiguous())


def sdf_query(nef, coords, lod_idx=None, gts=None, counts=None):
    """What `nef` answers at coords [n,3]: the distance [n,1] of a NeuralSDF, [rgb, distance] [n,4] of a textured field.  With
    gts [n] or [n,1] and counts (int64 [2] on the device) the intersection / union counts of (pred < 0), (gts < 0) are ADDED to
    counts - compute_sdf_iou's two sums without its read-back.  One launch on an nglod-shaped field (fused_sdf_field), else
    `nef(...)`.  (A textured field WITHOUT position input gets three zero weight columns for the position: exact for finite
    coordinates, NaN for non-finite ones, where the module ignores the position.)"""
    import wisp._C as _C
    if (counts is None) != (gts is None):
        raise ValueError("sdf_query: `gts` and `counts` go together")
    flat = coords.reshape(-1, 3)
    fld = fused_sdf_field(nef, lod_idx) if flat.is_cuda and flat.shape[0] > 0 else None
    textured = is_textured(nef)
    with torch.no_grad():
        if fld is not None:
            out = _C.sdf_query(flat, fld, gts=gts, counts=counts)
            if out.shape[1] == 4:
                out = torch.cat([torch.sigmoid(out[:, :3]), out[:, 3:4]], dim=1)
        else:
            if textured:
                out = torch.cat(list(nef(coords=flat, lod_idx=lod_idx, channels=["rgb", "sdf"])), dim=-1)
            else:
                out = nef(coords=flat, lod_idx=lod_idx, channels="sdf")
            if counts is not None:
                counts += sdf_iou_counts(out[:, -1], gts.reshape(-1).to(out.device)).to(counts.device)
    return out.reshape(*coords.shape[:-1], out.shape[-1])


def sdf_fd_gradient(nef, coords, lod_idx=None, eps=0.005):
    """Central-difference gradient [n,3] of the field's distance at coords [n,3] (finitediff_gradient on the 'sdf' channel): one
    launch on an nglod-shaped field, else six `nef(...)` queries."""
    import wisp._C as _C
    flat = coords.reshape(-1, 3)
    fld = fused_sdf_field(nef, lod_idx) if flat.is_cuda and flat.shape[0] > 0 else None
    with torch.no_grad():
        if fld is not None:
            grad = _C.sdf_fd_gradient(flat, _distance_rows(fld), eps)
        else:
            grad = finitediff_gradient(flat, lambda x: nef(coords=x, lod_idx=lod_idx, channels="sdf"), eps)
    return grad.reshape(coords.shape)
