"""PackedSPCTracer: rays against the cells of a Structured Point Cloud; every ray gets the colour of the first cell it hits
(tracer surface of wisp/tracers/packed_spc_tracer.py:7-90; black background, `bg_color` is ignored there and here).

Two paths behind the plain attribute `fused` (no constructor argument: the constructor's schema is the reference's):
  * modular - the reference body: every ray / cell intersection from the octree raytrace, the first of each ray through
    mark_pack_boundaries, colours from `nef(ridx_hit=..., channels="rgb")`, scattered into per-ray buffers;
  * fused - one `wisp_spc_first_hit` launch (csrc/spc.hip) that stops each ray at its first cell and writes depth, hit, rgb
    and alpha for every ray: no nugget list, no scan, no size read-back.  Same bits as the modular path.  Taken for an SPCField
    whose colours are contiguous f32 rows on the rays' GPU, at the finest level, when no gradient of the colours is wanted;
    anything else goes the modular way.
"""
import torch

from wisp.core import RenderBuffer
from wisp.tracers.base_tracer import BaseTracer
import wisp.ops.render as render_ops


class PackedSPCTracer(BaseTracer):
    def __init__(self):
        super().__init__(bg_color=(0.0, 0.0, 0.0))
        self.fused = True           # scripts/bench_spc_render.py: the fused path is ahead at level 8

    def get_supported_channels(self):
        return {"depth", "hit", "rgb", "alpha"}

    def get_required_nef_channels(self):
        return {"rgb"}

    @staticmethod
    def _fused_colors(nef, rays, extra_channels, lod_idx):
        """The colour table the fused launch can read, or None when this call has to take the modular path."""
        from wisp.models.nefs.spc_field import SPCField
        if not isinstance(nef, SPCField) or type(nef).rgba is not SPCField.rgba or extra_channels:
            return None
        blas, colors = nef.grid.blas, nef.colors
        if lod_idx != blas.max_level or not torch.is_tensor(colors):
            return None
        if (not colors.is_cuda or colors.device != rays.origins.device or colors.dtype != torch.float32 or colors.dim() != 2
                or colors.shape[1] < 3 or not colors.is_contiguous() or colors.shape[0] != int(blas.pyramid[0, lod_idx])):
            return None
        if colors.requires_grad and torch.is_grad_enabled():      # optimising the colours goes through autograd
            return None
        return colors

    def trace(self, nef, rays, channels, extra_channels, lod_idx=None):
        """RenderBuffer(depth [N,1], hit bool [N], rgb [N,3], alpha [N,1]); rays that hit no cell keep zeros."""
        N = rays.origins.shape[0]
        blas = nef.grid.blas
        if lod_idx is None:
            lod_idx = blas.max_level

        colors = self._fused_colors(nef, rays, extra_channels, lod_idx) if self.fused else None
        if colors is not None:
            import wisp._C as _C
            blas._to_device(rays.origins.device)
            _, depth, rgb, alpha, hit = _C.spc_first_hit(blas.octree, blas.points, blas.prefix, rays.origins, rays.dirs, lod_idx,
                                                         colors=colors, level_first=int(blas.pyramid[1, lod_idx]),
                                                         want_alpha=True, want_hit=True)
            return RenderBuffer(depth=depth, hit=hit, rgb=rgb, alpha=alpha)

        raytrace_results = blas.raytrace(rays, lod_idx, with_exit=False)
        ridx, pidx, depths = raytrace_results.ridx, raytrace_results.pidx, raytrace_results.depth

        first_hits_mask = render_ops.mark_pack_boundaries(ridx)
        first_hits_point = pidx[first_hits_mask]
        first_hits_ray = ridx[first_hits_mask].long()
        first_hits_depth = depths[first_hits_mask]

        color = nef(ridx_hit=first_hits_point.long(), channels="rgb")
        ray_colors = color.squeeze(1)
        dev = color.device
        depth = torch.zeros(N, 1, device=first_hits_depth.device)
        depth[first_hits_ray, :] = first_hits_depth
        alpha = torch.ones([color.shape[0], 1], device=dev)
        hit = torch.zeros(N, device=dev).bool()
        rgb = torch.zeros(N, 3, device=dev)
        out_alpha = torch.zeros(N, 1, device=dev)
        color = alpha * ray_colors

        hit[first_hits_ray] = alpha[..., 0] > 0.0
        rgb[first_hits_ray, :3] = color
        out_alpha[first_hits_ray] = alpha
        return RenderBuffer(depth=depth, hit=hit, rgb=rgb, alpha=out_alpha)
