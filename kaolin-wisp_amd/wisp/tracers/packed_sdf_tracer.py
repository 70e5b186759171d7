"""PackedSDFTracer: sphere tracing of a neural SDF through the occupied cells of its octree (NGLOD rendering).

Same tracer surface and stepping rule as wisp/tracers/packed_sdf_tracer.py:21-175, organised differently: the marching
state lives in a small struct of flat device buffers, and everything a marching iteration does apart from the field query
(advance, convergence and far-plane tests, search of the next occupied cell, jump to its entry point, new query position)
is ONE HIP launch (`wisp_sphere_trace_step`, csrc/render.hip) instead of ~25 masked tensor ops.  The octree raytrace and
the first-hit marking are HIP kernels too (csrc/spc.hip).
"""
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from wisp.core import RenderBuffer
from wisp.ops.differential import finitediff_gradient
from wisp.tracers.base_tracer import BaseTracer
import wisp.ops.render as render_ops


@dataclass
class _MarchState:
    """Per-pack (ray that owns at least one nugget) marching state; every tensor has leading dimension P."""
    ray: torch.Tensor          # int64  ray index of the pack
    o: torch.Tensor            # f32 [P,3] origin
    d: torch.Tensor            # f32 [P,3] direction
    t: torch.Tensor            # f32 [P]   current depth
    x: torch.Tensor            # f32 [P,3] current position
    dist: torch.Tensor         # f32 [P]   last (scaled) signed distance
    dist_prev: torch.Tensor    # f32 [P]
    active: torch.Tensor       # u8  [P]   still marching
    hit: torch.Tensor          # u8  [P]   converged on the surface
    nug: torch.Tensor          # i32 [P]   current nugget
    nug_next: torch.Tensor     # i32 [P]   scratch (double buffer)
    cell: torch.Tensor         # i64 [P]   point-hierarchy index of the current cell


class PackedSDFTracer(BaseTracer):
    def __init__(self, num_steps=1024, step_size=0.8, min_dis=0.0003):
        """num_steps: marching iterations at most; step_size: multiplier on every SDF step; min_dis: convergence distance."""
        super().__init__()
        self.num_steps = num_steps
        self.step_size = step_size
        self.min_dis = min_dis

    def get_supported_channels(self):
        return {"depth", "normal", "xyz", "hit", "rgb", "alpha"}

    def get_required_nef_channels(self):
        return {"sdf"}

    # ------------------------------------------------------------------ pieces of trace()
    @staticmethod
    def _start(rays, ridx, pidx, depth):
        first = render_ops.mark_pack_boundaries(ridx)
        nug = torch.nonzero(first)[..., 0].int()
        ray = ridx[first].long()
        o, d = rays.origins[ray].contiguous(), rays.dirs[ray].contiguous()
        t = depth[first][..., 0].contiguous()
        P = ray.shape[0]
        dev = o.device
        return _MarchState(ray=ray, o=o, d=d, t=t, x=torch.addcmul(o, d, t[:, None]), dist=torch.zeros(P, device=dev),
                           dist_prev=torch.zeros(P, device=dev), active=torch.ones(P, dtype=torch.uint8, device=dev),
                           hit=torch.zeros(P, dtype=torch.uint8, device=dev), nug=nug, nug_next=torch.empty_like(nug),
                           cell=pidx[first].long())

    @staticmethod
    def _query(nef, st, lod_idx, scale):
        """scaled SDF at the active positions, scattered into st.dist."""
        sel = st.active.bool()
        if bool(sel.any()):
            sdf = nef(coords=st.x[sel], lod_idx=lod_idx, pidx=st.cell[sel], channels="sdf") * scale
            st.dist[sel] = sdf.reshape(-1).to(st.dist.dtype)
        return sel

    # ------------------------------------------------------------------ fused iteration (field query inside the launch)
    @staticmethod
    def _fused_decoder(nef, outputs):
        """the decoder shape every fused march is built for: one hidden relu Linear of at most 256 units and an output
        Linear of `outputs` rows, both with bias, no skip connection"""
        dec = nef.decoder
        return (nef.activation_type == 'relu' and nef.num_layers == 1 and len(dec.layers) == 1 and not dec.skip
                and type(dec.layers[0]) is torch.nn.Linear and type(dec.lout) is torch.nn.Linear
                and dec.layers[0].bias is not None and dec.lout.bias is not None and dec.lout.out_features == outputs
                and dec.layers[0].out_features <= 256)

    @staticmethod
    def _fused_field(nef, lod_idx):
        """The tensors wisp_sdf_trace_step_fused needs, or None when the field is not the shape it is built for: a plain
        NeuralSDF (nglod_octree.yaml) - OctreeGrid with 16 'sum'-med feature channels, linear interpolation, raw position
        input without embedding, one hidden relu layer with bias.  A NeuralSDFTex of the same shape (four outputs; features
        alone, or the raw position in front of them) marches on its fourth output row.  Anything else marches through
        `nef(...)` per iteration.  A plain NeuralSDF over a HashGrid (nglod_hash.yaml) has a branch of its own:
        _fused_field_hash; so has one over a TriplanarGrid (nglod_triplanar.yaml): _fused_field_triplane."""
        from wisp.models.grids.hash_grid import HashGrid
        from wisp.models.grids.octree_grid import OctreeGrid
        from wisp.models.grids.triplanar_grid import TriplanarGrid
        from wisp.models.nefs.neural_sdf import NeuralSDF
        from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
        import os
        if os.environ.get("WISP_SDF_FUSED", "1") == "0":
            return None
        if type(nef.grid) is HashGrid:
            return PackedSDFTracer._fused_field_hash(nef, lod_idx) if type(nef) is NeuralSDF else None
        if type(nef.grid) is TriplanarGrid:
            return PackedSDFTracer._fused_field_triplane(nef, lod_idx) if type(nef) is NeuralSDF else None
        if type(nef.grid) is not OctreeGrid:
            return None
        if type(nef) is NeuralSDFTex:
            return PackedSDFTracer._fused_field_tex(nef, lod_idx)
        if type(nef) is not NeuralSDF:
            return None
        g, dec = nef.grid, nef.decoder
        if (g.multiscale_type != 'sum' or g.interpolation_type != 'linear' or g.feature_dim != 16 or lod_idx < 1
                or not nef.position_input or not isinstance(nef.pos_embedder, torch.nn.Identity)
                or not PackedSDFTracer._fused_decoder(nef, 1) or not g.features[0].is_cuda):
            return None
        n = lod_idx + 1
        feats = [g.features[i].detach().contiguous() for i in range(n)]
        if any(f.dtype != feats[0].dtype or f.shape[1] != 16 for f in feats):
            return None
        g._sync_device(feats[0].device)
        return dict(feats=feats, levels=[int(l) for l in g.active_lods[:n]], half_round=bool(g.half_features),
                    w1=dec.layers[0].weight.detach().float().contiguous(), b1=dec.layers[0].bias.detach().float().contiguous(),
                    w2=dec.lout.weight.detach().float().reshape(-1).contiguous(), b2=dec.lout.bias.detach().float().contiguous(),
                    octree=g.blas.octree, exsum=g.blas.prefix, points=g.blas.points, trinkets=g.trinkets.int().contiguous())

    @staticmethod
    def _fused_field_tex(nef, lod_idx):
        """_fused_field for a NeuralSDFTex: the distance is the decoder's fourth output, so the kernel gets that row of the
        output layer; the colour rows are not needed to march."""
        g, dec = nef.grid, nef.decoder
        with_pos = bool(nef.position_input)
        if (g.multiscale_type != 'sum' or g.interpolation_type != 'linear' or g.feature_dim != 16 or lod_idx < 1
                or (with_pos and not (isinstance(nef.pos_embedder, torch.nn.Identity) and nef.pos_embed_dim == 3))
                or (not with_pos and nef.embedder_type != 'none')
                or not PackedSDFTracer._fused_decoder(nef, 4) or dec.layers[0].in_features != (3 if with_pos else 0) + 16
                or not g.features[0].is_cuda):
            return None
        n = lod_idx + 1
        feats = [g.features[i].detach().contiguous() for i in range(n)]
        if any(f.dtype != feats[0].dtype or f.shape[1] != 16 for f in feats):
            return None
        g._sync_device(feats[0].device)
        w1 = dec.layers[0].weight.detach().float()
        if not with_pos:
            # the kernel's input layout is [position, features]: three zero columns in front make the position's share of every
            # dot product fmaf(0, x, a) == a exactly for the finite coordinates a march produces - the feature-only result
            w1 = torch.cat([torch.zeros(w1.shape[0], 3, dtype=w1.dtype, device=w1.device), w1], dim=1)
        return dict(feats=feats, levels=[int(l) for l in g.active_lods[:n]], half_round=bool(g.half_features),
                    w1=w1.contiguous(), b1=dec.layers[0].bias.detach().float().contiguous(),
                    w2=dec.lout.weight.detach().float()[3].contiguous(), b2=dec.lout.bias.detach().float()[3:4].contiguous(),
                    octree=g.blas.octree, exsum=g.blas.prefix, points=g.blas.points, trinkets=g.trinkets.int().contiguous())

    @staticmethod
    def _fused_field_hash(nef, lod_idx):
        """_fused_field for a plain NeuralSDF over a 3-D HashGrid (csrc/hash_sdf_eval.hip): feature_dim 2, 4 or 8, at most 16
        levels and 32 feature columns ('cat': num_lods * feature_dim, 'sum': feature_dim), raw position input without embedding,
        one hidden relu layer of at most 256 units with biases, one output, tables on the GPU.  Any lod_idx the grid accepts:
        'cat' zeroes the columns from lod_idx * feature_dim on (hash_grid.py:226-229), so at lod_idx 0 the decoder sees the
        position alone.  The dict carries kind='hash'; wisp._C dispatches on it."""
        g, dec = nef.grid, nef.decoder
        tables = g.codebook.feats
        if (g.coord_dim != 3 or g.multiscale_type not in ('cat', 'sum') or g.feature_dim not in (2, 4, 8)
                or not 1 <= g.num_lods <= 16 or not 0 <= lod_idx < g.num_lods
                or (g.num_lods * g.feature_dim if g.multiscale_type == 'cat' else g.feature_dim) > 32
                or not nef.position_input or not isinstance(nef.pos_embedder, torch.nn.Identity)
                or not PackedSDFTracer._fused_decoder(nef, 1) or not tables.is_cuda
                or tables.dtype not in (torch.float32, torch.float16, torch.bfloat16)):
            return None
        cat = g.multiscale_type == 'cat'
        return dict(kind='hash', codebook=tables.detach().contiguous(), begin_idxes=[int(b) for b in g.codebook.begin_idxes.tolist()],
                    resolutions=[int(r) for r in g.resolutions], feature_dim=int(g.feature_dim),
                    codebook_bitwidth=int(g.codebook_bitwidth), multiscale=g.multiscale_type,
                    zero_from_col=(lod_idx if cat else g.num_lods) * g.feature_dim,
                    w1=dec.layers[0].weight.detach().float().contiguous(), b1=dec.layers[0].bias.detach().float().contiguous(),
                    w2=dec.lout.weight.detach().float().reshape(-1).contiguous(), b2=dec.lout.bias.detach().float().contiguous())

    @staticmethod
    def _fused_field_triplane(nef, lod_idx):
        """_fused_field for a plain NeuralSDF over a TriplanarGrid (csrc/triplane_sdf_eval.hip): linear interpolation, f32 planes
        on the GPU, at most 48 feature columns ('cat': (lod_idx + 1) * 3 * features per plane, 'sum': 3 * features per plane), raw
        position input without embedding, one hidden relu layer of at most 256 units with biases, one output.  0 <= lod_idx <
        num_lods; 'cat' only at the last level - below it TriplanarGrid.interpolate returns fewer columns than the decoder has.
        The dict carries kind='triplane' and the planes of the levels 0..lod_idx; wisp._C dispatches on the kind."""
        g, dec = nef.grid, nef.decoder
        if (g.multiscale_type not in ('cat', 'sum') or g.interpolation_type != 'linear'
                or not 1 <= g.num_lods <= 16 or not 0 <= lod_idx < g.num_lods
                or (g.multiscale_type == 'cat' and lod_idx != g.num_lods - 1)
                or not nef.position_input or not isinstance(nef.pos_embedder, torch.nn.Identity)
                or not PackedSDFTracer._fused_decoder(nef, 1)):
            return None
        planes = [p for i in range(lod_idx + 1) for p in (g.features[i].fmx, g.features[i].fmy, g.features[i].fmz)]
        cols = (lod_idx + 1 if g.multiscale_type == 'cat' else 1) * g.feature_dim          # (the grid's feature_dim is 3 x per plane)
        if (cols > 48 or dec.layers[0].in_features != 3 + cols
                or any(not p.is_cuda or p.dtype != torch.float32 for p in planes)):
            return None
        return dict(kind='triplane', planes=[p.detach().contiguous() for p in planes], multiscale=g.multiscale_type,
                    w1=dec.layers[0].weight.detach().float().contiguous(), b1=dec.layers[0].bias.detach().float().contiguous(),
                    w2=dec.lout.weight.detach().float().reshape(-1).contiguous(), b2=dec.lout.bias.detach().float().contiguous())

    def _march_fused(self, fld, rays, rt_pidx, depth, st, num_steps, step_size, min_dis):
        """All marching iterations as one launch each, no host decision per iteration: the loop only peeks at a device
        counter of still-marching packs every 8 iterations (the reference reads `mask.any()` twice per iteration)."""
        import wisp._C as _C
        counter = torch.zeros(1, dtype=torch.int32, device=st.t.device)

        def launch(first, cnt):
            _C.sdf_trace_step_field(first, st.o, st.d, depth, rt_pidx, rays.dist_max, min_dis, min_dis * 5, st.t, st.dist,
                                    st.dist_prev, st.active, st.hit, st.nug, st.nug_next, st.cell, st.x, fld, step_size, cnt)
        launch(True, None)
        st.dist_prev.copy_(st.dist)
        for it in range(num_steps):
            peek = (it % 8) == 7
            if peek:
                counter.zero_()
            launch(False, counter if peek else None)
            st.nug, st.nug_next = st.nug_next, st.nug
            if peek and int(counter.item()) == 0:
                break

    def trace(self, nef, rays, channels, extra_channels, lod_idx=None, num_steps=64, step_size=1.0, min_dis=1e-4):
        """Sphere-trace `rays`; returns RenderBuffer(xyz, depth, hit, normal, rgb (= normal colours), alpha)."""
        import wisp._C as _C
        assert nef.grid is not None and "this tracer requires a grid"
        if lod_idx is None:
            lod_idx = nef.grid.num_lods - 1
        invres = 1.0
        rt = nef.grid.raytrace(rays, nef.grid.active_lods[lod_idx], with_exit=True)
        depth = rt.depth
        depth[..., 0:1] += 1e-5                               # start just inside the first cell
        st = self._start(rays, rt.ridx, rt.pidx, depth)
        fld = self._fused_field(nef, lod_idx) if st.t.shape[0] else None
        if fld is not None:
            with torch.no_grad():
                self._march_fused(fld, rays, rt.pidx, depth, st, num_steps, invres * step_size, min_dis * invres)
            return self._gather(nef, rays, st, channels, extra_channels, lod_idx, bool(getattr(self, "fused_normals", False)))
        with torch.no_grad():
            self._query(nef, st, lod_idx, invres * step_size)
            st.dist_prev.copy_(st.dist)
            for _ in range(num_steps):
                _C.sphere_trace_step(st.o, st.d, depth, rt.pidx, rays.dist_max, min_dis * invres, (min_dis * 5) * invres,
                                     st.t, st.dist, st.dist_prev, st.active, st.hit, st.nug, st.nug_next, st.cell, st.x)
                st.nug, st.nug_next = st.nug_next, st.nug
                if not bool(self._query(nef, st, lod_idx, invres * step_size).any()):
                    break
        return self._gather(nef, rays, st, channels, extra_channels, lod_idx, bool(getattr(self, "fused_normals", False)))

    @staticmethod
    def _gather(nef, rays, st, channels, extra_channels, lod_idx, fused_normals=False):
        """scatter the per-pack results into per-ray buffers (rays without nuggets keep zeros).  fused_normals (the tracer
        attribute of that name, unset by default; OfflineRenderer.render sets it): the normals come from
        wisp.ops.sdf.sdf_fd_gradient - one launch on an nglod-shaped field - instead of six field queries; at the finest LOD
        either way, as the forward function of the unfused path is called without a lod_idx."""
        o = rays.origins
        dev = o.device
        hit = st.hit.bool()
        out = dict(xyz=torch.zeros_like(o), depth=torch.zeros_like(o[..., 0:1]), hit=torch.zeros_like(o[..., 0]).bool(),
                   normal=torch.zeros_like(o), rgb=torch.zeros(*o.shape[:-1], 3, device=dev),
                   alpha=torch.zeros(*o.shape[:-1], 1, device=dev))
        out["hit"][st.ray] = hit
        on_surface = out["hit"]
        for channel in extra_channels:
            feats = nef(coords=st.x[hit], lod_idx=lod_idx, channels=channel)
            buf = torch.zeros(*o.shape[:-1], feats.shape[-1], device=feats.device)
            buf[on_surface] = feats.to(buf.dtype)
            out[channel] = buf
        out["xyz"][on_surface] = st.x[hit]
        out["depth"][on_surface] = st.t[hit][:, None]
        if "rgb" in channels or "normal" in channels:
            if bool(hit.any()):
                if fused_normals:
                    from wisp.ops.sdf import sdf_fd_gradient
                    grad = sdf_fd_gradient(nef, st.x[hit], None)
                else:
                    grad = finitediff_gradient(st.x[hit], nef.get_forward_function("sdf"))
                out["normal"][on_surface] = F.normalize(grad, p=2, dim=-1, eps=1e-5)
            out["rgb"][..., :3] = (out["normal"] + 1.0) / 2.0
        out["alpha"][on_surface] = 1.0
        return RenderBuffer(**out)
