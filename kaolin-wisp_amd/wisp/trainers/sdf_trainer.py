"""SDFTrainStep: the optimisation step of the reference's SDFTrainer (wisp/trainers/sdf_trainer.py:65-124) without its app
plumbing - regression of a signed-distance field on (coordinate, distance) pairs:

    loss = sum over the loss LODs of  sum((nef(coords, lod)['sdf'] - gts)^2) / batch      (only_last: the finest LOD alone)

and, for a field that answers 'rgb' and 'sdf' together (NeuralSDFTex; the reference's branch for a dataset with sample_tex), of
(coordinate, distance, colour) triples: the colour term sum((rgb_pred - rgb)^2) joins the loss (accumulated as the reference
accumulates it, see _forward_backward).

Parameter groups, learning-rate weighting and the fused single-launch optimizer over one flat parameter buffer are the
MultiviewTrainStep's (base_trainer.py:205-235); nglod_octree.yaml trains with Adam, lr 1e-3, eps 1e-15, grid lr x 1."""
import logging as log
from dataclasses import dataclass

import torch

from wisp.trainers.base_trainer import BaseTrainer, ConfigBaseTrainer
from wisp.trainers.multiview_trainer import FlatParams


def _hip():
    import wisp._C as _C
    return _C


class SDFTrainStep:
    def __init__(self, nef, lr=1e-3, eps=1e-15, weight_decay=0.0, grid_lr_weight=1.0, betas=(0.9, 0.999), optimizer='adam',
                 only_last=True, alpha=0.99, momentum=0.0, fused_hash=False, fused_triplane=False, fused_lods=False):
        self.nef = nef
        # opt-in: a NeuralSDF over a HashGrid trains through wisp_hash_sdf_train_step (see _fused_field); a trainer built without
        # it keeps the modular launches over a hash grid, with the results it always had
        self.fused_hash = bool(fused_hash)
        # opt-in, likewise: a NeuralSDF over a TriplanarGrid trains through wisp_triplane_sdf_train_step
        self.fused_triplane = bool(fused_triplane)
        # opt-in, likewise: with only_last=False a NeuralSDF / NeuralSDFTex over an OctreeGrid trains through
        # wisp_sdf_lods_train_step, the loss over every LOD in one launch; without it only_last=False keeps the modular launches
        self.fused_lods = bool(fused_lods)
        self.flat = FlatParams(nef)
        self.lr, self.eps, self.weight_decay, self.grid_lr_weight, self.betas = lr, eps, weight_decay, grid_lr_weight, betas
        self.optimizer = str(optimizer).lower()
        if self.optimizer not in ('adamw', 'adam', 'rmsprop'):
            raise ValueError(f"optimizer must be 'adamw', 'adam' or 'rmsprop', got {optimizer!r}")
        self.alpha, self.momentum = alpha, momentum
        self.only_last = only_last
        self.opt_steps = 0
        # a field whose forward registers 'rgb' and 'sdf' together (NeuralSDFTex): step() then needs the colour ground truth
        self.textured = any({"rgb", "sdf"} <= set(ch) for ch in getattr(nef, "_forward_functions", {}).values())
        self.last_l2 = self.last_rgb = None       # after a textured step: the two un-normalised sums (device tensors, no sync)

    def loss_lods(self):
        lods = list(range(self.nef.grid.num_lods))
        return lods[-1:] if self.only_last else lods

    def optimizer_step(self):
        C = _hip()
        self.opt_steps += 1
        f = self.flat
        groups = []
        for g, lr in (("decoder", self.lr), ("grid", self.lr * self.grid_lr_weight), ("rest", self.lr)):
            a, b = f.ranges[g]
            if b > a:
                groups.append((a, b - a, lr, self.weight_decay, None))
        if self.optimizer == 'rmsprop':
            C.optim_step_groups('rmsprop', f.data, f.grad, f.exp_avg if self.momentum > 0 else None, f.exp_avg_sq, groups,
                                self.alpha, self.momentum, self.eps, self.opt_steps, zero_grad=True)
        else:
            C.optim_step_groups(self.optimizer, f.data, f.grad, f.exp_avg, f.exp_avg_sq, groups, self.betas[0], self.betas[1],
                                self.eps, self.opt_steps, zero_grad=True)

    def _fused_field(self):
        """What wisp_sdf_train_step needs, or None when this field is not its shape: NeuralSDF's decoder (one hidden relu layer,
        biases, one output) over [position, 'sum' OctreeGrid features of 16 channels], fp32 parameters living in the flat
        buffers, loss on the finest LOD only.  A NeuralSDFTex (four outputs; features alone, or the identity position in front
        of them) gets what wisp_sdf_tex_train_step needs under the same gates.  A plain NeuralSDF over a HashGrid gets what
        wisp_hash_sdf_train_step needs (_fused_field_hash) - only in a trainer built with fused_hash=True; one over a TriplanarGrid
        what wisp_triplane_sdf_train_step needs (_fused_field_triplane) - only in a trainer built with fused_triplane=True.
        With only_last=False, the loss over every LOD, the two octree fields get what wisp_sdf_lods_train_step needs - the same
        gates, the cache entry marked lods_loss=True - only in a trainer built with fused_lods=True; every other field, and every
        trainer without that flag, then keeps the modular launches.  WISP_SDF_TRAIN_FUSED=0 keeps the modular launches."""
        import os
        if getattr(self, "_fused_seen_only_last", None) != self.only_last:        # toggled since the decision was taken
            self._fused_cache, self._fused_seen_only_last = None, self.only_last
        cached = getattr(self, "_fused_cache", None)
        if cached is not None:
            # the expensive shape checks are cached; what can change under a live trainer is re-checked on every call: the loss
            # selection, the field's grid / decoder objects, the number of levels, gradients set to None or re-homed
            if cached and not self._fused_still_valid(cached):
                cached = self._fused_cache = None                 # re-derive below
            else:
                return cached or None
        self._fused_cache = False
        all_lods = not self.only_last
        if os.environ.get("WISP_SDF_TRAIN_FUSED", "1") == "0" or (all_lods and not getattr(self, "fused_lods", False)):
            return None
        from wisp.accelstructs import OctreeAS
        from wisp.models.grids import HashGrid, OctreeGrid, TriplanarGrid
        from wisp.models.nefs._grid_mlp import _fusable_small_decoder
        nef = self.nef
        grid, dec = getattr(nef, "grid", None), getattr(nef, "decoder", None)
        if all_lods and type(grid) is not OctreeGrid:             # the all-LOD step exists for the octree fields only
            return None
        if type(grid) is HashGrid:
            return self._fused_field_hash(grid, dec) if self.fused_hash and dec is not None else None
        if type(grid) is TriplanarGrid:
            return self._fused_field_triplane(grid, dec) if self.fused_triplane and dec is not None else None
        if type(grid) is not OctreeGrid or type(getattr(grid, "blas", None)) is not OctreeAS or dec is None:
            return None
        if self.textured:
            return self._fused_field_tex(grid, dec)
        if not (grid.interpolation_type == 'linear' and grid.multiscale_type == 'sum' and grid.feature_dim == 16 and grid._fusable()
                and 1 <= grid.num_lods <= 16 and type(getattr(nef, "pos_embedder", None)) is torch.nn.Identity
                and getattr(nef, "position_input", False)):
            return None
        probe = torch.empty(1, 3 + grid.feature_dim, device=self.flat.data.device)
        if not probe.is_cuda or not _fusable_small_decoder(dec, probe) or dec.layers[0].in_features != 3 + grid.feature_dim:
            return None
        prm = list(grid.features[:grid.num_lods]) + [dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias]
        if not all(q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.grad is not None and q.grad.is_contiguous()
                   and q.grad.dtype == torch.float32 for q in prm):
            return None
        self._fused_cache = dict(grid=grid, dec=dec, lods=grid.num_lods, prm=prm, lods_loss=all_lods)
        return self._fused_cache

    def _fused_field_tex(self, grid, dec):
        """The textured branch of _fused_field (the grid / accelerator types are checked by the caller)."""
        from wisp.models.nefs._grid_mlp import BasicDecoder
        from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
        nef = self.nef
        if type(nef) is not NeuralSDFTex:
            return None
        if not (grid.interpolation_type == 'linear' and grid.multiscale_type == 'sum' and grid.feature_dim == 16 and grid._fusable()
                and 1 <= grid.num_lods <= 16):
            return None
        if nef.embedder_type == 'none' and not nef.position_input:
            pos = 0
        elif type(getattr(nef, "pos_embedder", None)) is torch.nn.Identity and nef.position_input and nef.pos_embed_dim == 3:
            pos = 1
        else:
            return None
        # (the shape check of _fusable_small_decoder, restated for four outputs: that function serves the one-output `decode`)
        layers, lout = getattr(dec, 'layers', None), getattr(dec, 'lout', None)
        if not (self.flat.data.is_cuda and type(dec) is BasicDecoder and layers is not None and len(layers) == 1 and not dec.skip
                and type(layers[0]) is torch.nn.Linear and type(lout) is torch.nn.Linear and layers[0].bias is not None
                and lout.bias is not None and lout.out_features == 4 and 1 <= layers[0].out_features <= 256
                and lout.in_features == layers[0].out_features and layers[0].in_features == 3 * pos + grid.feature_dim
                and dec.activation in (torch.relu, torch.nn.functional.relu)):
            return None
        prm = list(grid.features[:grid.num_lods]) + [layers[0].weight, layers[0].bias, lout.weight, lout.bias]
        if not all(q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.grad is not None and q.grad.is_contiguous()
                   and q.grad.dtype == torch.float32 for q in prm):
            return None
        self._fused_cache = dict(grid=grid, dec=dec, lods=grid.num_lods, prm=prm, tex=True, pos=pos, lods_loss=not self.only_last)
        return self._fused_cache

    def _fused_field_hash(self, grid, dec):
        """The hash branch of _fused_field (the caller has checked the grid's type and the opt-in): a plain NeuralSDF, the shape
        rules of PackedSDFTracer._fused_field_hash at the finest LOD - for 'cat' that is zero_from_col = (num_lods - 1) *
        feature_dim, because HashGrid.interpolate zeroes the columns from lod_idx * feature_dim on (hash_grid.py:226-229): the finest
        level gets no gradient, exactly as on the modular path - and an f32 table and decoder living in the flat buffers."""
        from wisp.models.nefs.neural_sdf import NeuralSDF
        from wisp.tracers import PackedSDFTracer
        nef = self.nef
        if type(nef) is not NeuralSDF or self.textured:
            return None
        fld = PackedSDFTracer._fused_field_hash(nef, grid.num_lods - 1)
        if fld is None:
            return None
        prm = [grid.codebook.feats, dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias]
        if not all(q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.grad is not None and q.grad.is_contiguous()
                   and q.grad.dtype == torch.float32 for q in prm):
            return None
        # the host-side description is kept (begin_idxes comes from a device tensor); the tensors are taken anew at every step
        host = {k: fld[k] for k in ("kind", "begin_idxes", "resolutions", "feature_dim", "codebook_bitwidth", "multiscale",
                                    "zero_from_col")}
        self._fused_cache = dict(grid=grid, dec=dec, lods=grid.num_lods, prm=prm, hash=True, host=host)
        return self._fused_cache

    def _fused_field_triplane(self, grid, dec):
        """The triplanar branch of _fused_field (the caller has checked the grid's type and the opt-in): a plain NeuralSDF, the shape
        rules of PackedSDFTracer._fused_field_triplane at the last level, and f32 contiguous planes and decoder whose contiguous f32
        gradients live in the flat buffers."""
        from wisp.models.nefs.neural_sdf import NeuralSDF
        from wisp.tracers import PackedSDFTracer
        nef = self.nef
        if type(nef) is not NeuralSDF or self.textured:
            return None
        if PackedSDFTracer._fused_field_triplane(nef, grid.num_lods - 1) is None:
            return None
        prm = self._triplane_planes(grid) + [dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias]
        if not all(q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.grad is not None and q.grad.is_contiguous()
                   and q.grad.dtype == torch.float32 for q in prm):
            return None
        self._fused_cache = dict(grid=grid, dec=dec, lods=grid.num_lods, prm=prm, triplane=True, multiscale=grid.multiscale_type)
        return self._fused_cache

    @staticmethod
    def _triplane_planes(grid):
        """x, y, z of level 0, then level 1, ...: the plane order of the kernels"""
        return [p for i in range(grid.num_lods) for p in (grid.features[i].fmx, grid.features[i].fmy, grid.features[i].fmz)]

    def _fused_still_valid(self, c):
        nef = self.nef
        grid, dec = c["grid"], c["dec"]
        all_lods = bool(c.get("lods_loss"))
        if self.only_last == all_lods or (all_lods and not getattr(self, "fused_lods", False)) \
                or getattr(nef, "grid", None) is not grid or getattr(nef, "decoder", None) is not dec \
                or grid.num_lods != c["lods"]:
            return False
        if c.get("triplane"):
            if grid.multiscale_type != c["multiscale"]:
                return False
            tables = self._triplane_planes(grid)
        else:
            tables = [grid.codebook.feats] if c.get("hash") else list(grid.features[:grid.num_lods])
        now = tables + [dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias]
        if len(now) != len(c["prm"]):
            return False
        for q, was in zip(now, c["prm"]):
            g = q.grad
            if q is not was or g is None or g.dtype != torch.float32 or not g.is_contiguous() or not q.is_contiguous():
                return False
        return True

    def _forward_backward(self, coords, gts, rgb=None):
        fused = self._fused_field() if coords.is_cuda and coords.ndim == 2 and coords.shape[0] > 0 else None
        if fused is not None:
            C = _hip()
            grid, dec = fused["grid"], fused["dec"]
            if fused.get("hash"):
                table = grid.codebook.feats
                w1, b1, w2, b2 = dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias
                fld = dict(fused["host"], codebook=table.detach(), w1=w1.detach(), b1=b1.detach(), w2=w2.detach().reshape(-1),
                           b2=b2.detach())
                return C.hash_sdf_train_step(coords, gts, fld, table.grad, w1.grad, b1.grad, w2.grad.reshape(-1), b2.grad)[0]
            if fused.get("triplane"):
                planes = self._triplane_planes(grid)
                w1, b1, w2, b2 = dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias
                fld = dict(kind='triplane', planes=[p.detach() for p in planes], multiscale=fused["multiscale"], w1=w1.detach(),
                           b1=b1.detach(), w2=w2.detach().reshape(-1), b2=b2.detach())
                return C.triplane_sdf_train_step(coords, gts, fld, [p.grad for p in planes], w1.grad, b1.grad, w2.grad.reshape(-1),
                                                 b2.grad)[0]
            L = grid.num_lods
            blas = grid.blas
            grid._sync_device(coords.device)
            tr = grid.trinkets if grid.trinkets.dtype == torch.int32 else grid.trinkets.int()
            w1, b1, w2, b2 = dec.layers[0].weight, dec.layers[0].bias, dec.lout.weight, dec.lout.bias
            if fused.get("lods_loss"):
                # every LOD weighs 1 in the distance term; the reference adds the RUNNING colour sum inside its LOD loop
                # (sdf_trainer.py:92-101; the modular branch below), so LOD k's colour error counts L - k times
                tex = bool(fused.get("tex"))
                colour = rgb[..., :3].reshape(-1, 3).to(torch.float32).contiguous() if tex else None
                out = C.sdf_lods_train_step(coords, gts, colour, blas.octree, blas.prefix, blas.points, tr,
                                            [f.detach() for f in grid.features[:L]], grid.active_lods[:L], grid.half_features,
                                            fused["pos"] if tex else 1, [1.0] * L, [float(L - k) for k in range(L)] if tex else None,
                                            w1.detach(), b1.detach(), w2.detach(), b2.detach(),
                                            [f.grad for f in grid.features[:L]], w1.grad, b1.grad, w2.grad, b2.grad)
                if tex:
                    self.last_l2, self.last_rgb = out[L], out[2 * L]
                return out[0]
            if fused.get("tex"):
                colour = rgb[..., :3].reshape(-1, 3).to(torch.float32).contiguous()
                out = C.sdf_tex_train_step(coords, gts, colour, blas.octree, blas.prefix, blas.points, tr,
                                           [f.detach() for f in grid.features[:L]], grid.active_lods[:L], grid.half_features,
                                           fused["pos"], w1.detach(), b1.detach(), w2.detach(), b2.detach(),
                                           [f.grad for f in grid.features[:L]], w1.grad, b1.grad, w2.grad, b2.grad)
                self.last_l2, self.last_rgb = out[1], out[2]
                return out[0]
            loss = C.sdf_train_step(coords, gts, blas.octree, blas.prefix, blas.points, tr, [f.detach() for f in grid.features[:L]],
                                    grid.active_lods[:L], grid.half_features, w1.detach(), b1.detach(), w2.detach(), b2.detach(),
                                    [f.grad for f in grid.features[:L]], w1.grad, b1.grad, w2.grad, b2.grad)
            return loss[0]
        if self.textured:
            # SDFTrainer.step with sample_tex: the running colour sum joins the loss INSIDE the LOD loop, as the reference does
            loss, l2_loss, rgb_loss = 0.0, 0.0, 0.0
            last_l2 = last_rgb = None
            preds = [self.nef(coords=coords, lod_idx=lod_idx, channels=["rgb", "sdf"]) for lod_idx in self.loss_lods()]
            for colour, dist in preds:
                last_rgb = ((colour - rgb[..., :3]) ** 2).sum()
                rgb_loss = rgb_loss + last_rgb
                last_l2 = ((dist - gts) ** 2).sum()
                l2_loss = l2_loss + last_l2
                loss = loss + rgb_loss
            loss = (loss + l2_loss) / coords.shape[0]
            loss.backward()
            self.last_l2, self.last_rgb = last_l2.detach(), last_rgb.detach()
            return loss.detach()
        loss = 0.0
        for lod_idx in self.loss_lods():
            pred = self.nef(coords=coords, lod_idx=lod_idx, channels="sdf")
            loss = loss + ((pred - gts) ** 2).sum()
        loss = loss / coords.shape[0]
        loss.backward()
        return loss.detach()

    def capture(self, batch_size):
        """Capture forward + loss + backward for a FIXED batch size as one HIP graph (torch.cuda.CUDAGraph on ROCm).
        The step of nglod_octree.yaml is 512 coordinates: a dozen small launches whose GPU time (~50 us) is a fraction of
        what Python + autograd need to issue them (~0.8 ms).  Every shape in it is static - query, trilinear blend and
        decoder see [batch_size, ...] tensors, nothing depends on data - so the launches are recorded once and replayed;
        the fused optimizer stays outside (its bias correction changes every step and it is one launch anyway).
        step() uses the graph whenever it is handed a batch of the captured size; results equal the eager step's."""
        dev = self.flat.data.device
        if dev.type != 'cuda':
            raise RuntimeError("SDFTrainStep.capture needs the model on the GPU")
        self._fused_cache = None                               # the graph bakes pointers in: decide afresh what gets captured
        self._g_coords = torch.zeros(batch_size, 3, dtype=torch.float32, device=dev)
        self._g_gts = torch.zeros(batch_size, 1, dtype=torch.float32, device=dev)
        self._g_rgb = torch.zeros(batch_size, 3, dtype=torch.float32, device=dev) if self.textured else None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # warm-up off the default stream (allocator, lazy set-up)
            for _ in range(3):
                self._forward_backward(self._g_coords, self._g_gts, self._g_rgb)
        torch.cuda.current_stream().wait_stream(side)
        self.flat.grad.zero_()                                 # the warm-up passes accumulated gradients; parameters untouched
        graph = torch.cuda.CUDAGraph()
        # (captured on the warm-up stream: the per-(device, stream) scratch the ops keep was created - and zeroed - there; on another
        #  stream they would allocate it anew INSIDE the capture, and every replay would zero a few MB again)
        with torch.cuda.graph(graph, stream=side):
            self._g_loss = self._forward_backward(self._g_coords, self._g_gts, self._g_rgb)
            self._g_l2, self._g_rgbsum = self.last_l2, self.last_rgb
        self.flat.grad.zero_()
        self._graph = graph
        return self

    def static_inputs(self):
        """(coords [B,3], gts [B,1]) buffers of the captured graph - for a textured field (coords, gts, rgb [B,3]) - or None: a
        loader that fills THESE and hands them to step() spares the device copies step() otherwise makes into them."""
        if getattr(self, "_graph", None) is None:
            return None
        if self.textured:
            return self._g_coords, self._g_gts, self._g_rgb
        return self._g_coords, self._g_gts

    def step(self, coords, gts, rgb=None):
        """coords [B,3], gts [B,1] on the GPU -> loss tensor (already divided by the batch size, like the reference).  A textured
        field (NeuralSDFTex) also needs rgb [B,3+]; afterwards last_l2 / last_rgb hold the two un-normalised sums the
        reference's tracker adds up, as device tensors."""
        if self.textured and rgb is None:
            raise ValueError("SDFTrainStep.step: `rgb` is required for a field that predicts 'rgb' and 'sdf' together")
        if not self.textured and rgb is not None:
            raise ValueError("SDFTrainStep.step: `rgb` was given, but this field has no colour output to fit it with")
        graph = getattr(self, "_graph", None)
        if graph is not None and tuple(coords.shape) == tuple(self._g_coords.shape) and tuple(gts.shape) == tuple(self._g_gts.shape) \
                and (rgb is None or tuple(rgb.shape) == tuple(self._g_rgb.shape)):
            if coords is not self._g_coords:
                self._g_coords.copy_(coords)
            if gts is not self._g_gts:
                self._g_gts.copy_(gts)
            if rgb is not None and rgb is not self._g_rgb:
                self._g_rgb.copy_(rgb)
            graph.replay()
            self.optimizer_step()
            if self.textured:
                self.last_l2, self.last_rgb = self._g_l2.clone(), self._g_rgbsum.clone()
            return self._g_loss.clone()
        loss = self._forward_backward(coords, gts, rgb)
        self.optimizer_step()
        return loss


@dataclass
class ConfigSDFTrainer(ConfigBaseTrainer):
    """Field names and defaults of wisp/trainers/sdf_trainer.py:20-29 (the YAML schema under `trainer:` of app/nglod)."""
    log_2d: bool = False
    only_last: bool = True
    resample: bool = False


class SDFTrainer(BaseTrainer):
    """The reference's SDF trainer as app/nglod uses it (wisp/trainers/sdf_trainer.py:32-135): the unchanged-trainer regime for
    signed-distance fields - BaseTrainer's life cycle (autocast around step() when enable_amp), autograd over the field, a
    torch.optim optimizer with the name-matched parameter groups.  Events of step() in the reference's order: zero the
    gradients, one field query per loss LOD, sum of squared errors (plus the colour term when the dataset samples textures),
    three metric read-backs, division by the batch size, backward, optimizer step - no GradScaler here (the reference's SDF step
    never scales, sdf_trainer.py:120-123).  SDFTrainStep is the fused MI355X step with the same arithmetic."""

    def __init__(self, cfg, pipeline, train_dataset, tracker=None, device='cuda', scene_state=None):
        super().__init__(cfg=cfg, pipeline=pipeline, train_dataset=train_dataset, tracker=tracker, device=device,
                         scene_state=scene_state)

    def pre_training(self):
        super().pre_training()
        self.tracker.metrics.define_metric('rgb_loss', aggregation_type=float)
        self.tracker.metrics.define_metric('l2_loss', aggregation_type=float)

    def pre_epoch(self):
        super().pre_epoch()
        lods = list(range(self.pipeline.nef.grid.num_lods))
        self.loss_lods = lods[-1:] if self.cfg.only_last else lods

    def post_epoch(self):
        super().post_epoch()
        if self.cfg.log_2d and self.cfg.render_every > -1 and self.epoch % self.cfg.render_every == 0:
            self.render_snapshot()
        if self.cfg.resample:
            self.resample_dataset()

    def step(self, data):
        pts = data['coords'].to(self.device)
        gts = data['sdf'].to(self.device)
        with_colour = bool(getattr(self.train_dataset, 'sample_tex', False))
        rgb = data['rgb'].to(self.device) if with_colour else None
        batch_size = pts.shape[0]
        self.pipeline.zero_grad()
        nef = self.pipeline.nef
        loss, l2_loss, rgb_loss = 0, 0.0, 0.0
        last_l2, last_rgb = 0.0, None
        if with_colour:
            preds = [nef(coords=pts, lod_idx=lod_idx, channels=["rgb", "sdf"]) for lod_idx in self.loss_lods]
            for colour, dist in preds:
                last_rgb = ((colour - rgb[..., :3]) ** 2).sum()
                rgb_loss += last_rgb
                last_l2 = ((dist - 1.0 * gts) ** 2).sum()
                l2_loss += last_l2
                loss += rgb_loss                                    # (accumulated inside the loop, as the reference does)
        else:
            preds = [nef(coords=pts, lod_idx=lod_idx, channels=["sdf"])[0] for lod_idx in self.loss_lods]
            for dist in preds:
                last_l2 = ((dist - 1.0 * gts) ** 2).sum()
                l2_loss += last_l2
        loss += l2_loss
        m = self.tracker.metrics
        m.total_loss += loss.item()
        m.l2_loss += last_l2.item()
        if last_rgb is not None:
            m.rgb_loss += last_rgb.item()
        m.num_samples += batch_size
        loss /= batch_size
        loss.backward()
        self.optimizer.step()

    def _validation_metric_name(self):
        from wisp.datasets import MeshSampledSDFDataset, OctreeSampledSDFDataset
        if isinstance(self.train_dataset, MeshSampledSDFDataset):
            return "volumetric_iou"
        if isinstance(self.train_dataset, OctreeSampledSDFDataset):
            return "narrowband_iou"
        raise NotImplementedError

    def validate(self):
        """Intersection over union of the field's interior with the ground truth's over the TRAINING set (the field is fitted to
        one shape), one score per loader batch and loss LOD, as wisp/trainers/sdf_trainer.py:156-190: metric name by dataset
        class, `tracker.log_metric('Validation/<name>/<lod>', score, epoch)` for the pairs of zip(loss_lods, scores) - the
        reference's loop, which logs only the first len(loss_lods) scores while its console line divides their sum by the
        number of ALL scores; reproduced as it stands.  Added: returns {name: [mean score over all batches, per loss LOD]}
        (the reference returns None).
        On an nglod-shaped field (wisp.ops.sdf.fused_sdf_field) a batch is one wisp_sdf_query launch that adds its two counts
        to its own row of a zeroed [batches x lods, 2] int64 tensor, read back once at the end; otherwise one field query and
        compute_sdf_iou - with its two read-backs - per batch, as in the reference."""
        from wisp.ops.sdf import compute_sdf_iou, fused_sdf_field
        metric_name = self._validation_metric_name()
        nef = self.pipeline.nef
        loss_lods = getattr(self, "loss_lods", None)
        if loss_lods is None:                             # (pre_epoch sets it; validate() before any epoch derives it the same way)
            lods = list(range(nef.grid.num_lods))
            loss_lods = lods[-1:] if self.cfg.only_last else lods
        on_gpu = torch.device(self.device).type == 'cuda'
        fields = {lod: (fused_sdf_field(nef, lod) if on_gpu else None) for lod in loss_lods}
        rows = len(self.train_data_loader) * len(loss_lods)
        counts = torch.zeros(rows, 2, dtype=torch.int64, device=self.device) if any(f is not None for f in fields.values()) else None
        scores = []                                       # a float, or the row of `counts` that will give it
        with torch.no_grad():
            for data in self.train_data_loader:
                pts = data['coords'].to(self.device)
                gts = data['sdf'].to(self.device)
                for lod_idx in loss_lods:
                    fld, row = fields[lod_idx], len(scores)
                    if fld is not None and row < rows and pts.shape[0] > 0:
                        _hip().sdf_query(pts, fld, gts=gts, counts=counts[row], with_out=False)
                        scores.append(row)
                    else:
                        pred = nef(coords=pts, lod_idx=lod_idx, channels="sdf")
                        scores.append(float(compute_sdf_iou(pred, gts)))
        if counts is not None:
            host = counts.cpu().tolist()                  # the one read-back
            scores = [s if isinstance(s, float) else 100.0 * (float(host[s][0]) / float(host[s][1])) for s in scores]
        val_dict = {metric_name: scores}
        log_text = 'EPOCH {}/{}'.format(self.epoch, self.max_epochs)
        for k, v in val_dict.items():
            score_total = 0.0
            for lod, score in zip(loss_lods, v):
                self.tracker.log_metric(f'Validation/{k}/{lod}', score, self.epoch)
                score_total += score
            log_text += ' | {}: {:.4f}'.format(k, score_total / len(v))
        log.info(log_text)
        n = len(loss_lods)
        return {metric_name: [sum(scores[i::n]) / len(scores[i::n]) for i in range(n)] if scores else []}

    def render_snapshot(self):
        """The three axis-aligned cross-sections of the distance field through `tracker.visualizer.sdf_slice`, logged as images
        when cfg.log_2d is set (wisp/trainers/sdf_trainer.py:138-154).  A tracker without a visualizer gets an OfflineRenderer."""
        self.pipeline.eval()
        if not self.cfg.log_2d:
            return
        from wisp.trainers.tracker import OfflineRenderer
        renderer = getattr(self.tracker, 'visualizer', None)
        if renderer is None:
            renderer = self.tracker.visualizer = OfflineRenderer(device=self.device)
        nef = self.pipeline.nef
        d = nef.grid.num_lods - 1
        # an OfflineRenderer of this package is handed the field itself and evaluates it through wisp.ops.sdf.sdf_query (one
        # launch on an nglod-shaped field); any other visualizer gets the 'sdf' forward function, as the reference hands it
        what = nef if isinstance(renderer, OfflineRenderer) else nef.get_forward_function("sdf")
        for axis, name in enumerate("XYZ"):
            img = torch.FloatTensor(renderer.sdf_slice(what, dim=axis))
            self.tracker.log_image(f'Cross-section/{name}/{d}', img.permute(2, 0, 1), self.epoch)

    def log_console(self):
        m = self.tracker.metrics
        log.info('EPOCH {}/{} | total loss: {:>.3E} | l2 loss: {:>.3E} | rgb loss: {:>.3E}'.format(
            self.epoch, self.max_epochs, m.average_metric('total_loss'), m.average_metric('l2_loss'), m.average_metric('rgb_loss')))
