"""NeuralSDFTex: octree feature grid (+ optional embedded position) -> MLP -> surface colour and signed distance, NGLOD with
albedo.  Mirrors wisp/models/nefs/neural_sdf_tex.py:20-123: constructor schema and attributes, a BasicDecoder with four outputs,
the forward function `rgbsdf` registered for the channels "rgb" and "sdf".  `rgbsdf` itself runs over the grid ops and autograd
(what existing calls return stays as it is; wisp.ops.sdf.sdf_query evaluates the same four outputs in one launch for that shape).  Training and marching have fused paths for the
shape of nglod_octree.yaml - 16 'sum' OctreeGrid features, one hidden relu layer, embedder_type 'none' or the identity position:
SDFTrainStep.step(coords, gts, rgb) runs forward + loss + backward as wisp_sdf_tex_train_step (four launches), and
PackedSDFTracer marches on the decoder's fourth output row through wisp_sdf_trace_step_fused; any other shape takes the modular
launches.

Differences from the reference:
  * it reads `self.grid.num_lods` where the reference reads `self.num_lods`, an attribute its base class does not define
    (:66 for a 'cat' grid, :102 whenever lod_idx is None);
  * the reference's init_embedder (:59) passes `active=` to an embedder factory that no longer takes it; what the keyword
    meant is kept: 'positional' gives the Fourier embedder of `pos_multires` octaves with the raw input in front, anything
    else the identity of width 3 (used only when embedder_type != 'none')."""
import logging as log
from typing import Any, Dict

import torch

from wisp.models.embedders import get_positional_embedder
from wisp.models.grids import BLASGrid
from wisp.models.nefs import _grid_mlp
from wisp.models.nefs.base_nef import BaseNeuralField


class NeuralSDFTex(BaseNeuralField):
    def __init__(self, grid: BLASGrid = None, embedder_type: str = 'none', pos_multires: int = 10,
                 activation_type: str = 'relu', layer_type: str = 'none', hidden_dim: int = 128, num_layers: int = 1):
        super().__init__()
        self.grid = grid
        self.embedder_type = embedder_type
        self.pos_multires = pos_multires
        self.pos_embedder, self.pos_embed_dim = self.init_embedder(embedder_type, pos_multires)
        self.activation_type = activation_type
        self.layer_type = layer_type
        self.hidden_dim = hidden_dim
        self.num_layers = num_layers
        self.position_input = embedder_type != 'none'
        self.decoder, self.effective_feature_dim, self.input_dim = \
            self.init_decoder(activation_type, layer_type, num_layers, hidden_dim, self.position_input, self.pos_embed_dim)

    def init_embedder(self, embedder_type, pos_multires):
        if embedder_type == "positional":
            pos_embedder, pos_embed_dim = get_positional_embedder(frequencies=pos_multires)
        else:
            pos_embedder, pos_embed_dim = torch.nn.Identity(), 3
        log.info(f"Position Embed Dim: {pos_embed_dim}")
        return pos_embedder, pos_embed_dim

    def init_decoder(self, activation_type, layer_type, num_layers, hidden_dim, position_input, pos_embed_dim):
        effective_feature_dim = _grid_mlp.grid_feature_width(self.grid)
        input_dim = effective_feature_dim + (pos_embed_dim if position_input else 0)
        decoder = _grid_mlp.make_decoder(input_dim, 4, activation_type, layer_type, num_layers, hidden_dim)
        return decoder, effective_feature_dim, input_dim

    def register_forward_functions(self):
        self._register_forward_function(self.rgbsdf, ["rgb", "sdf"])

    def rgbsdf(self, coords, lod_idx=None):
        """coords [batch, 3] or [batch, num_samples, 3] -> rgb (sigmoid of the first three decoder outputs) and sdf (the fourth),
        keeping the leading shape."""
        shape = coords.shape
        if shape[0] == 0:
            return dict(rgb=torch.zeros_like(coords)[..., :3], sdf=torch.zeros_like(coords)[..., 0:1])
        if lod_idx is None:
            lod_idx = self.grid.num_lods - 1
        if len(shape) == 2:
            coords = coords[:, None]
        feats = self.grid.interpolate(coords, lod_idx)
        if self.position_input:
            emb = self.pos_embedder(coords.reshape(-1, 3)).reshape(*coords.shape[:-1], -1)
            feats = torch.cat([emb, feats], dim=-1)
        rgbsdf = self.decoder(feats)
        if len(shape) == 2:
            rgbsdf = rgbsdf[:, 0]
        return dict(rgb=torch.sigmoid(rgbsdf[..., :3]), sdf=rgbsdf[..., 3:4])

    def public_properties(self) -> Dict[str, Any]:
        return {"Grid": self.grid, "Pos. Embedding": self.pos_embedder, "Decoder (rgb, sdf)": self.decoder}
