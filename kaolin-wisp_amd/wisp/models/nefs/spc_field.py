"""SPCField: a Structured Point Cloud rendered directly with its per-cell colours - no grid features, embedders or decoders
(class surface of wisp/models/nefs/spc_field.py:19-157: constructor, init_grid, the three colour sources, rgba, device,
public_properties).  The field only holds `colors`, one row per cell of the finest level in point-hierarchy order;
PackedSPCTracer reads them either through rgba() or straight from its fused first-hit launch (csrc/spc.hip)."""
from typing import Any, Dict

import torch

from wisp.accelstructs import OctreeAS
from wisp.models.grids import OctreeGrid
from wisp.models.nefs.base_nef import BaseNeuralField


class SPCField(BaseNeuralField):
    def __init__(self, spc_octree: torch.ByteTensor, features_dict: Dict[str, torch.Tensor] = None, device: torch.device = 'cuda'):
        """spc_octree: one occupancy byte per non-leaf cell, breadth first, Morton order.
        features_dict: a subset of {'colors': u8 RGBA (any shape with 4 * cells entries), 'normals': [cells, 3]}, one row per
        cell of the finest level.  device: what `self.device` reports; nothing is moved (the tensors stay where the caller
        put them, as in the reference)."""
        super().__init__()
        self.spc_octree = spc_octree
        self.features_dict = features_dict if features_dict is not None else dict()
        self.spc_device = device
        self.grid = None
        self.colors = None
        self.normals = None
        self.init_grid(spc_octree)

    def init_grid(self, spc_octree: torch.ByteTensor):
        """Colours from the features (spc_field.py:79-103) and the octree as an OctreeGrid without feature levels."""
        if "colors" in self.features_dict:
            colors = self.features_dict["colors"].reshape(-1, 4)
            # a tensor divisor: torch divides by a Python scalar on the GPU as a multiplication by its rounded reciprocal, which
            # is off by an ulp for some bytes; this is the correctly rounded quotient, the same bits on every device
            self.colors = colors / torch.full((), 255.0, dtype=torch.float32, device=colors.device)
        if "normals" in self.features_dict:
            self.normals = self.features_dict["normals"].reshape(-1, 3)
        blas = OctreeAS(spc_octree)
        if self.colors is None:
            if self.normals is not None:                        # no colours: shade with the normals
                self.colors = 0.5 * (self.normals + 1.0)
            else:                                               # neither: the finest level's cell coordinates / 2^level
                level = blas.max_level
                self.colors = blas.points[int(blas.pyramid[1, level]):].float() / float(2 ** level)
        # the field keeps its features itself: an OctreeGrid with num_lods = 0 allocates none
        self.grid = OctreeGrid(blas=blas, feature_dim=3, num_lods=0)

    @property
    def device(self):
        return self.spc_device

    def register_forward_functions(self):
        self._register_forward_function(self.rgba, ["rgb"])

    def rgba(self, ridx_hit=None):
        """ridx_hit: int64 [batch] point-hierarchy indices of cells of the finest level -> {'rgb': f32 [batch, 1, 3]}."""
        level = self.grid.blas.max_level
        offset = self.grid.blas.pyramid[1, level]
        ridx_hit = ridx_hit - offset
        return dict(rgb=self.colors[ridx_hit, :3].unsqueeze(1))

    def public_properties(self) -> Dict[str, Any]:
        return {"Grid": self.grid}
