"""OctreeSampledSDFDataset (wisp/datasets/formats/octree_sdf_dataset.py:20-220): a pool of samples drawn in the occupied cells of
an octree built from a mesh (OctreeAS.from_mesh) and on / near that mesh, with their signed distances (wisp.ops.mesh.compute_sdf,
the HIP kernels of csrc/mesh_sdf.hip); resample() subsamples the pool.

Differences from the reference:
  * the pool and the working set stay on the device and `get_batch(indices)` reads a whole batch with one indexed load (the
    trainer's loader uses it); the reference copies everything to the host;
  * with `sample_tex=True` the colours come from wisp.ops.mesh.closest_tex (one HIP launch behind the nearest-triangle search,
    csrc/mesh_tex.hip) over the texture bank OctreeAS.from_mesh(sample_tex=True) keeps in `extent`; `sdf` stays [M,1] there too
    (the reference's textured branch leaves [M], which broadcasts to [B,B] against the field's [B,1] in SDFTrainer.step) and is
    bitwise what compute_sdf gives; a BLAS without materials raises NotImplementedError (the reference asserts "No materials
    detected")."""
import logging as log
from typing import Callable, List, Optional

import torch

import wisp.ops.mesh as mesh_ops
import wisp.ops.spc as wisp_spc_ops
from wisp.accelstructs import BaseAS, OctreeAS
from wisp.datasets.base_datasets import SDFDataset
from wisp.datasets.batch import SDFBatch


class OctreeSampledSDFDataset(SDFDataset):
    """Pool: samples_per_voxel uniform draws per occupied cell of the finest level for each 'rand' entry of `sample_mode`, and as
    many 'near' / 'trace' mesh samples per such entry; the working set is `num_samples` rows of it."""

    def __init__(self,
                 occupancy_struct: OctreeAS,
                 split: str,
                 transform: Optional[Callable] = None,
                 sample_mode: List[str] = None,
                 num_samples: int = 100000,
                 sample_tex: bool = False,
                 samples_per_voxel: int = 32
                 ):
        super().__init__(transform=transform, split=split)
        self.blas = occupancy_struct
        self.sample_mode = sample_mode if sample_mode is not None else ['rand', 'near', 'near', 'trace', 'trace']
        self.num_samples = num_samples
        self.sample_tex = sample_tex
        self.samples_per_voxel = samples_per_voxel
        self.validate()
        if sample_tex and not (self.blas.extent.get('mats') and 'texv' in self.blas.extent and 'texf' in self.blas.extent):
            raise NotImplementedError("OctreeSampledSDFDataset(sample_tex=True): the acceleration structure holds no materials "
                                      "(build it with OctreeAS.from_mesh(..., sample_tex=True) from a mesh that has some)")
        self.data_pool = None
        self.data = None
        self.load()

    @staticmethod
    def supports_blas(blas: BaseAS) -> bool:
        """True for an OctreeAS that keeps its mesh in `extent` (built by OctreeAS.from_mesh)."""
        return isinstance(blas, OctreeAS) and 'vertices' in blas.extent and 'faces' in blas.extent

    def validate(self) -> None:
        if not self.supports_blas(self.blas):
            raise RuntimeError("The Octree acceleration structure was not initialized from a mesh. To use "
                               "an OctreeAS with this dataset, make sure to construct it with a mesh.")

    @property
    def device(self):
        return self.data_pool['coords'].device

    def _sample_from_grid(self, blas: OctreeAS, samples_per_voxel=32):
        dev = torch.device("cuda", torch.cuda.current_device())
        vertices = blas.extent['vertices'].to(dev)
        faces = blas.extent['faces'].to(dev)
        level = blas.max_level
        corners = wisp_spc_ops.unbatched_get_level_points(blas.points, blas.pyramid, level).to(dev)
        pts = []
        for mode in self.sample_mode:                      # the 'rand' draws first, whatever their position in the list
            if mode == "rand":
                pts.append(wisp_spc_ops.sample_spc(corners, level, samples_per_voxel))
        for mode in self.sample_mode:                      # then as many mesh samples as ONE 'rand' entry made, per entry
            if mode == "rand":
                pass
            elif mode == "near":
                pts.append(mesh_ops.sample_near_surface(vertices, faces, pts[0].shape[0], variance=1.0 / (2 ** level)))
            elif mode == "trace":
                pts.append(mesh_ops.sample_surface(vertices, faces, pts[0].shape[0])[0])
            else:
                raise ValueError(f"Sampling mode {mode} not implemented")
        pts = torch.cat(pts, dim=0)
        # Reference quirk, kept (octree_sdf_dataset.py:129): the narrow-band filter queries level 0, whose one cell is the whole
        # cube, so it only drops the points outside [-1, 1]^3.
        pts = pts[self.blas.query(pts, 0).pidx > -1]
        if self.sample_tex:                                # one search gives the distance and the triangle of the colour
            ext = blas.extent
            if 'tex_bank' not in ext:
                ext['tex_bank'] = mesh_ops.TextureBank(ext['mats'])
            rgb, _, d = mesh_ops.closest_tex(vertices, faces, ext['texv'], ext['texf'], ext['tex_bank'], pts)
            return dict(coords=pts, sdf=d[..., None], rgb=rgb)
        d = mesh_ops.compute_sdf(vertices, faces, pts)
        assert d.shape[0] == pts.shape[0]
        return dict(coords=pts, sdf=d)

    def resample(self) -> None:
        """num_samples rows of the pool, drawn without replacement."""
        log.info(f"Resampling {self.num_samples} samples..")
        # Reference quirk, kept (octree_sdf_dataset.py:157): the permutation is of pool_size - 1, so the last pool sample is
        # never drawn.
        idx = torch.randperm(self.pool_size - 1, device=self.device)
        if self.num_samples is not None and self.num_samples < self.pool_size:
            idx = idx[:self.num_samples]
        self.data = {k: v[idx] for k, v in self.data_pool.items() if v is not None}

    def load_singleprocess(self):
        log.info("Computing SDFs for entire samples pool (may take a while)..")
        self.data_pool = self._sample_from_grid(blas=self.blas, samples_per_voxel=self.samples_per_voxel)
        log.info(f"Total Samples in Pool: {self.data_pool['coords'].shape[0]}")
        self.resample()

    @classmethod
    def is_root_of_dataset(cls, root: str, files_list: List[str]) -> bool:
        return False

    def __len__(self):
        return self.data["coords"].shape[0]

    @property
    def pool_size(self) -> int:
        return self.data_pool['coords'].shape[0]

    def __getitem__(self, idx) -> SDFBatch:
        out = SDFBatch(coords=self.data["coords"][idx], sdf=self.data["sdf"][idx],
                       rgb=self.data["rgb"][idx] if "rgb" in self.data else None)
        return self.transform(out) if self.transform is not None else out

    def get_batch(self, indices) -> SDFBatch:
        return self[indices]

    @property
    def coordinates(self) -> torch.Tensor:
        return self.data["coords"]
