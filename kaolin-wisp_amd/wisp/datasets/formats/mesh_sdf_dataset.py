"""MeshSampledSDFDataset (wisp/datasets/formats/mesh_sdf_dataset.py:23-215): points sampled on, near and around an OBJ mesh with
their signed distances (wisp.ops.mesh.compute_sdf, the HIP kernels of csrc/mesh_sdf.hip).

Differences from the reference:
  * the samples stay on the device and `get_batch(indices)` reads a whole batch with one indexed load (the trainer's loader uses
    it); the reference copies everything to the host;
  * `sample_tex=True` raises NotImplementedError: textures are not read anywhere in this package."""
import logging as log
import os
from typing import Callable, List, Optional

import torch

import wisp.ops.mesh as mesh_ops
from wisp.datasets.base_datasets import SDFDataset
from wisp.datasets.batch import SDFBatch

_SUPPORTED_FORMATS = ['obj']


class MeshSampledSDFDataset(SDFDataset):
    """`num_samples` points per entry of `sample_mode` ('rand' / 'near' / 'trace', mesh_ops.point_sample), or
    num_samples * len(sample_mode) surface points with their normals when `get_normals`; resample() draws a new set."""

    def __init__(self,
                 mesh_path: str,
                 split: str,
                 transform: Optional[Callable] = None,
                 sample_mode: List[str] = None,
                 num_samples: int = 100000,
                 get_normals: bool = False,
                 sample_tex: bool = False,
                 mode_norm: str = 'sphere'
                 ):
        super().__init__(dataset_path=mesh_path, transform=transform, split=split)
        self.sample_mode = sample_mode if sample_mode is not None else ['rand', 'near', 'near', 'trace', 'trace']
        self.num_samples = num_samples
        self.get_normals = get_normals
        self.sample_tex = sample_tex
        self.mode_norm = mode_norm
        self.verts = self.faces = self.texv = self.texf = self.mats = None
        self.validate(mesh_path)
        if sample_tex:
            raise NotImplementedError("MeshSampledSDFDataset(sample_tex=True): textures are not read by this backend")
        self.data = None
        self.load()

    def validate(self, dataset_path) -> None:
        """FileNotFoundError for a missing path or a format other than .obj (mesh_sdf_dataset.py:83-98)."""
        if not os.path.exists(dataset_path):
            raise FileNotFoundError(f"MeshSampledSDFDataset requires a mesh path, "
                                    f"the dataset_path does not exist: {self.dataset_path}")
        if not any([dataset_path.endswith(ext) for ext in _SUPPORTED_FORMATS]):
            raise FileNotFoundError(f"MeshSampledSDFDataset does not support the mesh format of {self.dataset_path}. "
                                    f"Please use any of the supported formats: {_SUPPORTED_FORMATS}")

    @property
    def device(self):
        return torch.device("cuda", torch.cuda.current_device()) if self.verts is None else self.verts.device

    def load_singleprocess(self) -> None:
        verts, faces = mesh_ops.load_obj(self.dataset_path)
        verts, faces = mesh_ops.normalize(verts, faces, self.mode_norm)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.verts, self.faces = verts.to(dev), faces.to(dev)
        self.resample()

    @classmethod
    def is_root_of_dataset(cls, root: str, files_list: List[str]) -> bool:
        return any([root.endswith(ext) for ext in _SUPPORTED_FORMATS])

    def __len__(self):
        return self.data["coords"].shape[0]

    def __getitem__(self, idx) -> SDFBatch:
        out = SDFBatch(coords=self.data["coords"][idx], sdf=self.data["sdf"][idx],
                       rgb=self.data["rgb"][idx] if "rgb" in self.data else None,
                       normals=self.data["normals"][idx] if "normals" in self.data else None)
        return self.transform(out) if self.transform is not None else out

    def get_batch(self, indices) -> SDFBatch:
        return self[indices]

    def resample(self) -> None:
        """A new working set: coords [M,3] f32, sdf [M,1] f64 (compute_sdf), normals [M,3] with `get_normals`."""
        log.info("Resampling mesh for new sdf samples...")
        nrm = None
        if self.get_normals:
            pts, nrm = mesh_ops.sample_surface(self.verts, self.faces, self.num_samples * len(self.sample_mode))
        else:
            pts = mesh_ops.point_sample(self.verts, self.faces, self.sample_mode, self.num_samples)
        data = dict(coords=pts, sdf=mesh_ops.compute_sdf(self.verts, self.faces, pts))
        if nrm is not None:
            data['normals'] = nrm
        self.data = data

    @property
    def coordinates(self) -> torch.Tensor:
        return self.data["coords"]
