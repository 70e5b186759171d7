"""MeshSampledSDFDataset (wisp/datasets/formats/mesh_sdf_dataset.py:23-215): points sampled on, near and around an OBJ mesh with
their signed distances (wisp.ops.mesh.compute_sdf, the HIP kernels of csrc/mesh_sdf.hip).

Differences from the reference:
  * the samples stay on the device and `get_batch(indices)` reads a whole batch with one indexed load (the trainer's loader uses
    it); the reference copies everything to the host;
  * with `sample_tex=True` the colours come from wisp.ops.mesh.closest_tex (one HIP launch behind the nearest-triangle search,
    csrc/mesh_tex.hip) and the texture bank is built once, not per resample(); `sdf` stays [M,1] there too (the reference's
    textured branch leaves [M], which broadcasts to [B,B] against the field's [B,1] in SDFTrainer.step) and is bitwise what
    compute_sdf gives; a mesh without materials raises NotImplementedError (the reference asserts "No materials detected")."""
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
        self.verts = self.faces = self.texv = self.texf = self.mats = self.tex_bank = None
        self.validate(mesh_path)
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
        texv = texf = None
        if self.sample_tex:                                # parsed and checked on the host, before anything touches a device
            verts, faces, texv, texf, self.mats = mesh_ops.load_obj(self.dataset_path, load_materials=True)
            if not self.mats:
                raise NotImplementedError(f"MeshSampledSDFDataset(sample_tex=True): {self.dataset_path} defines no materials")
            self.tex_bank = mesh_ops.TextureBank(self.mats)
        else:
            verts, faces = mesh_ops.load_obj(self.dataset_path)
        verts, faces = mesh_ops.normalize(verts, faces, self.mode_norm)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.verts, self.faces = verts.to(dev), faces.to(dev)
        if self.sample_tex:
            self.texv, self.texf = texv.to(dev), texf.to(dev)
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
        """A new working set: coords [M,3] f32, sdf [M,1] f64 (compute_sdf), normals [M,3] with `get_normals`, rgb [M,3] f32
        with `sample_tex`."""
        log.info("Resampling mesh for new sdf samples...")
        nrm = None
        if self.get_normals:
            pts, nrm = mesh_ops.sample_surface(self.verts, self.faces, self.num_samples * len(self.sample_mode))
        else:
            pts = mesh_ops.point_sample(self.verts, self.faces, self.sample_mode, self.num_samples)
        if self.sample_tex:                                # one search gives the distance and the triangle of the colour
            rgb, _, d = mesh_ops.closest_tex(self.verts, self.faces, self.texv, self.texf, self.tex_bank, pts)
            data = dict(coords=pts, sdf=d[..., None], rgb=rgb)
        else:
            data = dict(coords=pts, sdf=mesh_ops.compute_sdf(self.verts, self.faces, pts))
        if nrm is not None:
            data['normals'] = nrm
        self.data = data

    @property
    def coordinates(self) -> torch.Tensor:
        return self.data["coords"]
