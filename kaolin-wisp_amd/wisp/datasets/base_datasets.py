"""SDFDataset: the part of the reference's dataset base classes (wisp/datasets/base_datasets.py:22-223: WispDataset, SDFDataset)
that the mesh-sampled SDF datasets rely on - constructor fields, load() -> load_singleprocess(), the item contract.  Loading
always runs on the calling process (the reference's multiprocess path only exists for image datasets)."""
from typing import Callable, Optional

import torch

from wisp.datasets.batch import SDFBatch


class SDFDataset(torch.utils.data.Dataset):
    """(coordinate, supervision) samples of a signed-distance function; `resample()` refreshes the working set in place."""

    def __init__(self, dataset_path: str = None, dataset_num_workers: int = -1, transform: Optional[Callable] = None,
                 split: str = None):
        self.dataset_path = dataset_path
        self.dataset_num_workers = dataset_num_workers
        self.transform = transform
        self.split = split

    def name(self) -> str:
        return type(self).__name__

    def load(self):
        return self.load_singleprocess()

    def load_singleprocess(self):
        raise NotImplementedError(f"{self.name()} should override load_singleprocess")

    @property
    def coordinates(self) -> torch.Tensor:
        raise NotImplementedError('SDFDatasets should return a (N, d) tensor of sample coordinates.')

    def resample(self) -> None:
        pass

    def __getitem__(self, idx) -> SDFBatch:
        raise NotImplementedError('SDFDataset should override __getitem__')

    def __len__(self):
        raise NotImplementedError('SDFDataset should override __len__')
