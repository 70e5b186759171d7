"""SDFDataset / MultiviewDataset: the part of the reference's dataset base classes (wisp/datasets/base_datasets.py:22-223:
WispDataset, MultiviewDataset, SDFDataset) that the datasets of this package rely on - constructor fields, load() ->
load_singleprocess() / load_multiprocess(), the item contract.  SDF datasets always load on the calling process (the reference's
multiprocess path only exists for image datasets)."""
from typing import Callable, Optional

import torch

from wisp.datasets.batch import MultiviewBatch, SDFBatch


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


class MultiviewDataset(torch.utils.data.Dataset):
    """Views of one scene (base_datasets.py:148-194): one item = one view's rays with their supervision channels."""

    def __init__(self, dataset_path: str = None, dataset_num_workers: int = -1, transform: Optional[Callable] = None,
                 split: str = None):
        self.dataset_path = dataset_path
        self.dataset_num_workers = dataset_num_workers
        self.transform = transform
        self.split = split

    def name(self) -> str:
        return type(self).__name__

    @classmethod
    def is_root_of_dataset(cls, root: str, files_list) -> bool:
        """Whether the folder `root` (holding `files_list`) is a dataset of this class; classes that do not say are built explicitly."""
        return False

    def load(self):
        """base_datasets.py:97-107: worker processes when dataset_num_workers > 0, else the calling process."""
        if self.dataset_num_workers > 0:
            return self.load_multiprocess()
        return self.load_singleprocess()

    def load_singleprocess(self):
        raise NotImplementedError(f"{self.name()} should override load_singleprocess")

    def load_multiprocess(self):
        raise NotImplementedError(f"{self.name()} should override load_multiprocess")

    @property
    def img_shape(self):
        raise NotImplementedError('MultiviewDatasets should return the shape of their ground truth images')

    @property
    def num_images(self) -> int:
        raise NotImplementedError('MultiviewDatasets should return the number of views they hold')

    @property
    def cameras(self) -> dict:
        return dict()

    def __getitem__(self, idx) -> MultiviewBatch:
        raise NotImplementedError('MultiviewDatasets should override __getitem__')

    def __len__(self):
        return self.num_images
