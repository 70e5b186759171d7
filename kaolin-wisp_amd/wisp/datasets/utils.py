"""load_multiview_dataset (wisp/datasets/utils.py:21-117): pick the MultiviewDataset class whose `is_root_of_dataset` recognises the
folder, and build it with the keyword arguments its constructor takes."""
import inspect
import os
from typing import Callable

from wisp.datasets.base_datasets import MultiviewDataset


def _subclasses(cls):
    return set(cls.__subclasses__()).union(s for c in cls.__subclasses__() for s in _subclasses(c))


def load_multiview_dataset(dataset_path: str, dataset_num_workers: int = -1, transform: Callable = None, split: str = None,
                           **kwargs) -> MultiviewDataset:
    """The dataset class that matches the files under `dataset_path`, constructed.  Ambiguous or unknown folders raise
    RuntimeError; keyword arguments the matched class does not take are dropped, as the reference does."""
    files_list = os.listdir(dataset_path)
    matches = [c for c in _subclasses(MultiviewDataset)
               if not inspect.isabstract(c) and c.is_root_of_dataset(root=dataset_path, files_list=files_list)]
    if len(matches) > 1:
        raise RuntimeError(f"{dataset_path} matches more than one dataset class ({matches}); construct the one you mean directly")
    if not matches:
        raise RuntimeError(f"no multiview dataset class recognises the contents of {dataset_path}")
    cls = matches[0]
    accepted = inspect.signature(cls.__init__).parameters
    ds_args = {k: v for k, v in kwargs.items() if k in accepted}
    return cls(dataset_path=dataset_path, dataset_num_workers=dataset_num_workers, transform=transform, split=split, **ds_args)
