"""ImageDataset: one image to fit with a neural field (wisp/datasets/image_dataset.py:37-69).

The reference keeps, on the host, the image divided by 255, the [H*W, 2] coordinate grid and the [H*W, 3] pixel view - 32 bytes per
pixel - and every item is a CPU randint, two CPU gathers and a copy to the device.  Here the bank is what the file held - 8-bit
RGB, 3 bytes per pixel, on `device` - and an item is one on-device randint plus one launch (wisp_image_sample, csrc/image_field.hip)
that turns the indices into coordinates and colours.  `coords` / `pixels` / `get_image()` still hand out the reference's tensors,
materialised on demand in plain torch (20 bytes per pixel for the first two): nothing in this package calls them while training or
validating."""
import os

import torch
from torch.utils.data import Dataset

import wisp.ops.geometric as geo_ops
from wisp.ops.image import load_u8


class ImageDataset(Dataset):
    def __init__(self, dataset_path: str, num_pixels_per_image: int = 4096, device='cuda'):
        self.root = os.path.abspath(os.path.expanduser(dataset_path))
        image = torch.from_numpy(load_u8(self.root))
        self.num_pixels_per_image = num_pixels_per_image
        if not image.shape[-1] == 3:
            raise Exception("Alpha channel detected for image."
                            "You should create a 3 channel RGB with alpha channels dealt in whatever way makes sense.")
        self.h, self.w = image.shape[:2]
        self.device = torch.device(device)
        self.image_u8 = image.contiguous().to(self.device)                  # the bank: u8 [h, w, 3]

    # ---- the reference's tensors, on demand (host layout: fp32 on the CPU)
    def get_image(self):
        return self.image_u8.cpu() / 255.0

    @property
    def coords(self):
        return geo_ops.normalized_grid(self.h, self.w, device='cpu', use_aspect=False).reshape(-1, 2)

    @property
    def pixels(self):
        return self.get_image().reshape(-1, 3)

    def __len__(self):
        return 100

    def sample(self, indices):
        """(coords [n, 2], rgb [n, 3]) of the pixels `indices` (i64, row * w + col), on the bank's device."""
        if self.image_u8.is_cuda:
            import wisp._C as _C
            out = _C.image_sample(self.image_u8, indices.to(self.device))
            return out["coords"], out["rgb"]
        indices = indices.reshape(-1)
        return self.coords[indices], self.pixels[indices]

    def __getitem__(self, idx: int):
        rand_idx = torch.randint(0, self.h * self.w, (self.num_pixels_per_image,), device=self.device)
        return self.sample(rand_idx)
