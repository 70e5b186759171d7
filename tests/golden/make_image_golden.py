"""Writes tests/golden/image_dataset_ref.npz: the reference's ImageDataset (wisp/datasets/image_dataset.py), executed where it
lies on a 37 x 23 RGB PNG generated from a seed, with geo_ops.normalized_grid bound to device='cpu'.  Data only: the u8 image,
`coords` [851, 2] and `pixels` [851, 3].  The GPU tests have no reference tree; this file holds them to its output.

    python tests/golden/make_image_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_ref                                                       # noqa: E402


def main():
    h, w = image_ref.GOLDEN_SIZE
    img = image_ref.seeded_image(h, w, image_ref.GOLDEN_SEED)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "golden.png")
        image_ref.write_png(path, img)
        ds = image_ref.reference_image_dataset_class()(path, num_pixels_per_image=64)
    assert (ds.h, ds.w) == (h, w) and len(ds) == 100
    out = os.path.join(HERE, "image_dataset_ref.npz")
    np.savez_compressed(out, image=img, coords=ds.coords.numpy(), pixels=ds.pixels.numpy().astype(np.float32))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
