"""Test infrastructure of the image application's tests: the reference's ImageDataset and normalized_grid executed from the files
where they lie (their modules import the whole application, so the class / function is compiled on its own), a seeded test image,
and the test's own PNG writer."""
import ast
import functools
import os
import struct
import zlib

import numpy as np
import torch

REF = "/root/reference/wisp"


def have_reference():
    return os.path.isdir(REF)


def _compile_node(rel, name, glb):
    path = os.path.join(REF, rel)
    tree = ast.parse(open(path).read(), path)
    node = next(n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name == name)
    ns = dict(glb)
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def reference_normalized_grid():
    """wisp/ops/geometric.py:65-99, the function itself."""
    return _compile_node("ops/geometric.py", "normalized_grid", dict(torch=torch, np=np))


def reference_image_dataset_class():
    """wisp/datasets/image_dataset.py:37-69, the class itself; geo_ops.normalized_grid is the reference's function bound to
    device='cpu' (its default is 'cuda')."""
    import types
    from PIL import Image
    grid = reference_normalized_grid()
    geo_ops = types.SimpleNamespace(normalized_grid=functools.partial(grid, device='cpu'))
    return _compile_node("datasets/image_dataset.py", "ImageDataset",
                         dict(os=os, torch=torch, np=np, Image=Image, Dataset=torch.utils.data.Dataset, geo_ops=geo_ops))


def reference_trainer_method(name, glb):
    """One method body of wisp/trainers/image_trainer.py's ImageTrainer, decorators dropped (profiler ranges)."""
    path = os.path.join(REF, "trainers/image_trainer.py")
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ImageTrainer")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == name)
    fn.decorator_list = []
    ns = dict(glb)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def reference_psnr():
    return _compile_node("ops/image/metrics.py", "psnr", dict(torch=torch, np=np))


def seeded_image(h, w, seed, channels=3):
    """u8 [h, w, channels]: smooth ramps plus noise, every byte value likely somewhere."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    base = np.stack([(xs * 255) // max(w - 1, 1), (ys * 255) // max(h - 1, 1), ((xs + ys) * 37) % 256] + [np.full((h, w), 200)] * (channels - 3), -1)
    if channels < 3:
        base = base[..., :channels]
    return ((base + rng.integers(0, 64, base.shape)) % 256).astype(np.uint8)


def procedural_image(h, w):
    """A smooth u8 [h, w, 3] image a small field can fit (the GPU tests train on it)."""
    ys, xs = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing='ij')
    img = np.stack([0.5 + 0.5 * np.sin(6 * xs), 0.5 + 0.5 * np.cos(4 * ys), 0.5 + 0.5 * np.sin(5 * xs * ys)], -1)
    return np.clip(img * 255.0, 0, 255).astype(np.uint8)


def write_png(path, img):
    """The tests' own PNG writer (standard library only, filter 0): u8 [H, W] or [H, W, C], C in 1, 3, 4."""
    img = np.ascontiguousarray(img)
    if img.ndim == 2:
        img = img[..., None]
    h, w, ch = img.shape
    body = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * ch)], 1).tobytes()

    def chunk(kind, payload):
        return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[ch], 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(body)) + chunk(b"IEND", b""))


GOLDEN_SIZE = (37, 23)      # height, width
GOLDEN_SEED = 20


def torch_sample(image_u8, indices):
    """The torch restatement of wisp_image_sample (include/wisp_hip.h): CPU tensors in, (coords [n, 2], rgb [n, 3]) out."""
    h, w = image_u8.shape[:2]
    xs, ys = torch.linspace(-1, 1, steps=w), torch.linspace(1, -1, steps=h)
    idx = indices.cpu().reshape(-1)
    idx = torch.where(idx < 0, idx + h * w, idx)
    return torch.stack([xs[idx % w], ys[idx // w]], -1), (image_u8.cpu().reshape(-1, 3) / 255.0)[idx]
