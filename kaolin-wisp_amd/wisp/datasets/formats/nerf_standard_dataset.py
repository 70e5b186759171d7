"""NeRFSyntheticDataset: files in the standard NeRF / instant-ngp layout (transforms*.json + images) -> training rays
(wisp/datasets/formats/nerf_standard_dataset.py:30-466), with a device layout of its own.

The reference keeps fp32 origins, directions and colours plus a mask for every pixel of every view: 37 bytes per pixel, 2.3 GB for
100 views of 800 x 800.  Here the device holds what the files held - one u8 RGBA bank [V, H, W, 4], 4 bytes per pixel - and one
64-byte camera record per view; rays, background-blended colours and masks are made from (view, pixel) indices by one HIP launch
(csrc/dataset.hip, wisp_multiview_sample) when a batch is asked for.  `mip > 0` does not resize the bank: the kernel averages the
2^mip x 2^mip block behind a pixel on the fly.  (The reference resizes with cv2.INTER_AREA, a box mean for such sizes; cv2 is not a
dependency here, so its rounding is not pinned - the summation order is the one include/wisp_hip.h states.)

Host side (no GPU needed): directory rules, frame list, image decoding (wisp.ops.image: PIL, or the built-in PNG reader), the
intrinsics / pose arithmetic of `_collect_data_entries` with its quirks.  The basis change from Blender's world is
PinholeCamera.change_coordinate_system (wisp/ops/raygen/raygen.py); Kaolin's own rule is not pinned, see DESIGN.md section 6.
"""
import copy
import glob
import json
import logging as log
import os
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from wisp.core import Rays
from wisp.datasets.base_datasets import MultiviewDataset
from wisp.datasets.batch import MultiviewBatch
from wisp.datasets.transforms import SampleRays
from wisp.ops.raygen import PinholeCamera, blender_coords
from wisp.ops.raygen.raygen import _axis_tan, _scalar, _view_transform

DEFAULT_NEAR, DEFAULT_FAR = 1.0, 5.0          # nerf_standard_dataset.py:401-403


def _hip():
    import wisp._C as _C
    return _C


def _decode_entry(args):
    """One frame of the transform file -> (basename, u8 [H, W, C], pose 4x4) or None when its image does not exist
    (nerf_standard_dataset.py:213-243).  Runs in pool workers too: host code only, nothing here touches the GPU."""
    frame, root = args
    from wisp.ops.image import load_u8
    path = os.path.join(root, frame['file_path'].replace("\\", "/"))      # Windows-written files use backslashes
    stem, ext = os.path.splitext(path)
    if not ext:
        path = stem + '.png'                  # the NeRF-synthetic convention: no extension means PNG
    if not os.path.exists(path):
        return None                           # frames whose image is missing are skipped silently, as instant-ngp allows
    return os.path.basename(stem), load_u8(path), np.array(frame['transform_matrix'])


def collect_host_entries(metadata: dict, image_hw: Tuple[int, int], poses, mip: int = 0) -> dict:
    """The intrinsics and pose arithmetic of `_collect_data_entries` (nerf_standard_dataset.py:338-412) for stored images of
    `image_hw` = (H, W) and camera-to-world `poses` [V, 4, 4] -> dict(h, w, fx, fy, x0, y0, poses, view_matrices): h, w the
    mip-sized image, fx / fy Python floats (doubles, as numpy forms them there), poses the scaled fp32 camera-to-world matrices
    and view_matrices [V, 4, 4] = [R^T | -R^T t] of those, BEFORE the change of basis."""
    H, W = int(image_hw[0]), int(image_hw[1])
    if mip < 0 or mip > 5:
        raise ValueError(f"mip must be in 0..5, got {mip}")
    if H % (1 << mip) or W % (1 << mip):
        raise ValueError(f"image size {H} x {W} is not a multiple of 2^mip = {1 << mip}")
    h, w = H >> mip, W >> mip
    if 'x_fov' in metadata:                   # degrees
        fx = (0.5 * w) / np.tan(0.5 * float(metadata['x_fov']) * (np.pi / 180.0))
        fy = (0.5 * h) / np.tan(0.5 * float(metadata['y_fov']) * (np.pi / 180.0)) if 'y_fov' in metadata else fx
    elif 'camera_angle_x' in metadata:        # radians.  ('fl_x' / 'fl_y' are ignored: the reference's branch is `and False`, :349)
        fx = (0.5 * w) / np.tan(0.5 * float(metadata['camera_angle_x']))
        fy = (0.5 * h) / np.tan(0.5 * float(metadata['camera_angle_y'])) if 'camera_angle_y' in metadata else fx
    else:
        raise ValueError("the transform file gives no field of view: looked for 'x_fov' (with optional 'y_fov') and "
                         "'camera_angle_x' (with optional 'camera_angle_y'); 'fl_x' / 'fl_y' are not read")
    for key, what in (('fix_premult', 'premultiplied-alpha correction'), ('k1', 'lens distortion correction'),
                      ('rolling_shutter', 'rolling shutter correction')):
        if key in metadata:               # the reference only warns about these too (:370-380)
            log.info(f"WARNING: the transform file asks for {what} ('{key}'), which this dataset does not apply.")
    # principal point: the file stores an absolute pixel position, wisp a displacement from the image centre (:382-390)
    x0 = (float(metadata['cx']) / (2 ** mip)) - (w // 2) if 'cx' in metadata else 0.0
    y0 = (float(metadata['cy']) / (2 ** mip)) - (h // 2) if 'cy' in metadata else 0.0
    offset = torch.tensor(metadata.get('offset', [0, 0, 0]), dtype=torch.float32)
    scale, aabb_scale = metadata.get('scale', 1.0), metadata.get('aabb_scale', 1.25)
    c2w = torch.stack([torch.as_tensor(np.array(p), dtype=torch.float32) for p in poses]).clone()
    # t / aabb_scale * scale + offset, three fp32 roundings in this order (:397-399)
    t = c2w[:, :3, 3]
    t = t / aabb_scale
    t = t * scale
    c2w[:, :3, 3] = t + offset
    # world -> camera: [R^T | -R^T t] (:409-412), the product formed by torch.matmul of the negated rotation as it is there
    w2c = torch.zeros_like(c2w)
    for v in range(c2w.shape[0]):
        rot_t = c2w[v, :3, :3].T
        w2c[v, :3, :3] = rot_t
        w2c[v, :3, 3] = torch.matmul(-w2c[v, :3, :3], c2w[v, :3, 3])
        w2c[v, 3, 3] = 1.0
    return dict(h=h, w=w, fx=float(fx), fy=float(fy), x0=float(x0), y0=float(y0), poses=c2w, view_matrices=w2c)


def u8_to_unit_float(images_u8: torch.Tensor) -> torch.Tensor:
    """fp32 `u8 / 255.0` as load_rgb forms it on the host (ops/image/io.py:83, an IEEE division).  The 256 quotients are formed on
    the CPU and looked up: torch's GPU division by a Python scalar multiplies by the reciprocal, which is not the same number for
    every u8."""
    lut = torch.arange(256, dtype=torch.float32) / 255.0
    return lut.to(images_u8.device)[images_u8.long()]


def blend_colors_torch(images_u8: torch.Tensor, bg_color, has_alpha: bool = True):
    """(rgb f32 [..., 3], masks bool [..., 1]) of a u8 [..., 4] bank: the torch expression of nerf_standard_dataset.py:432-439
    on load_rgb's floats, op by op, on whatever device the bank is on.  It is the yardstick the tests hold the kernel to (and is
    itself held to the reference's method); the dataset never calls it."""
    imgs = u8_to_unit_float(images_u8)
    rgbs = imgs[..., :3]
    if not has_alpha:
        return rgbs, torch.ones_like(rgbs[..., 0:1]).bool()
    alpha = imgs[..., 3:4]
    masks = (alpha > 0.5).bool()
    bg = torch.tensor(np.array(bg_color).astype(np.float32), device=images_u8.device)
    rgbs = rgbs * alpha + (1 - alpha) * bg
    return torch.clamp(rgbs, 0.0, 1.0), masks


class NeRFSyntheticDataset(MultiviewDataset):
    """A dataset for files in the standard NeRF format, including the extensions instant-ngp reads (RGBA / RGB images)."""

    def __init__(self, dataset_path: str, split: str, bg_color: Tuple[float, float, float] = (0.0, 0.0, 0.0), mip: int = 0,
                 dataset_num_workers: int = -1, transform: Optional[Callable] = None, device=None):
        """dataset_path: root directory with the transform json file(s) and the images.  split: 'train' / 'val' / 'test' (a
        single transform file is the 'train' split).  bg_color: what alpha = 0 shows.  mip: work at 1 / 2^mip of the stored
        size.  dataset_num_workers > 0: decode the images in that many worker processes.  transform: applied per batch by
        __getitem__ (SampleRays is recognised and runs fused).  device: where the bank lives (default: the GPU when there is
        one; a bank on the CPU can be built and inspected, but batches are made on the GPU only)."""
        super().__init__(dataset_path=dataset_path, dataset_num_workers=dataset_num_workers, transform=transform, split=split)
        self.mip = mip
        self.bg_color = bg_color
        self.device = device
        self._transform_file = self._validate_and_find_transform(self.dataset_path, self.split)
        if self._transform_file is None:
            raise RuntimeError(f"NeRF dataset folder {dataset_path} has no transform file for split {split!r}")
        self.load()

    # ------------------------------------------------------------------------------------------ files
    @classmethod
    def is_root_of_dataset(cls, root: str, files_list: List[str]) -> bool:
        """The two layouts of nerf_standard_dataset.py:136-165: `transforms.json` next to a folder `images`, or
        `transforms_train.json` next to a folder `train` (only the train split is looked for)."""
        names = set(files_list)
        for json_name, folder in (('transforms.json', 'images'), ('transforms_train.json', 'train')):
            if json_name in names and folder in names:
                return os.path.isdir(os.path.join(root, folder))
        return False

    @staticmethod
    def _validate_and_find_transform(dataset_path: str, split: str) -> Optional[str]:
        """The transform file of `split`, or None when the dataset has no such split (nerf_standard_dataset.py:167-211).  One
        *.json in the folder is the 'train' split whatever its name; three are 'test' / 'train' / 'val', each matched by that
        word appearing in the file name; none, two or more than three raise RuntimeError."""
        if not os.path.exists(dataset_path):
            raise FileNotFoundError(f"NeRF dataset path does not exist: {dataset_path}")
        found = sorted(glob.glob(os.path.join(dataset_path, "*.json")))
        if not found:
            raise RuntimeError(f"no transform *.json file with camera data in NeRF dataset folder {dataset_path}")
        if len(found) not in (1, 3):
            raise RuntimeError(f"a NeRF dataset folder holds one transform file or the three splits ['test', 'train', 'val']; "
                               f"found {found}")
        if len(found) == 1:
            return found[0] if split == 'train' else None
        by_split = {}
        for name in ('test', 'train', 'val'):
            for path in found:                 # (a later file name that also holds the word wins, as in the reference)
                if name in os.path.basename(path):
                    by_split[name] = path
        return by_split.get(split)

    def create_split(self, split: str, transform: Optional[Callable] = None):
        """A dataset with the same settings and another split; when that split does not exist, a shallow copy of this one (same
        bank) with the new transform (nerf_standard_dataset.py:79-111)."""
        if self._validate_and_find_transform(self.dataset_path, split) is None:
            log.warning(f"WARNING: Split type ['{split}'] does not exist in the dataset. Falling back to {self.split} data.")
            validation_split = copy.copy(self)
            validation_split.transform = transform
            return validation_split
        return type(self)(dataset_path=self.dataset_path, split=split, bg_color=self.bg_color, mip=self.mip,
                          dataset_num_workers=self.dataset_num_workers, transform=transform, device=self.device)

    def load_singleprocess(self):
        return self._load(None)

    def load_multiprocess(self):
        return self._load(self.dataset_num_workers)

    def _load(self, workers):
        with open(self._transform_file, 'r') as f:
            metadata = json.load(f)
        entries = [(frame, self.dataset_path) for frame in metadata['frames']]
        if workers:
            from multiprocessing import Pool
            pool = Pool(workers)
            try:
                decoded = list(pool.imap(_decode_entry, entries))
            finally:
                pool.close()
                pool.join()
        else:
            decoded = [_decode_entry(e) for e in entries]
        decoded = [d for d in decoded if d is not None]
        if not decoded:
            raise RuntimeError(f"none of the {len(entries)} frames of {self._transform_file} has an image on disk")
        self._init_from_arrays([d[1] for d in decoded], [d[2] for d in decoded], metadata, [d[0] for d in decoded])
        return self

    # ------------------------------------------------------------------------------------------ arrays -> device
    @classmethod
    def from_arrays(cls, images_u8, poses, metadata: dict, basenames: Optional[List[str]] = None,
                    bg_color: Tuple[float, float, float] = (0.0, 0.0, 0.0), mip: int = 0, transform: Optional[Callable] = None,
                    device=None, split: str = 'train', dataset_path: str = None, dataset_num_workers: int = -1):
        """The same object from arrays in memory: images_u8 [V, H, W, 3 | 4] (or a list of [H, W, C]) as the files would hold
        them, poses [V, 4, 4] camera-to-world as `transform_matrix`, metadata the transform file's top-level dict."""
        self = cls.__new__(cls)
        MultiviewDataset.__init__(self, dataset_path=dataset_path, dataset_num_workers=dataset_num_workers, transform=transform,
                                  split=split)
        self.mip, self.bg_color, self.device, self._transform_file = mip, bg_color, device, None
        self._init_from_arrays(list(images_u8), list(poses), metadata, basenames)
        return self

    def _init_from_arrays(self, images, poses, metadata, basenames):
        images = [np.asarray(im) for im in images]
        if len(images) == 0 or len(images) != len(poses):
            raise ValueError(f"{len(images)} images for {len(poses)} poses")
        shape = images[0].shape
        if any(im.shape != shape for im in images):
            raise ValueError(f"all views must share one size and channel count; found {sorted({im.shape for im in images})}")
        if len(shape) != 3 or shape[2] not in (3, 4) or any(im.dtype != np.uint8 for im in images):
            raise ValueError(f"images must be uint8 [H, W, 3] or [H, W, 4], got {images[0].dtype} {shape}")
        H, W, C = shape
        host = collect_host_entries(metadata, (H, W), poses, self.mip)
        V = len(images)
        if basenames is None:
            basenames = [f"r_{i}" for i in range(V)]
        if self.device is None:
            self.device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.has_alpha = C == 4
        self.focal_x, self.focal_y, self.x0, self.y0 = host['fx'], host['fy'], host['x0'], host['y0']
        self.poses, self.view_matrices = host['poses'], host['view_matrices']
        self._img_shape = torch.Size([host['h'], host['w']])
        cams: Dict[str, PinholeCamera] = dict()
        records = np.zeros((V, 16), dtype=np.float32)
        for i in range(V):
            camera = PinholeCamera.from_args(view_matrix=host['view_matrices'][i], focal_x=host['fx'], focal_y=host['fy'],
                                             width=host['w'], height=host['h'], far=DEFAULT_FAR, near=DEFAULT_NEAR,
                                             x0=host['x0'], y0=host['y0'], dtype=torch.float)
            camera.change_coordinate_system(blender_coords())
            cams[basenames[i]] = camera
            # the record is read off the camera the way generate_pinhole_rays reads it, so both give the kernels the same floats
            records[i, :9], records[i, 9:12] = _view_transform(camera)
        self._cameras = cams
        self._camera_list = list(cams.values())
        if len(cams) != V:
            raise ValueError("two frames share a basename; cameras are keyed by it")
        first = self._camera_list[0]
        self._tan = (np.float32(_axis_tan(first, True)), np.float32(_axis_tan(first, False)))
        self._principal = (np.float32(_scalar(first.x0)), np.float32(_scalar(first.y0)))
        bank = np.empty((V, H, W, 4), dtype=np.uint8)
        for i, im in enumerate(images):
            bank[i, ..., :C] = im
        if C == 3:
            bank[..., 3] = 255
        self._records_host = records
        self.images = torch.from_numpy(bank).to(self.device)               # u8 [V, H, W, 4]: the only per-pixel data held
        self.camera_records = torch.from_numpy(records).to(self.device)    # f32 [V, 16]
        self._shared = {}                                                  # `data` cache, shared with shallow copies

    # ------------------------------------------------------------------------------------------ batches
    def _launch(self, pix, view=None, view_index=0, want=("origins", "dirs", "rgb", "mask")):
        out = _hip().multiview_sample(self.images, pix, view=view, view_index=view_index, cameras=self.camera_records,
                                      camera_host=None if view is not None else self._records_host[view_index], mip=self.mip,
                                      has_alpha=self.has_alpha, x0=self._principal[0], y0=self._principal[1], tan_x=self._tan[0],
                                      tan_y=self._tan[1], bg=self.bg_color, want=want)
        return MultiviewBatch(rays=Rays(out["origins"], out["dirs"], dist_min=DEFAULT_NEAR, dist_max=DEFAULT_FAR),
                              rgb=out["rgb"], masks=out["mask"])

    def _view_index(self, idx):
        idx = int(idx)
        n = len(self._camera_list)
        if not -n <= idx < n:
            raise IndexError(f"view {idx} of a dataset of {n}")
        return idx % n

    def view(self, idx) -> MultiviewBatch:
        """The whole view `idx`: H*W rays in row-major pixel order, their colours and masks [H*W, 1]."""
        h, w = self._img_shape
        return self._launch(torch.arange(h * w, dtype=torch.int64, device=self.images.device), view_index=self._view_index(idx))

    def iter_views(self):
        """(Rays [H*W, 3], rgb [H*W, 3]) per view - what wisp.trainers.validation.evaluate_psnr takes."""
        for i in range(len(self)):
            batch = self.view(i)
            yield batch['rays'], batch['rgb']

    def __getitem__(self, idx) -> MultiviewBatch:
        """A batch of rays of view `idx` with "rgb" and "masks" (mask = alpha > 0.5), nerf_standard_dataset.py:113-134.  With a
        SampleRays transform the pixels are drawn exactly as SampleRays draws them and only those rays are made (one launch);
        any other transform receives the whole view."""
        if isinstance(self.transform, SampleRays):
            h, w = self._img_shape
            torch.cuda.nvtx.range_push("SampleRays")                       # the range SampleRays itself opens (ray_sampler.py:24)
            try:
                pix = torch.randint(0, h * w, [self.transform.num_samples], device=self.images.device, generator=None)
                return self._launch(pix, view_index=self._view_index(idx))
            finally:
                torch.cuda.nvtx.range_pop()
        out = self.view(idx)
        return out if self.transform is None else self.transform(out)

    def sample(self, num_rays: int, generator=None) -> MultiviewBatch:
        """`num_rays` rays drawn uniformly over all pixels of all views (what MultiviewTrainStep.step(rays, gts) consumes); the
        batch also names where each ray came from: "view_idx", "pixel_idx" (int64 [num_rays])."""
        h, w = self._img_shape
        dev = self.images.device
        view = torch.randint(0, len(self), [num_rays], device=dev, generator=generator)
        pix = torch.randint(0, h * w, [num_rays], device=dev, generator=generator)
        out = self._launch(pix, view=view)
        out['view_idx'], out['pixel_idx'] = view, pix
        return out

    # ------------------------------------------------------------------------------------------ the reference's fields
    @property
    def data(self) -> dict:
        """The reference's resident layout, materialised on first access and cached: "rays" Rays [V, H*W, 3], "rgb" [V, H*W, 3],
        "masks" [V, H*W, 1] (flattened as flatten_tensors does, :443-450), "cameras".  MultiviewTrainer.validate reads it.
        This costs the 37 bytes per pixel the class otherwise avoids - meant for validation splits, not for training."""
        if "data" not in self._shared:
            views = [self.view(i) for i in range(len(self))]
            self._shared["data"] = dict(rays=Rays.stack([b['rays'] for b in views]), rgb=torch.stack([b['rgb'] for b in views]),
                                        masks=torch.stack([b['masks'] for b in views]), cameras=self._cameras)
        return self._shared["data"]

    def device_bytes(self) -> int:
        """Bytes this dataset holds on its device: the bank and the camera records, 4 * V * H * W + 64 * V - plus the resident
        layout once `data` has been asked for."""
        total = self.images.numel() * self.images.element_size() + self.camera_records.numel() * self.camera_records.element_size()
        cached = self._shared.get("data")
        if cached is not None:
            for t in (cached["rays"].origins, cached["rays"].dirs, cached["rgb"], cached["masks"]):
                total += t.numel() * t.element_size()
        return total

    @property
    def img_shape(self) -> torch.Size:
        """(H >> mip, W >> mip): the size of the images batches are drawn from."""
        return self._img_shape

    @property
    def cameras(self) -> Dict[str, PinholeCamera]:
        """basename -> camera, in frame order."""
        return self._cameras

    @property
    def num_images(self) -> int:
        return len(self._camera_list)
