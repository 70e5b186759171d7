"""CPU: the host side of wisp.datasets.NeRFSyntheticDataset - directory rules, frame list, the built-in PNG reader, and the
intrinsics / pose / colour arithmetic against the reference's own `_collect_data_entries`, executed in place from the reference
tree (that one test is skipped where the tree is not mounted).  Datasets are built with device='cpu': the bank can be inspected
there, batches are made on the GPU only (tests/test_gpu_nerf_synthetic.py)."""
import json
import os
import struct
import sys
import types
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/wisp"
ANGLE = 0.6911112


def _zlib_png(path, img, filter_type=0):
    """The test's own PNG writer (no PIL, not the package's writer): u8 [H, W, C], one filter type for every row."""
    h, w, ch = img.shape
    flat = img.reshape(h, w * ch).astype(np.int64)
    rows = bytearray()
    for y in range(h):
        rows.append(filter_type)
        for i in range(w * ch):
            a = flat[y, i - ch] if i >= ch else 0
            b = flat[y - 1, i] if y > 0 else 0
            c = flat[y - 1, i - ch] if (y > 0 and i >= ch) else 0
            if filter_type == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            else:
                pred = (0, a, b, (a + b) // 2)[filter_type]
            rows.append(int(flat[y, i] - pred) % 256)

    def chunk(kind, payload):
        return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[ch], 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(bytes(rows))) + chunk(b"IEND", b""))


def _pose(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, rng.uniform(-4, 4, 3)
    return m


def _scene(root, names=("transforms.json",), folder="images", frames=3, size=(6, 8), channels=4, meta=None, file_path=None):
    """A tiny dataset folder: `names` transform files that all list the same `frames` frames under `folder`."""
    os.makedirs(os.path.join(root, folder), exist_ok=True)
    rng = np.random.default_rng(5)
    imgs, fr = [], []
    for i in range(frames):
        img = rng.integers(0, 256, size + (channels,), dtype=np.uint8)
        _zlib_png(os.path.join(root, folder, f"r_{i}.png"), img, filter_type=i % 5)
        imgs.append(img)
        fp = file_path(i) if file_path else f"./{folder}/r_{i}"
        fr.append(dict(file_path=fp, transform_matrix=_pose(i).tolist()))
    for name in names:
        with open(os.path.join(root, name), "w") as f:
            json.dump(dict(camera_angle_x=ANGLE, **(meta or {}), frames=fr), f)
    return imgs


# ------------------------------------------------------------------------------------------------ 1. file layout
def test_one_transform_file_is_the_train_split_and_other_splits_fall_back(tmp_path):
    from wisp.datasets import NeRFSyntheticDataset, SampleRays, load_multiview_dataset
    imgs = _scene(str(tmp_path))
    find = NeRFSyntheticDataset._validate_and_find_transform
    assert find(str(tmp_path), 'train') == str(tmp_path / "transforms.json")
    assert find(str(tmp_path), 'val') is None and find(str(tmp_path), 'test') is None
    assert NeRFSyntheticDataset.is_root_of_dataset(str(tmp_path), os.listdir(tmp_path))
    ds = NeRFSyntheticDataset(str(tmp_path), split='train', device='cpu')
    assert len(ds) == ds.num_images == 3 and tuple(ds.img_shape) == (6, 8) and ds.has_alpha
    assert list(ds.cameras) == ["r_0", "r_1", "r_2"]                          # frame order
    assert ds.images.dtype == torch.uint8 and tuple(ds.images.shape) == (3, 6, 8, 4)
    assert np.array_equal(ds.images.numpy(), np.stack(imgs))
    assert ds.device_bytes() == 4 * 3 * 6 * 8 + 64 * 3
    val = ds.create_split('val', transform=None)                               # no such split: a shallow copy of this one
    assert type(val) is NeRFSyntheticDataset and val is not ds and val.images is ds.images and val.transform is None
    tr = SampleRays(7)
    assert ds.create_split('test', transform=tr).transform is tr and ds.transform is None
    assert type(load_multiview_dataset(str(tmp_path), split='train', device='cpu', mip=0, unknown_option=1)) is NeRFSyntheticDataset


def test_three_transform_files_are_matched_to_splits_by_name(tmp_path):
    from wisp.datasets import NeRFSyntheticDataset
    names = ("transforms_train.json", "transforms_val.json", "transforms_test.json")
    _scene(str(tmp_path), names=names, folder="train")
    for split, name in zip(("train", "val", "test"), names):
        assert NeRFSyntheticDataset._validate_and_find_transform(str(tmp_path), split) == str(tmp_path / name)
    assert NeRFSyntheticDataset.is_root_of_dataset(str(tmp_path), os.listdir(tmp_path))
    ds = NeRFSyntheticDataset(str(tmp_path), split='train', device='cpu', bg_color=(1.0, 1.0, 1.0), mip=1)
    val = ds.create_split('val')
    assert val.split == 'val' and val.images is not ds.images and val.bg_color == (1.0, 1.0, 1.0) and val.mip == 1
    assert tuple(val.img_shape) == (3, 4)


def test_zero_two_or_four_transform_files_raise_as_the_reference_does(tmp_path):
    from wisp.datasets import NeRFSyntheticDataset
    find = NeRFSyntheticDataset._validate_and_find_transform
    with pytest.raises(FileNotFoundError):
        find(str(tmp_path / "nowhere"), 'train')
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(RuntimeError):
        find(str(empty), 'train')
    for count in (2, 4):
        d = tmp_path / f"n{count}"
        _scene(str(d), names=tuple(f"transforms_{k}.json" for k in ("train", "val", "test", "extra")[:count]))
        with pytest.raises(RuntimeError):
            find(str(d), 'train')
    assert not NeRFSyntheticDataset.is_root_of_dataset(str(empty), [])


def test_frames_with_backslashes_without_extension_and_with_missing_files(tmp_path):
    from wisp.datasets import NeRFSyntheticDataset
    paths = {0: ".\\images\\r_0", 1: "images/r_1.png", 2: "./images/r_2", 3: "./images/not_there"}
    imgs = _scene(str(tmp_path), frames=4, file_path=lambda i: paths[i])
    os.remove(tmp_path / "images" / "r_3.png")
    ds = NeRFSyntheticDataset(str(tmp_path), split='train', device='cpu')
    assert list(ds.cameras) == ["r_0", "r_1", "r_2"]                          # the frame without a file is skipped silently
    assert np.array_equal(ds.images.numpy(), np.stack(imgs[:3]))
    pooled = NeRFSyntheticDataset(str(tmp_path), split='train', device='cpu', dataset_num_workers=2)
    assert list(pooled.cameras) == list(ds.cameras) and torch.equal(pooled.images, ds.images)
    assert torch.equal(pooled.camera_records, ds.camera_records)


def test_views_of_different_sizes_and_sizes_not_divisible_by_the_mip_raise(tmp_path):
    from wisp.datasets import NeRFSyntheticDataset
    _scene(str(tmp_path))
    _zlib_png(str(tmp_path / "images" / "r_1.png"), np.zeros((6, 9, 4), np.uint8))
    with pytest.raises(ValueError):
        NeRFSyntheticDataset(str(tmp_path), split='train', device='cpu')
    imgs = np.zeros((2, 6, 8, 4), np.uint8)
    poses = [_pose(0), _pose(1)]
    with pytest.raises(ValueError):
        NeRFSyntheticDataset.from_arrays(imgs, poses, dict(camera_angle_x=ANGLE), mip=2, device='cpu')      # 6 % 4 != 0
    with pytest.raises(ValueError) as err:
        NeRFSyntheticDataset.from_arrays(imgs, poses, dict(fl_x=100.0), device='cpu')                        # fl_x is not read
    assert "x_fov" in str(err.value) and "camera_angle_x" in str(err.value)
    rgb = NeRFSyntheticDataset.from_arrays(imgs[..., :3], poses, dict(camera_angle_x=ANGLE), device='cpu')
    assert not rgb.has_alpha and int(rgb.images[..., 3].min()) == 255 and rgb.device_bytes() == 4 * 2 * 6 * 8 + 64 * 2


# ------------------------------------------------------------------------------------------------ 2. PNG reader
def _test_images():
    rng = np.random.default_rng(11)
    out = []
    for ch in (1, 3, 4):
        img = rng.integers(0, 256, (19, 23, ch), dtype=np.uint8)
        img[3:12, 2:17] = img[3, 2]                                            # a flat patch: the predictors' tie rules
        yy, xx = np.mgrid[0:19, 0:23]
        img[12:, :, 0] = ((xx * 11 + yy * 7) % 256)[12:]                       # a ramp that wraps
        out.append(img)
    return out


def test_builtin_png_reader_equals_the_tests_own_zlib_writer_for_every_filter(tmp_path):
    from wisp.ops.image import read_png, write_png, load_rgb
    for img in _test_images():
        for ft in range(5):
            path = str(tmp_path / f"z_{img.shape[2]}_{ft}.png")
            _zlib_png(path, img, ft)
            assert np.array_equal(read_png(path), img), (img.shape, ft)
            mine = str(tmp_path / f"w_{img.shape[2]}_{ft}.png")
            write_png(mine, img, ft)                                           # the package's writer makes the same bytes rows
            assert np.array_equal(read_png(mine), img)
    path = str(tmp_path / "z_4_4.png")
    f = load_rgb(path)
    assert f.dtype == np.float32 and f.shape == (19, 23, 4)
    assert np.array_equal(f, _test_images()[2].astype(np.float32) / np.float32(255.0))
    assert np.array_equal(load_rgb(path, normalize=False), _test_images()[2])
    with open(str(tmp_path / "bad.png"), "wb") as fh:
        fh.write(b"not a png")
    with pytest.raises(ValueError):
        read_png(str(tmp_path / "bad.png"))


def test_builtin_png_reader_equals_pil(tmp_path):
    PIL_Image = pytest.importorskip("PIL.Image")
    from wisp.ops.image import read_png, write_png, load_u8
    for img in _test_images():
        ch = img.shape[2]
        for ft in range(5):
            path = str(tmp_path / f"p_{ch}_{ft}.png")
            write_png(path, img, ft)
            pil = np.array(PIL_Image.open(path))
            pil = pil[..., None] if pil.ndim == 2 else pil
            assert np.array_equal(pil, img), (ch, ft)                          # PIL reads what the package writes
            assert np.array_equal(read_png(path), pil)
        path = str(tmp_path / f"pil_{ch}.png")                                 # and the reader reads what PIL writes (its own filters)
        PIL_Image.fromarray(img[..., 0] if ch == 1 else img).save(path)
        assert np.array_equal(read_png(path), img)
        assert np.array_equal(load_u8(path, use_pil=True), load_u8(path, use_pil=False))
    yy, xx = np.mgrid[0:64, 0:64]
    smooth = np.stack([(xx + yy) % 256, (xx * 2) % 256, (yy * 3) % 256, (xx * yy) % 256], -1).astype(np.uint8)
    PIL_Image.fromarray(smooth).save(str(tmp_path / "smooth.png"))
    assert np.array_equal(read_png(str(tmp_path / "smooth.png")), smooth)


# ------------------------------------------------------------------------------------------------ 3. against the reference
def _reference_method(rel, cls_name, meth_name, glb):
    """compile ONE method of a reference class from the file where it lies (the module itself imports the whole application)"""
    import ast
    path = os.path.join(REF, rel)
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == meth_name)
    fn.decorator_list = []
    mod = ast.Module(body=[fn], type_ignores=[])
    ns = dict(glb)
    exec(compile(mod, path, "exec"), ns)
    return ns[meth_name]


class _RecordingCamera:
    """stand-in for kaolin.render.camera.Camera: `from_args` records its arguments; the basis change is the rule DESIGN.md states"""
    made = []

    def __init__(self, **kw):
        self.kw = kw
        self.width, self.height = kw["width"], kw["height"]
        self.view_before = kw["view_matrix"].clone()
        self.view = kw["view_matrix"].clone()

    @classmethod
    def from_args(cls, **kw):
        cam = cls(**kw)
        cls.made.append(cam)
        return cam

    def change_coordinate_system(self, basis):
        self.view[:3, :3] = self.view[:3, :3] @ torch.as_tensor(basis, dtype=torch.float32).T

    def to(self, *a, **k):
        return self


class _TorchRecordingStack:
    """`torch` for the reference method: every attribute is torch's, `stack` remembers what it returned (the method scales the
    stacked poses in place and does not return them)"""

    def __init__(self):
        self.stacked = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def stack(self, tensors, *a, **k):
        out = torch.stack(tensors, *a, **k)
        self.stacked.append(out)
        return out


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not mounted")
@pytest.mark.parametrize("case", ["x_fov", "x_fov_y_fov", "camera_angles", "principal_point_mip1", "scale_offset_aabb", "rgb_only"])
def test_intrinsics_poses_and_colours_equal_the_reference_collect_data_entries(case):
    """NeRFSyntheticDataset._collect_data_entries (datasets/formats/nerf_standard_dataset.py:322-441), the method itself compiled
    from the reference file and run with stand-ins for Kaolin's camera and for the ray generator, against this package's host
    arithmetic (collect_host_entries, PinholeCamera) and its statement of the colour blend (blend_colors_torch: what the GPU tests
    hold the kernel to).  fx / fy, x0 / y0, scaled poses, view matrices before and after the basis change, rgb, masks: equal."""
    import logging
    import typing
    from wisp.core import Rays
    from wisp.datasets import NeRFSyntheticDataset
    from wisp.datasets.formats.nerf_standard_dataset import blend_colors_torch, collect_host_entries
    from wisp.ops.raygen import blender_coords
    meta, mip, bg, channels = dict(camera_angle_x=ANGLE), 0, (0.2, 0.5, 0.7), 4
    if case == "x_fov":
        meta = dict(x_fov=41.5, camera_angle_x=1.0)                            # x_fov wins
    elif case == "x_fov_y_fov":
        meta = dict(x_fov=41.5, y_fov=33.25)
    elif case == "camera_angles":
        meta = dict(camera_angle_x=ANGLE, camera_angle_y=0.52, fl_x=123.0, fl_y=77.0)      # fl_x / fl_y are ignored
    elif case == "principal_point_mip1":
        meta, mip = dict(camera_angle_x=ANGLE, cx=9.25, cy=5.5), 1
    elif case == "scale_offset_aabb":
        meta, bg = dict(camera_angle_x=ANGLE, scale=0.33, offset=[0.5, -0.25, 0.125], aabb_scale=4), (1.0, 1.0, 1.0)
    elif case == "rgb_only":
        channels = 3
    V, H, W = 4, 12, 18
    rng = np.random.default_rng(3)
    bank = rng.integers(0, 256, (V, H, W, channels), dtype=np.uint8)
    if channels == 4:
        bank[..., 3][rng.uniform(size=(V, H, W)) < 0.3] = 0
        bank[..., 3][rng.uniform(size=(V, H, W)) < 0.3] = 255
        bank[0, 0, :4, 3] = (127, 128, 1, 254)
    poses = [_pose(10 + i) for i in range(V)]
    h, w = H >> mip, W >> mip
    # what _load_single_entry hands over: load_rgb's float image (resized when mip > 0: any image of that size serves here) + pose
    imgs = [torch.FloatTensor((bank[i, :h, :w].astype(np.float32) / np.float32(255.0))) for i in range(V)]
    _RecordingCamera.made = []
    rec = _TorchRecordingStack()
    glb = dict(torch=rec, np=np, log=logging, Rays=Rays, Camera=_RecordingCamera, blender_coords=blender_coords,
               generate_centered_pixel_coords=lambda *a, **k: (torch.zeros(1), torch.zeros(1)),
               generate_pinhole_rays=lambda cam, grid: Rays(torch.zeros(cam.height * cam.width, 3), torch.zeros(cam.height * cam.width, 3)),
               Dict=typing.Dict, Union=typing.Union, List=typing.List, Optional=typing.Optional, Tuple=typing.Tuple)
    collect = _reference_method("datasets/formats/nerf_standard_dataset.py", "NeRFSyntheticDataset", "_collect_data_entries", glb)
    me = types.SimpleNamespace(mip=mip, bg_color=bg)
    names = [f"r_{i}" for i in range(V)]
    want = collect(me, metadata=meta, basenames=names, imgs=imgs, poses=[torch.FloatTensor(np.array(p)) for p in poses])
    ref_poses = rec.stacked[1]                                                 # (stack 0: the images, stack 1: the poses, scaled in place)

    got = collect_host_entries(meta, (H, W), poses, mip)
    cams = _RecordingCamera.made
    assert len(cams) == V and list(want["cameras"]) == names
    assert (got["h"], got["w"]) == (cams[0].kw["height"], cams[0].kw["width"]) == (h, w)
    f32 = np.float32
    for key, mine in (("focal_x", got["fx"]), ("focal_y", got["fy"]), ("x0", got["x0"]), ("y0", got["y0"])):
        assert f32(mine) == f32(cams[0].kw[key]), (key, mine, cams[0].kw[key])
        assert float(mine) == float(cams[0].kw[key])                           # and as the doubles they are formed in
    assert cams[0].kw["near"] == 1.0 and cams[0].kw["far"] == 5.0
    assert torch.equal(got["poses"], ref_poses)
    for i in range(V):
        assert torch.equal(got["view_matrices"][i], cams[i].view_before)

    if mip == 0:
        ds = NeRFSyntheticDataset.from_arrays(bank, poses, meta, basenames=names, bg_color=bg, mip=mip, device='cpu')
        assert list(ds.cameras) == names and tuple(ds.img_shape) == (h, w)
        for i, cam in enumerate(ds.cameras.values()):
            assert torch.equal(cam.view_matrix()[0], cams[i].view)             # after the change of basis
            assert (cam.focal_x, cam.focal_y, cam.x0, cam.y0, cam.near, cam.far) == (got["fx"], got["fy"], got["x0"], got["y0"], 1.0, 5.0)
            assert cam.tan_half_fov('horizontal') == (w / 2) / got["fx"] and cam.tan_half_fov('vertical') == (h / 2) / got["fy"]
            rec16 = ds.camera_records[i]
            assert torch.equal(rec16[:9].reshape(3, 3), cams[i].view[:3, :3]) and torch.equal(rec16[9:12], cams[i].view[:3, 3])
        rgb, masks = blend_colors_torch(ds.images, bg, has_alpha=ds.has_alpha)
        want_rgb = torch.as_tensor(np.asarray(want["rgb"]), dtype=torch.float32)
        assert rgb.dtype == torch.float32 and torch.equal(rgb, want_rgb)
        assert masks.dtype == torch.bool and torch.equal(masks, want["masks"])
        assert bool(masks.all()) == (channels == 3)


def test_a_world_point_of_the_file_becomes_x_z_minus_y():
    """The basis change in words: the camera sees the same picture, and a world point (x, y, z) of the file
    is (x, z, -y) afterwards - Blender's z-up becomes y-up."""
    from wisp.ops.raygen import PinholeCamera, blender_coords
    from wisp.datasets.formats.nerf_standard_dataset import collect_host_entries
    pose = _pose(4)
    host = collect_host_entries(dict(camera_angle_x=ANGLE, aabb_scale=1.0), (8, 8), [pose], 0)
    cam = PinholeCamera.from_args(view_matrix=host["view_matrices"][0], focal_x=host["fx"], focal_y=host["fy"], width=8, height=8)
    before = cam.view_matrix()[0].double()
    cam.change_coordinate_system(blender_coords())
    after = cam.view_matrix()[0].double()
    p = torch.tensor([0.3, -1.2, 0.7, 1.0], dtype=torch.float64)
    q = torch.tensor([0.3, 0.7, 1.2, 1.0], dtype=torch.float64)               # (x, z, -y)
    assert torch.allclose(before @ p, after @ q, atol=1e-6)
    eye_file = torch.as_tensor(pose[:3, 3])
    eye_after = -(after[:3, :3].T @ after[:3, 3])
    assert torch.allclose(eye_after, torch.stack([eye_file[0], eye_file[2], -eye_file[1]]), atol=1e-5)


def test_written_synlego_scene_reproduces_synlego_rays(tmp_path):
    """scripts/train_nerf_synthetic.py --write-synlego: the cameras the dataset reads back from the files give the rays
    synlego.pixel_rays gives (oracle ray generator on the host), so the scene on disk is the scene bench.py trains on."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from train_nerf_synthetic import write_synlego_scene
    finally:
        sys.path.pop(0)
    import synlego
    from oracle import raygen as orc
    from wisp.datasets import load_multiview_dataset
    from wisp.ops.raygen.raygen import _view_transform
    res = 16
    write_synlego_scene(str(tmp_path), views=(2, 1, 1), res=res, steps=48)
    ds = load_multiview_dataset(str(tmp_path), split='train', device='cpu')
    assert len(ds) == 2 and ds.has_alpha and len(ds.create_split('val')) == 1
    rot, pos = synlego.cameras(2, seed=0)
    py, px = torch.meshgrid(torch.arange(res), torch.arange(res), indexing='ij')
    gy, gx = orc.centered_pixel_coords(res, res)
    for i, cam in enumerate(ds.cameras.values()):
        o, d = synlego.pixel_rays(rot, pos, torch.full((res * res,), i), px.reshape(-1), py.reshape(-1), res)
        R, t = _view_transform(cam)
        ow, dw = orc.generate_rays(gx, gy, False, cam.x0, cam.y0, res, res, cam.tan_half_fov('horizontal'),
                                   cam.tan_half_fov('vertical'), R, t)
        assert np.abs(ow - o.numpy()).max() < 1e-5 and np.abs(dw - d.numpy()).max() < 1e-5
    alpha = ds.images[..., 3]
    assert int(alpha.min()) == 0 and int(alpha.max()) == 255                   # the brick assembly against empty space


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_multiview_sample_is_declared_bound_and_exported():
    import ctypes
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    assert "int wisp_multiview_sample(" in header
    assert "wisp_multiview_sample" in C.SIGNATURES and len(C.SIGNATURES["wisp_multiview_sample"]) == 22
    lib = ctypes.CDLL(C.LIB_PATH)
    assert hasattr(lib, "wisp_multiview_sample")
    assert C.lib.wisp_abi_version() == 4
    # argument checks that need no device memory: they fail before any launch
    f = C._cdll.wisp_multiview_sample
    null = ctypes.c_void_p(0)
    base = [null, null, null, 1, 8, 8, 0, 1, null, null, 0, 4, 0.0, 0.0, 1.0, 1.0, null, null, null, null, null, null]
    for patch in ({11: -1}, {6: 6}, {6: -1}, {}, {4: 6, 6: 2}):               # negative count, mip out of range, null pix, size % 2^mip
        args = list(base)
        for k, v in patch.items():
            args[k] = v
        assert f(*args) == -1, patch                                           # WISP_ERR_INVALID
    args = list(base)
    args[11] = 0
    assert f(*args) == 0                                                       # nothing to do
