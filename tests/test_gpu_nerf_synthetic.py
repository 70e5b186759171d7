"""GPU: wisp.datasets.NeRFSyntheticDataset on a SynLego scene the test writes to disk (12 training views of 64 x 64 RGBA, 2 each
for val / test): the fused sampling kernel (csrc/dataset.hip, wisp_multiview_sample) against the ray generator, against the torch
statement of the reference's colour blend, and against the resident-tensor path (SampleRays over MultiviewTensorDataset) it
replaces - all bit for bit - and the dataset under MultiviewTrainer."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
RES, VIEWS = 64, 12


def _writer():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from train_nerf_synthetic import write_synlego_scene
    finally:
        sys.path.pop(0)
    return write_synlego_scene


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("synlego_rgba"))
    _writer()(root, views=(VIEWS, 2, 2), res=RES, device=DEV, steps=256)
    return root


@pytest.fixture(scope="module")
def dataset(scene):
    from wisp.datasets import NeRFSyntheticDataset
    return NeRFSyntheticDataset(scene, split='train')


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _poses(scene, split='train'):
    import json
    with open(os.path.join(scene, f"transforms_{split}.json")) as f:
        meta = json.load(f)
    return [np.array(fr['transform_matrix']) for fr in meta['frames']], {k: v for k, v in meta.items() if k != 'frames'}


# ------------------------------------------------------------------------------------------------ 5. rays
def test_view_rays_equal_generate_pinhole_rays_bit_for_bit(dataset):
    from wisp.ops.raygen import generate_centered_pixel_coords, generate_pinhole_rays
    assert len(dataset) == VIEWS and tuple(dataset.img_shape) == (RES, RES) and dataset.images.is_cuda
    h, w = dataset.img_shape
    grid = generate_centered_pixel_coords(w, h, w, h, device=DEV)
    for i, (name, cam) in enumerate(dataset.cameras.items()):
        want = generate_pinhole_rays(cam, grid)
        got = dataset.view(i)
        assert _bits_equal(got['rays'].origins, want.origins), name
        assert _bits_equal(got['rays'].dirs, want.dirs), name
        assert got['rays'].dist_min == want.dist_min == 1.0 and got['rays'].dist_max == want.dist_max == 5.0
        assert got['rgb'].shape == (h * w, 3) and got['masks'].shape == (h * w, 1) and got['masks'].dtype == torch.bool
    # a negative pixel index counts from the end, as in wisp_gather_rows
    import wisp._C as C
    kw = dict(view_index=3, camera_host=dataset._records_host[3], x0=dataset._principal[0], y0=dataset._principal[1],
              tan_x=dataset._tan[0], tan_y=dataset._tan[1])
    last = C.multiview_sample(dataset.images, torch.tensor([-1, -h * w], device=DEV), **kw)
    full = dataset.view(3)
    assert _bits_equal(last["origins"], full['rays'].origins[[-1, 0]]) and _bits_equal(last["dirs"], full['rays'].dirs[[-1, 0]])
    assert _bits_equal(last["rgb"], full['rgb'][[-1, 0]]) and _bits_equal(last["mask"], full['masks'][[-1, 0]])
    only = C.multiview_sample(dataset.images, torch.tensor([5], device=DEV), want=("rgb",), view_index=3)       # outputs are optional
    assert list(only) == ["rgb"] and _bits_equal(only["rgb"], full['rgb'][5:6])
    with pytest.raises(RuntimeError):
        C.multiview_sample(dataset.images.cpu(), torch.tensor([0]), **kw)       # no CPU path
    with pytest.raises(RuntimeError):
        C.multiview_sample(dataset.images, torch.tensor([0], device=DEV), **dict(kw, view_index=VIEWS))


# ------------------------------------------------------------------------------------------------ 6. colours and masks
@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.2, 0.5, 0.7)])
def test_colours_and_masks_equal_the_torch_expression_of_the_reference(scene, bg):
    """nerf_standard_dataset.py:432-439 evaluated op by op on the device from the u8 bank (blend_colors_torch; the host suite holds
    that expression to the reference's own method)."""
    from wisp.datasets import NeRFSyntheticDataset
    from wisp.datasets.formats.nerf_standard_dataset import blend_colors_torch
    ds = NeRFSyntheticDataset(scene, split='train', bg_color=bg)
    alpha = ds.images[..., 3]
    assert int(alpha.min()) == 0 and int(alpha.max()) == 255 and int(((alpha > 0) & (alpha < 255)).sum()) > 0     # all three kinds
    for i in range(len(ds)):
        want_rgb, want_mask = blend_colors_torch(ds.images[i].reshape(-1, 4), bg, has_alpha=True)
        got = ds.view(i)
        assert _bits_equal(got['rgb'], want_rgb), i
        assert _bits_equal(got['masks'], want_mask), i
    assert 0 < int(ds.view(0)['masks'].sum()) < RES * RES


def test_rgb_only_files_give_unblended_colours_and_true_masks(scene, tmp_path):
    from wisp.datasets import NeRFSyntheticDataset
    from wisp.datasets.formats.nerf_standard_dataset import u8_to_unit_float
    from wisp.ops.image import load_u8, write_png
    import shutil
    for name in os.listdir(scene):
        if name.endswith(".json"):
            shutil.copy(os.path.join(scene, name), tmp_path / name)
    for split in ("train", "val", "test"):
        os.makedirs(tmp_path / split)
        for name in os.listdir(os.path.join(scene, split)):
            write_png(str(tmp_path / split / name), load_u8(os.path.join(scene, split, name))[..., :3])
    ds = NeRFSyntheticDataset(str(tmp_path), split='train', bg_color=(1.0, 1.0, 1.0))
    assert not ds.has_alpha and ds.device_bytes() == 4 * VIEWS * RES * RES + 64 * VIEWS
    for i in range(len(ds)):
        got = ds.view(i)
        assert _bits_equal(got['rgb'], u8_to_unit_float(ds.images[i].reshape(-1, 4)[:, :3])), i
        assert bool(got['masks'].all())


# ------------------------------------------------------------------------------------------------ 7. mip
def _mip_restatement(bank, mip, bg):
    """numpy float32, one rounding per operation: every texel converted (u8 / 255), the converted texels of a 2^mip x 2^mip block
    summed in row-major order, times 1 / 4^mip, then the blend; the mask tests the averaged alpha."""
    f32 = np.float32
    conv = (np.arange(256, dtype=f32) / f32(255.0))[bank]                      # [V, H, W, 4]
    s = 1 << mip
    acc = None
    for dy in range(s):
        for dx in range(s):
            t = conv[:, dy::s, dx::s]
            acc = t.copy() if acc is None else (acc + t).astype(f32)
    acc = (acc * f32(1.0 / 4 ** mip)).astype(f32)
    a = acc[..., 3:4]
    rgb = np.clip((acc[..., :3] * a).astype(f32) + ((f32(1.0) - a).astype(f32) * np.array(bg, dtype=f32)).astype(f32), f32(0), f32(1))
    V, h, w = acc.shape[:3]
    return rgb.astype(f32).reshape(V, h * w, 3), (a > f32(0.5)).reshape(V, h * w, 1)


@pytest.mark.parametrize("mip", [1, 2])
def test_mip_colours_equal_the_numpy_restatement_and_intrinsics_scale(scene, dataset, mip):
    from wisp.datasets import NeRFSyntheticDataset
    from wisp.ops.raygen import generate_centered_pixel_coords, generate_pinhole_rays
    bg = (0.2, 0.5, 0.7)
    poses, meta = _poses(scene)
    bank = dataset.images.cpu().numpy()
    meta = dict(meta, cx=35.0, cy=30.5)
    ds = NeRFSyntheticDataset.from_arrays(bank, poses, meta, bg_color=bg, mip=mip)
    h, w = RES >> mip, RES >> mip
    assert tuple(ds.img_shape) == (h, w)
    assert ds.x0 == 35.0 / 2 ** mip - w // 2 and ds.y0 == 30.5 / 2 ** mip - h // 2                 # :387-390
    assert ds.focal_x == (0.5 * w) / np.tan(0.5 * float(meta['camera_angle_x'])) and ds.focal_y == ds.focal_x
    assert ds.device_bytes() == 4 * VIEWS * RES * RES + 64 * VIEWS                                   # the bank stays full size
    want_rgb, want_mask = _mip_restatement(bank, mip, bg)
    grid = generate_centered_pixel_coords(w, h, w, h, device=DEV)
    for i, cam in enumerate(ds.cameras.values()):
        got = ds.view(i)
        assert got['rgb'].shape == (h * w, 3)
        assert np.array_equal(got['rgb'].cpu().numpy(), want_rgb[i]), i
        assert np.array_equal(got['masks'].cpu().numpy(), want_mask[i]), i
        want = generate_pinhole_rays(cam, grid)                                                      # principal point off centre
        assert _bits_equal(got['rays'].origins, want.origins) and _bits_equal(got['rays'].dirs, want.dirs)
    for bad in (bank[:, :63], bank[:, :, :63]) + ((bank[:, :62],) if mip == 2 else ()):              # 63 is odd, 62 % 4 != 0
        with pytest.raises(ValueError):
            NeRFSyntheticDataset.from_arrays(bad, poses, meta, mip=mip)


# ------------------------------------------------------------------------------------------------ 8. SampleRays
@pytest.mark.parametrize("n", [1, 4096, RES * RES + 7])
def test_item_with_sample_rays_equals_sample_rays_of_the_whole_view(dataset, n):
    from wisp.datasets import MultiviewBatch, SampleRays
    ds = dataset.create_split('no_such_split', transform=SampleRays(n))        # shallow copy, same bank
    for i in (0, 7, VIEWS - 1):
        torch.manual_seed(100 + i)
        got = ds[i]
        torch.manual_seed(100 + i)
        want = SampleRays(n)(dataset.view(i))
        assert isinstance(got, MultiviewBatch) and got['rays'].origins.shape == (n, 3)
        assert _bits_equal(got['rays'].origins, want['rays'].origins) and _bits_equal(got['rays'].dirs, want['rays'].dirs)
        assert _bits_equal(got['rgb'], want['rgb']) and _bits_equal(got['masks'], want['masks'])
        assert got['rays'].dist_min == want['rays'].dist_min and got['rays'].dist_max == want['rays'].dist_max
    # any other transform, or none, receives the whole view
    whole = dataset.create_split('no_such_split', transform=lambda b: dict(b, seen=True))[2]
    assert whole['seen'] and _bits_equal(whole['rgb'], dataset.view(2)['rgb'])
    assert dataset.transform is None and _bits_equal(dataset[2]['rays'].dirs, dataset.view(2)['rays'].dirs)


# ------------------------------------------------------------------------------------------------ 9. footprint
def test_device_footprint_is_the_u8_bank_and_items_leave_nothing_behind(scene):
    from wisp.datasets import NeRFSyntheticDataset, SampleRays
    n = 4096
    ds = NeRFSyntheticDataset(scene, split='train', transform=SampleRays(n))
    assert ds.device_bytes() == 4 * VIEWS * RES * RES + 64 * VIEWS
    assert ds.images.dtype == torch.uint8 and tuple(ds.images.shape) == (VIEWS, RES, RES, 4)
    assert ds.camera_records.dtype == torch.float32 and tuple(ds.camera_records.shape) == (VIEWS, 16)
    batch = ds[0]
    one_batch = sum(-(-(t.numel() * t.element_size()) // 512) * 512                                  # the allocator's 512-byte blocks
                    for t in (batch['rays'].origins, batch['rays'].dirs, batch['rgb'], batch['masks']))
    del batch
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for k in range(100):
        batch = ds[k % VIEWS]
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    print(f"memory_allocated grew by {grown} bytes over 100 items; one batch is {one_batch} bytes")
    assert grown <= one_batch


# ------------------------------------------------------------------------------------------------ 10. sample()
def test_sample_draws_rays_of_all_views_equal_to_the_resident_layout(dataset):
    n = 20000
    torch.manual_seed(5)
    batch = dataset.sample(n)
    data = dataset.data
    assert data['rays'].origins.shape == (VIEWS, RES * RES, 3) and data['rgb'].shape == (VIEWS, RES * RES, 3)
    assert data['masks'].shape == (VIEWS, RES * RES, 1) and list(data['cameras']) == list(dataset.cameras)
    v, p = batch['view_idx'], batch['pixel_idx']
    assert v.shape == p.shape == (n,) and int(v.min()) == 0 and int(v.max()) == VIEWS - 1 and int(v.unique().numel()) == VIEWS
    assert int(p.min()) >= 0 and int(p.max()) < RES * RES
    assert _bits_equal(batch['rays'].origins, data['rays'].origins[v, p]) and _bits_equal(batch['rays'].dirs, data['rays'].dirs[v, p])
    assert _bits_equal(batch['rgb'], data['rgb'][v, p]) and _bits_equal(batch['masks'], data['masks'][v, p])
    g = torch.Generator(device=DEV).manual_seed(9)
    a = dataset.sample(257, generator=g)
    g.manual_seed(9)
    b = dataset.sample(257, generator=g)
    assert _bits_equal(a['view_idx'], b['view_idx']) and _bits_equal(a['rgb'], b['rgb'])
    pairs = list(dataset.iter_views())
    assert len(pairs) == VIEWS and _bits_equal(pairs[4][0].origins, data['rays'].origins[4]) and _bits_equal(pairs[4][1], data['rgb'][4])
    # `data` is cached, and is counted once it exists
    assert dataset.data is data and dataset.device_bytes() == (4 + 37) * VIEWS * RES * RES + 64 * VIEWS


# ------------------------------------------------------------------------------------------------ 11. end to end
def _pipeline():
    import synlego
    from wisp.accelstructs import OctreeAS
    from wisp.models import Pipeline
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralRadianceField
    from wisp.tracers import PackedRFTracer
    torch.manual_seed(0)
    blas = OctreeAS.from_quantized_points(synlego.occupied_cells(4, device=DEV), 4)
    grid = HashGrid.from_geometric(blas, feature_dim=2, num_lods=8, multiscale_type='cat', feature_std=0.2, codebook_bitwidth=12,
                                   min_grid_res=4, max_grid_res=64)
    nef = NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=64, num_layers=1, bias=True).to(DEV)
    return Pipeline(nef, PackedRFTracer(raymarch_type='ray', num_steps=64, bg_color=(0.0, 0.0, 0.0)))


def _run_trainer(train_dataset, validation_dataset=None, iterations=31):
    """MultiviewTrainer.iterate() `iterations` times from fixed seeds; returns what step() was handed each time, and the running
    loss the trainer's metrics held after each call."""
    from wisp.trainers import ConfigAdamW, ConfigMultiviewTrainer, MultiviewTrainer
    cfg = ConfigMultiviewTrainer(optimizer=ConfigAdamW(lr=1e-3, eps=1e-15, weight_decay=1e-6), grid_lr_weight=100.0, enable_amp=True,
                                 prune_every=-1, rgb_loss_type='huber', rgb_loss_denom='rays', max_epochs=10, scheduler=False)
    trainer = MultiviewTrainer(cfg, _pipeline(), train_dataset, validation_dataset=validation_dataset, device=DEV)
    torch.manual_seed(1)
    handed, losses = [], []
    inner = trainer.step

    def recording_step(data):
        handed.append((data['rays'].origins.clone(), data['rays'].dirs.clone(), data['rgb'].clone()))
        return inner(data)
    trainer.step = recording_step
    trainer.is_optimization_running = True
    for _ in range(iterations):
        trainer.iterate()
        losses.append((trainer.tracker.metrics.total_loss, trainer.tracker.metrics.num_samples))
    torch.cuda.synchronize()
    return trainer, handed, losses


def test_training_on_the_dataset_hands_the_trainer_the_batches_of_the_resident_path(scene, dataset):
    """No threshold: the batches MultiviewTrainer.step receives over 31 iterations (the first only sizes the batch) from the new
    dataset and from a MultiviewTensorDataset built from its `data` must be the same bits - origins, directions, colours, ray
    counts - and so must the loss of the first optimisation step.  Later losses are printed, not asserted: one step's hash-grid
    backward already differs between two runs through its float atomics."""
    from wisp.datasets import MultiviewTensorDataset, NeRFSyntheticDataset, SampleRays
    from wisp.trainers import MultiviewTrainStep
    new = NeRFSyntheticDataset(scene, split='train', transform=SampleRays(512))
    data = dataset.data
    old = MultiviewTensorDataset(data['rays'].origins, data['rays'].dirs, data['rgb'], 1.0, 5.0, transform=SampleRays(512),
                                 img_shape=tuple(dataset.img_shape))
    val = new.create_split('val', transform=None)
    assert len(val) == 2 and val.split == 'val'
    tr_new, handed_new, loss_new = _run_trainer(new, validation_dataset=val)
    tr_old, handed_old, loss_old = _run_trainer(old)
    assert len(handed_new) == len(handed_old) == 31
    for k, (a, b) in enumerate(zip(handed_new, handed_old)):
        assert a[0].shape == b[0].shape, (k, a[0].shape, b[0].shape)                                # ray counts
        assert all(_bits_equal(x, y) for x, y in zip(a, b)), k
    assert handed_new[0][0].shape == (1, 512, 3) and handed_new[5][0].shape[1] != 512                # the adaptive count took over
    assert loss_new[0] == loss_old[0] == (0.0, 0)                                                    # the first call only sized the batch
    first_new, first_old = loss_new[1][0], loss_old[1][0]
    for k in range(1, 31):
        print(f"iteration {k:2d}: running loss  new {loss_new[k][0]:.9g}  resident {loss_old[k][0]:.9g}")
    assert loss_new[1][1] == loss_old[1][1] == 1 and np.isfinite(first_new) and first_new > 0.0
    assert first_new == first_old                                                                    # bitwise: both are Python floats
    out = tr_new.validate()
    print(f"validation psnr after 30 steps: {out['psnr']:.3f}")
    assert np.isfinite(out["psnr"])
    # the fused step consumes sample() batches
    torch.manual_seed(2)
    step = MultiviewTrainStep(_pipeline(), prune_every=-1)
    batch = new.sample(2048)
    loss, num_samples = step.step(batch['rays'], batch['rgb'])
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and num_samples > 0


# ------------------------------------------------------------------------------------------------ 12. loader
def test_load_multiview_dataset_picks_the_class(scene):
    from wisp.datasets import NeRFSyntheticDataset, SampleRays, load_multiview_dataset
    tr = SampleRays(64)
    ds = load_multiview_dataset(scene, split='test', transform=tr, bg_color=(1.0, 1.0, 1.0), mip=1, not_an_option=3)
    assert type(ds) is NeRFSyntheticDataset and len(ds) == 2 and ds.split == 'test' and ds.transform is tr
    assert ds.bg_color == (1.0, 1.0, 1.0) and tuple(ds.img_shape) == (RES // 2, RES // 2) and ds.images.is_cuda
    assert ds[1]['rgb'].shape == (64, 3)
