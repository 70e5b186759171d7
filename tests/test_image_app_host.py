"""CPU: the host side of the image application - wisp.datasets.ImageDataset and wisp.ops.geometric.normalized_grid against the
reference's own class and function executed in place, ImageTrainer against the reference's step / log_console bodies, validate()
through the chunked fallback, and the header / binding agreement of the two new entry points.  Tests that need the reference tree
are skipped where it is not mounted; datasets are built with device='cpu'."""
import logging
import os
import re
import types

import numpy as np
import pytest
import torch

import image_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not image_ref.have_reference(), reason="reference tree not mounted")


# ------------------------------------------------------------------------------------------------ 1. dataset
@needs_ref
@pytest.mark.parametrize("size", [(37, 23), (64, 64), (1, 5), (5, 1), (801, 3)])
def test_image_dataset_equals_the_reference_class_bit_for_bit(tmp_path, size):
    from wisp.datasets import ImageDataset
    h, w = size
    img = image_ref.seeded_image(h, w, seed=h * 1000 + w)
    path = str(tmp_path / "img.png")
    image_ref.write_png(path, img)
    ref = image_ref.reference_image_dataset_class()(path, num_pixels_per_image=17)
    ds = ImageDataset(path, num_pixels_per_image=17, device='cpu')
    assert (ds.h, ds.w, len(ds), ds.root, ds.num_pixels_per_image) == (ref.h, ref.w, len(ref), ref.root, 17) and len(ds) == 100
    for name, got, want in (("coords", ds.coords, ref.coords), ("pixels", ds.pixels, ref.pixels), ("image", ds.get_image(), ref.get_image())):
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert torch.equal(got, want), name
    assert np.array_equal(ds.image_u8.numpy(), img)
    c, p = ds[0]
    assert c.shape == (17, 2) and p.shape == (17, 3)
    idx = torch.tensor([0, h * w - 1, (h * w) // 2])
    c, p = ds.sample(idx)
    assert torch.equal(c, ref.coords[idx]) and torch.equal(p, ref.pixels[idx])
    tc, tp = image_ref.torch_sample(torch.from_numpy(img), idx)             # the restatement the GPU tests hold the kernel to
    assert torch.equal(tc, ref.coords[idx]) and torch.equal(tp, ref.pixels[idx])


@needs_ref
@pytest.mark.parametrize("channels", [1, 4])
def test_image_dataset_raises_the_reference_exception_for_other_channel_counts(tmp_path, channels):
    from wisp.datasets import ImageDataset
    img = image_ref.seeded_image(6, 7, seed=3, channels=channels)
    path = str(tmp_path / "img.png")
    image_ref.write_png(path, img[..., 0] if channels == 1 else img)
    with pytest.raises(Exception) as want:
        image_ref.reference_image_dataset_class()(path)
    with pytest.raises(Exception) as got:
        ImageDataset(path, device='cpu')
    assert str(got.value) == str(want.value) and type(got.value) is type(want.value) is Exception


@needs_ref
def test_committed_fixture_is_the_reference_output(tmp_path, golden_dir):
    fix = np.load(os.path.join(golden_dir, "image_dataset_ref.npz"))
    h, w = image_ref.GOLDEN_SIZE
    img = image_ref.seeded_image(h, w, image_ref.GOLDEN_SEED)
    assert np.array_equal(fix["image"], img)
    path = str(tmp_path / "img.png")
    image_ref.write_png(path, img)
    ref = image_ref.reference_image_dataset_class()(path)
    assert np.array_equal(fix["coords"], ref.coords.numpy()) and np.array_equal(fix["pixels"], ref.pixels.numpy())


def test_image_dataset_equals_the_committed_fixture(tmp_path, golden_dir):
    from wisp.datasets import ImageDataset
    fix = np.load(os.path.join(golden_dir, "image_dataset_ref.npz"))
    path = str(tmp_path / "img.png")
    image_ref.write_png(path, fix["image"])
    ds = ImageDataset(path, device='cpu')
    assert np.array_equal(ds.coords.numpy(), fix["coords"]) and np.array_equal(ds.pixels.numpy(), fix["pixels"])
    assert fix["coords"].dtype == np.float32 and fix["pixels"].dtype == np.float32


# ------------------------------------------------------------------------------------------------ 2. normalized_grid
@needs_ref
@pytest.mark.parametrize("use_aspect", [False, True])
@pytest.mark.parametrize("size", [(37, 23), (23, 37), (64, 64), (1, 5), (5, 1), (480, 640)])
def test_normalized_grid_equals_the_reference_function(size, use_aspect):
    from wisp.ops.geometric import normalized_grid
    ref = image_ref.reference_normalized_grid()
    got = normalized_grid(size[0], size[1], device='cpu', use_aspect=use_aspect)
    want = ref(size[0], size[1], device='cpu', use_aspect=use_aspect)
    assert got.shape == (size[0], size[1], 2) and torch.equal(got, want)
    torch.manual_seed(4)
    a = normalized_grid(size[0], size[1], jitter=True, device='cpu', use_aspect=use_aspect)
    torch.manual_seed(4)
    b = ref(size[0], size[1], jitter=True, device='cpu', use_aspect=use_aspect)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. trainer
class _Field(torch.nn.Module):
    """CPU stand-in for ImageNeuralField: 'grid' and 'decoder' parameter names, rgb(coords) -> [n, 3] in (0, 1)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(8)
        self.grid = torch.nn.Module()
        self.grid.feats = torch.nn.Parameter(torch.randn(16, 16, 4) * 0.1)
        self.decoder = torch.nn.Linear(4 + 2, 3)

    def rgb(self, coords, lod=None):
        cell = ((coords * 0.5 + 0.5) * 15).long().clamp(0, 15)
        return torch.sigmoid(self.decoder(torch.cat([self.grid.feats[cell[:, 1], cell[:, 0]], coords], -1)))


class _Pipe(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.nef = _Field()


class _TorchForReference:
    """`torch` for the reference's method bodies on a CPU box: torch.cuda.amp.autocast() a no-op context, the rest forwarded"""

    def __init__(self):
        import contextlib
        self.cuda = types.SimpleNamespace(amp=types.SimpleNamespace(autocast=lambda *a, **k: contextlib.nullcontext()),
                                          nvtx=types.SimpleNamespace(range=lambda *a, **k: contextlib.nullcontext()))

    def __getattr__(self, name):
        return getattr(torch, name)


def _dataset(tmp_path, h=24, w=32):
    from wisp.datasets import ImageDataset
    path = str(tmp_path / "train.png")
    image_ref.write_png(path, image_ref.procedural_image(h, w))
    return ImageDataset(path, num_pixels_per_image=64, device='cpu')


def _cfg(**kw):
    from wisp.trainers import ConfigAdam, ConfigBaseTrainer
    base = dict(optimizer=ConfigAdam(lr=1e-2, eps=1e-16, weight_decay=1e-6), grid_lr_weight=5.0, max_epochs=2, enable_amp=False,
                scheduler=True, valid_every=-1, profile_nvtx=False)
    base.update(kw)
    return ConfigBaseTrainer(**base)


@needs_ref
def test_image_trainer_step_and_log_line_equal_the_reference_methods(tmp_path, caplog):
    import torch.nn.functional as F
    from wisp.trainers import ImageTrainer
    ds = _dataset(tmp_path)
    tr = ImageTrainer(_cfg(), _Pipe(), ds, device='cpu')
    tr.pre_training()
    assert tr.tracker.metrics.rgb_loss == 0.0

    pipe_r = _Pipe()
    named = dict(pipe_r.nef.named_parameters())
    opt = torch.optim.Adam([dict(params=[p for n, p in named.items() if 'decoder' in n], lr=1e-2, eps=1e-16, weight_decay=1e-6),
                            dict(params=[p for n, p in named.items() if 'decoder' not in n], lr=5e-2, eps=1e-16)],
                           lr=1e-2, eps=1e-16, weight_decay=1e-6)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[200 * x for x in (0.5, 0.75, 0.9)], gamma=0.333)
    metrics = types.SimpleNamespace(total_loss=0.0, rgb_loss=0.0, num_samples=0)
    metrics.average_metric = lambda name: getattr(metrics, name) / max(metrics.num_samples, 1)
    me = types.SimpleNamespace(pipeline=pipe_r, device='cpu', optimizer=opt, scheduler=sched, scaler=None, epoch=1, max_epochs=2,
                               cfg=types.SimpleNamespace(enable_amp=False, scheduler=True), tracker=types.SimpleNamespace(metrics=metrics))
    glb = dict(torch=_TorchForReference(), F=F, log=logging)
    ref_step = image_ref.reference_trainer_method("step", glb)
    ref_log = image_ref.reference_trainer_method("log_console", glb)
    g = torch.Generator().manual_seed(2)
    for _ in range(5):
        idx = torch.randint(0, ds.h * ds.w, (64,), generator=g)
        c, p = ds.sample(idx)
        batch = [c[None], p[None]]
        before_r, before_m = metrics.total_loss, tr.tracker.metrics.total_loss
        ref_step(me, batch)
        tr.step(batch)
        assert metrics.total_loss - before_r == tr.tracker.metrics.total_loss - before_m          # the same loss, bit for bit
    assert metrics.rgb_loss == tr.tracker.metrics.rgb_loss
    for (n1, p1), (n2, p2) in zip(pipe_r.nef.named_parameters(), tr.pipeline.nef.named_parameters()):
        assert torch.equal(p1, p2), n1
    with pytest.raises(AssertionError):
        tr.step([torch.zeros(2, 4, 2), torch.zeros(2, 4, 3)])                   # a batch dimension other than 1
    with caplog.at_level(logging.INFO):
        caplog.clear()
        ref_log(me)
        want = caplog.records[-1].getMessage()
        tr.log_console()
        got = caplog.records[-1].getMessage()
    assert got == want and re.fullmatch(r"EPOCH 1/2 \| total loss: \d\.\d{3}E[+-]\d\d \| rgb loss: \d\.\d{3}E[+-]\d\d", got)


def test_image_trainer_runs_its_life_cycle_over_tuple_batches(tmp_path):
    from wisp.trainers import ImageTrainer
    ds = _dataset(tmp_path)
    tracker_dir = str(tmp_path / "logs")
    from wisp.trainers.base_trainer import _Tracker
    tr = ImageTrainer(_cfg(max_epochs=2, valid_every=2), _Pipe(), ds, tracker=_Tracker(tracker_dir), device='cpu')
    assert tr.iterations_per_epoch == 100
    batch = next(iter(tr.train_data_loader))
    assert isinstance(batch, list) and batch[0].shape == (1, 64, 2) and batch[1].shape == (1, 64, 3)
    out = tr.train()
    assert tr.epoch == 2 and 'psnr' in out and os.path.exists(os.path.join(tracker_dir, "img_pred.png"))


# ------------------------------------------------------------------------------------------------ 4. validate
def test_validate_on_the_fallback_path_writes_the_reference_images_and_psnr(tmp_path):
    from wisp.models.nefs import render_image
    from wisp.ops.image import load_u8
    from wisp.trainers import ImageTrainer
    from wisp.trainers.base_trainer import _Tracker
    ds = _dataset(tmp_path, h=19, w=27)
    log_dir = str(tmp_path / "run")
    tr = ImageTrainer(_cfg(), _Pipe(), ds, tracker=_Tracker(log_dir), device='cpu')
    nef = tr.pipeline.nef
    tr.validate()
    with torch.no_grad():
        img = nef.rgb(ds.coords).reshape(ds.h, ds.w, 3)                         # what image_trainer.py:113-119 computes
    gts = ds.pixels.reshape(ds.h, ds.w, 3)
    assert np.array_equal(load_u8(os.path.join(log_dir, "img_pred.png")), (img * 255).byte().numpy())
    assert np.array_equal(load_u8(os.path.join(log_dir, "img_gts.png")), (gts * 255).byte().numpy())
    assert np.array_equal(load_u8(os.path.join(log_dir, "img_gts.png")), ds.image_u8.numpy())
    psnr = image_ref.reference_psnr() if image_ref.have_reference() else __import__("wisp.ops.image", fromlist=["psnr"]).psnr
    first = psnr(img, gts)
    assert tr.return_dict['psnr'] == first
    # the max rule of image_trainer.py:153-157: a worse field later does not lower the record, a better one raises it
    with torch.no_grad():
        nef.decoder.bias += 3.0
    tr.validate()
    assert tr.return_dict['psnr'] == first
    # render_image's pieces, ranges and u8 form on the host
    whole = render_image(nef, ds.h, ds.w)
    parts = torch.cat([render_image(nef, ds.h, ds.w, first=0, count=100, chunk=33), render_image(nef, ds.h, ds.w, first=100)])
    assert torch.equal(whole, parts)
    u8, err = render_image(nef, ds.h, ds.w, out='u8', gts_u8=ds.image_u8)
    assert torch.equal(u8, (whole * 255).byte()) and err.dtype == torch.float64
    want = ((whole - ds.pixels) ** 2).double().sum()
    assert abs(float(err) - float(want)) <= 1e-12 * float(want)
    for metric in ('ssim', 'lpips'):
        tr.cfg.valid_metrics = ('psnr', metric)
        with pytest.raises(NotImplementedError, match=metric):
            tr.validate()


def test_image_train_step_schedule_follows_multistep_lr():
    """ImageTrainStep.set_schedule against torch's MultiStepLR (host arithmetic only: no optimizer launch)."""
    from wisp.trainers.image_trainer import ImageTrainStep
    step = ImageTrainStep.__new__(ImageTrainStep)
    step.lr, step.opt_steps = 1e-3, 0
    step.set_schedule([5.0, 7.5, 9.0], 0.333)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[5.0, 7.5, 9.0], gamma=0.333)
    for _ in range(12):
        opt.step(); sched.step()
        step.opt_steps += 1
        step.lr = step.scheduled_lr()
        assert abs(step.lr - opt.param_groups[0]['lr']) <= 1e-12


# ------------------------------------------------------------------------------------------------ 5. ABI
def test_header_and_binding_agree_on_the_image_entry_points():
    import ctypes
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    kinds = {"ptr": ctypes.c_void_p, "i64": ctypes.c_int64, "i32": ctypes.c_int32, "f32": ctypes.c_float}
    for name, ret in (("wisp_image_sample", "int"), ("wisp_image_field_render", "int"), ("wisp_image_field_render_partials", "int64_t")):
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", bare)
        assert m, name
        want = []
        for arg in (a.strip() for a in m.group(1).split(",")):
            base = " ".join(arg.split()).rsplit(" ", 1)[0].replace("const ", "")
            want.append(kinds["ptr"] if ("*" in arg or arg.startswith("wisp_stream_t")) else kinds[{"int64_t": "i64", "int": "i32", "float": "f32"}[base]])
        assert C.SIGNATURES[name] == want, name
        assert hasattr(C._cdll, name)
    assert C._cdll.wisp_image_field_render_partials.restype is ctypes.c_int64
    assert C.lib.wisp_image_field_render_partials(0) == 0 and C.lib.wisp_image_field_render_partials(257) == 2
    assert C.ABI_VERSION == 4 and "wisp_image_field_render" in header and "fmaf(step, i, start)" in header
    with pytest.raises(RuntimeError):
        C.image_sample(torch.zeros(2, 2, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))      # no CPU fallback in the binding
