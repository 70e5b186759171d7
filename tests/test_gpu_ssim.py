"""GPU: wisp_ssim (csrc/ssim.hip), wisp.ops.image.ssim / structural_similarity, and SSIM in the trainers' validation.

The kernel is held to the float64 restatement of tests/ssim_ref.py (itself within 1e-12 / 1e-13 of a long-double direct sum,
tests/test_ssim_host.py) within 1e-9, on the mean and on every element of the map.  The bound is derived, not measured: a
121-tap fp64 sum errs by at most about 1.3e-14 relative, and the cancellation uxx - ux ux against C2 = 9e-4 amplifies that by at
most 1 / C2 = 1.1e3; 1e-9 leaves four orders of margin and lies five orders below the 1e-4 of an fp32 implementation.
Shapes: 11 x 11 (one cropped pixel, every tap in the halo), 12 x 37, 17 x 17 (the 16 x 16 tile plus one pixel in each axis),
67 x 130, and 263 x 258 (289 tiles: the sum kernel takes more than one round of its 256 threads).
Measured on an MI355X (profiles/ssim_test_margins.jsonl): see SSIM_MEASURED below."""
import json
import logging
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import ssim_ref as ref
from gpu_helpers import DEV, cuda, margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9
TILE = 16
SHAPES = ((11, 11), (12, 37), (TILE + 1, TILE + 1), (67, 130), (263, 258))
SSIM_MEASURED = "mean within 1.5e-13 (near flat, 11 x 11), map within 8.1e-13 (sigma 2, near flat) of the restatement; argument swap 0"


def _C():
    import wisp._C as C
    return C


def _ops():
    from wisp.ops import image as ops
    return ops


def _check(name, got_mean, got_map, want):
    mean, channel, smap = want
    assert got_mean.dtype == torch.float64 and got_mean.dim() == 0 and got_mean.is_cuda
    assert got_map.dtype == torch.float64 and tuple(got_map.shape) == smap.shape
    margin(f"ssim mean {name}", abs(float(got_mean) - float(mean)), BOUND)
    margin(f"ssim map {name}", float(np.abs(got_map.cpu().numpy() - smap).max()), BOUND)


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ref.KINDS)
def test_mean_and_map_match_the_float64_restatement(kind, shape):
    x, y = ref.pair(kind, *shape)
    got_mean, got_map = _ops().structural_similarity(cuda(x), cuda(y), full=True)
    _check(f"{kind} {shape}", got_mean, got_map, ref.expected(kind, *shape))
    if kind == "identical":
        assert float(got_mean) == 1.0 and bool((got_map == 1.0).all())
    else:
        back_mean, back_map = _ops().structural_similarity(cuda(y), cuda(x), full=True)
        margin(f"ssim swap {kind} {shape}", max(abs(float(back_mean) - float(got_mean)), float((back_map - got_map).abs().max())), 1e-12)
    assert abs(float(_ops().structural_similarity(cuda(x), cuda(y))) - float(got_mean)) == 0.0      # (without the map: the same mean)


@pytest.mark.parametrize("case", ["sigma0.5", "sigma2", "radius15", "population_covariance", "data_range2"])
def test_parameters(case):
    shape, kw = {"sigma0.5": ((12, 37), dict(sigma=0.5)), "sigma2": ((67, 130), dict(sigma=2.0)), "radius15": ((31, 31), dict(sigma=4.2)),
                 "population_covariance": ((12, 37), dict(use_sample_covariance=False)), "data_range2": ((12, 37), dict(data_range=2.0))}[case]
    assert {"sigma0.5": 2, "sigma2": 7, "radius15": 15}.get(case, 5) == ref.radius_of(kw.get("sigma", 1.5))
    for kind in ("random", "near_flat"):
        x, y = ref.pair(kind, *shape)
        got_mean, got_map = _ops().structural_similarity(cuda(x), cuda(y), full=True, **kw)
        want = ref.ssim(x, y, **kw)
        _check(f"{case} {kind}", got_mean, got_map, want)
        if case in ("population_covariance", "data_range2"):               # the parameter reaches the kernel: not the default's value
            assert abs(float(got_mean) - float(ref.expected(kind, *shape)[0])) > 1e-6


@pytest.mark.parametrize("channels", [1, 4])
def test_one_and_four_channels(channels):
    x, y = ref.pair("near_flat", 12, 37, channels)
    got_mean, got_map = _ops().structural_similarity(cuda(x), cuda(y), full=True)
    want = ref.expected("near_flat", 12, 37, channels)
    _check(f"{channels} channels", got_mean, got_map, want)
    C = _C()
    out, _ = C.ssim(cuda(x), cuda(y), channels, _ops().gaussian_window(), 121 / 120, 1e-4, 9e-4)
    assert out.shape == (channels + 1,) and float(np.abs(out[:channels].cpu().numpy() - want[1]).max()) <= BOUND
    if channels == 1:
        flat_mean = _ops().structural_similarity(cuda(x)[..., 0], cuda(y)[..., 0])       # [H, W] is one channel
        assert float(flat_mean) == float(got_mean)
    else:
        first3 = _ops().structural_similarity(cuda(x), cuda(y), channels=3)
        assert abs(float(first3) - float(want[1][:3].mean())) <= BOUND


# ------------------------------------------------------------------------------------------------ layout
def test_strided_views_go_in_without_a_copy_and_change_nothing():
    C, ops = _C(), _ops()
    h, w = 67, 130
    x, y = (cuda(a) for a in ref.pair("random", h, w))
    base_mean, base_map = ops.structural_similarity(x, y, full=True)
    rgba = torch.rand(h, w, 4, device=DEV)
    rgba[..., :3] = x
    padded = torch.rand(h, w + 5, 3, device=DEV)
    padded[:, 2:w + 2] = y
    planar = x.permute(2, 0, 1).contiguous().permute(1, 2, 0)             # channel stride h * w: not addressable, copied
    views = dict(rgba=rgba[..., :3], padded=padded[:, 2:w + 2], planar=planar)
    assert C._ssim_view(views["rgba"], 3, "a").data_ptr() == rgba.data_ptr() and C._ssim_view(views["rgba"], 3, "a").stride() == (4 * w, 4, 1)
    assert C._ssim_view(views["padded"], 3, "a").data_ptr() == padded[:, 2:].data_ptr()
    assert C._ssim_view(views["planar"], 3, "a").is_contiguous() and C._ssim_view(x, 3, "a") is x
    for name, (a, b) in dict(rgba=(views["rgba"], y), padded=(x, views["padded"]), both=(views["rgba"], views["padded"]),
                             planar=(views["planar"], y), four_of_four=(rgba, torch.cat([y, y[..., :1]], -1))).items():
        mean, smap = ops.structural_similarity(a, b, full=True, channels=3)
        assert torch.equal(mean, base_mean) and torch.equal(smap, base_map), name
    assert ops.ssim(rgba, views["padded"]) == float(base_mean)            # ssim(): the first three channels


@pytest.mark.parametrize("shape,channels,with_map", [((17, 17), 3, True), ((67, 130), 4, True), ((12, 37), 1, False)])
def test_every_output_element_is_written_and_nothing_beyond(shape, channels, with_map):
    """out, the map and the scratch sit inside NaN-filled buffers with guard bands on both sides"""
    C = _C()
    h, w = shape
    x, y = (cuda(a) for a in ref.pair("random", h, w, channels))
    guard = 512
    need = int(C.lib.wisp_ssim_scratch_bytes(h, w, channels))
    tiles = -(-h // TILE) * -(-w // TILE)
    assert need == 8 * channels * tiles
    sizes = dict(out=channels + 1, map=h * w * channels, scratch=need // 8)
    bufs = {k: torch.full((guard + n + guard,), float("nan"), dtype=torch.float64, device=DEV) for k, n in sizes.items()}
    inner = {k: b[guard:guard + sizes[k]] for k, b in bufs.items()}
    weights = np.ascontiguousarray(_ops().gaussian_window())
    rc = C.lib.wisp_ssim(C._p(x), x.stride(0), x.stride(1), C._p(y), y.stride(0), y.stride(1), h, w, channels, 5,
                         weights.ctypes.data_as(C.c_vp), 121 / 120, 1e-4, 9e-4, C._p(inner["out"]),
                         C._p(inner["map"]) if with_map else None, C._p(inner["scratch"]), need, C._stream())
    assert rc == 0, C.last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool(torch.isnan(b[:guard]).all()) and bool(torch.isnan(b[guard + sizes[k]:]).all()), k
    want = ref.expected("random", h, w, channels)
    assert bool(torch.isfinite(inner["out"]).all()) and abs(float(inner["out"][channels]) - float(want[0])) <= BOUND
    if with_map:
        assert bool(torch.isfinite(inner["map"]).all())
        assert float(np.abs(inner["map"].reshape(h, w, channels).cpu().numpy() - want[2]).max()) <= BOUND
    else:
        assert bool(torch.isnan(inner["map"]).all())
    # the scratch: one finite sum per channel and tile
    sums = inner["scratch"].reshape(channels, tiles)
    assert bool(torch.isfinite(sums).all())
    count = (h - 10) * (w - 10)
    assert float((sums.sum(1) / count - inner["out"][:channels]).abs().max()) <= 1e-12


def test_three_runs_give_the_same_bits():
    x, y = (cuda(a) for a in ref.pair("near_flat", 263, 258))
    runs = [_ops().structural_similarity(x, y, full=True) for _ in range(3)]
    C = _C()
    outs = [C.ssim(x, y, 3, _ops().gaussian_window(), 121 / 120, 1e-4, 9e-4)[0] for _ in range(3)]
    for mean, smap in runs[1:]:
        assert torch.equal(mean.view(torch.int64), runs[0][0].view(torch.int64)) and torch.equal(smap.view(torch.int64), runs[0][1].view(torch.int64))
    for out in outs:
        assert torch.equal(out.view(torch.int64), outs[0].view(torch.int64)) and torch.equal(out[3], runs[0][0])


# ------------------------------------------------------------------------------------------------ conventions
def test_ssim_follows_the_reference_conventions():
    ops = _ops()
    x, y = (cuda(a) for a in ref.pair("random", 67, 130))
    got = ops.ssim(x, y)
    assert type(got) is float and abs(got - float(ref.expected("random", 67, 130)[0])) <= BOUND
    assert got == float(ops.structural_similarity(x, y, channels=3))
    for bad in (x + 0.2, x - 0.2):                                        # the reference's range asserts, on either argument
        with pytest.raises(AssertionError):
            ops.ssim(bad, y)
        with pytest.raises(AssertionError):
            ops.ssim(y, bad)
    for dtype in (torch.float16, torch.bfloat16):                          # upcast, not computed in half
        assert ops.ssim(x.to(dtype), y.to(dtype)) == ops.ssim(x.to(dtype).float(), y.to(dtype).float())
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        ops.ssim(x[:10], y[:10])
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        ops.structural_similarity(x[:, :10], y[:, :10])
    with pytest.raises(ValueError, match="radius of 16"):
        ops.structural_similarity(x, y, sigma=4.5)
    with pytest.raises(ValueError, match="one size"):
        ops.structural_similarity(x, y[:-1])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.ssim(x, y.cpu())


# ------------------------------------------------------------------------------------------------ MultiviewTrainer
class _Tracer:
    pass


def _multiview_stub(tmp_path, valid_metrics, views=3, h=13, w=17):
    from wisp.core import Rays, RenderBuffer
    g = torch.Generator().manual_seed(3)
    buffers = [RenderBuffer(rgb=torch.rand(h * w, 3, generator=g).to(DEV), depth=(torch.rand(h * w, 1, generator=g) * 4).to(DEV),
                            alpha=torch.rand(h * w, 1, generator=g).to(DEV), hit=(torch.rand(h * w, 1, generator=g) > 0.5).to(DEV))
               for _ in range(views)]

    class Visualizer:
        calls = 0

        def render(self, pipeline, rays, lod_idx=None):
            self.calls += 1
            return buffers[(self.calls - 1) % views]
    rays = Rays(torch.rand(views, h * w, 3, generator=g), torch.rand(views, h * w, 3, generator=g), dist_min=0.5, dist_max=6.0)
    ds = types.SimpleNamespace(img_shape=torch.Size([h, w]), data=dict(rays=rays, rgb=torch.rand(views, h * w, 3, generator=g)))
    me = types.SimpleNamespace(tracker=types.SimpleNamespace(log_dir=str(tmp_path), visualizer=Visualizer()),
                               cfg=types.SimpleNamespace(valid_metrics=tuple(valid_metrics), save_valid_imgs=False),
                               validation_dataset=ds, pipeline=types.SimpleNamespace(tracer=_Tracer()), epoch=7, max_epochs=50,
                               return_dict={}, device=DEV)
    return me, ds, buffers


def test_evaluate_metrics_computes_ssim_per_view(tmp_path, caplog):
    from wisp.ops.image import ssim
    from wisp.trainers import MultiviewTrainer
    h, w = 13, 17
    me, ds, buffers = _multiview_stub(tmp_path, ("psnr", "ssim"))
    with caplog.at_level(logging.INFO):
        out = MultiviewTrainer.evaluate_metrics(me, ds, 2, name="lod2")
    per_view = [ssim(rb.rgb.reshape(h, w, 3), ds.data["rgb"][k].reshape(h, w, 3).to(DEV)) for k, rb in enumerate(buffers)]
    assert list(out) == ["psnr", "ssim"] and out["ssim"] == sum(per_view) / 3
    want = np.mean([ref.ssim(rb.rgb.reshape(h, w, 3).cpu().numpy(), ds.data["rgb"][k].reshape(h, w, 3).numpy())[0]
                    for k, rb in enumerate(buffers)])
    assert abs(out["ssim"] - want) <= BOUND and abs(out["ssim"]) < 1.0
    line = [r.getMessage() for r in caplog.records if r.getMessage().startswith("EPOCH")][-1]
    assert line == "EPOCH 7/50 | lod2 psnr: %.2f | lod2 ssim: %.6f" % (out["psnr"], out["ssim"]), line
    assert me.return_dict == out and not os.path.exists(tmp_path / "val")
    # the max rule over two calls: a better record stays, a worse one is replaced
    me.return_dict["ssim"] = 2.0
    me.return_dict["psnr"] = 0.0
    again = MultiviewTrainer.evaluate_metrics(me, ds, 2, name="lod2")
    assert again == out and me.return_dict == {"psnr": out["psnr"], "ssim": 2.0}
    # PSNR is what a ('psnr',) run gives
    alone, ds1, _ = _multiview_stub(tmp_path, ("psnr",))
    assert MultiviewTrainer.evaluate_metrics(alone, ds1, 2, name="lod2") == {"psnr": out["psnr"]}


# ------------------------------------------------------------------------------------------------ ImageTrainer and its script
def test_image_trainer_validate_adds_ssim_and_changes_nothing_else(tmp_path):
    import image_ref
    from wisp.datasets import ImageDataset
    from wisp.models import Pipeline
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import ImageNeuralField
    from wisp.models.nefs.image_nef import fused_render_shape, render_image
    from wisp.trainers import ConfigAdam, ConfigBaseTrainer, ImageTrainer
    from wisp.trainers.base_trainer import _Tracker
    h, w = 40, 52
    path = str(tmp_path / "train.png")
    image_ref.write_png(path, image_ref.procedural_image(h, w))
    ds = ImageDataset(path, num_pixels_per_image=64, device=DEV)
    torch.manual_seed(0)
    grid = HashGrid.from_geometric(None, feature_dim=2, num_lods=16, multiscale_type='cat', feature_std=0.3, codebook_bitwidth=12,
                                   min_grid_res=16, max_grid_res=64)
    nef = ImageNeuralField(grid, hidden_dim=64, num_layers=1).to(DEV)
    assert fused_render_shape(nef) is not None
    results, files = {}, {}
    for metrics in (("psnr",), ("psnr", "ssim")):
        cfg = ConfigBaseTrainer(optimizer=ConfigAdam(lr=1e-2, eps=1e-16, weight_decay=1e-6), grid_lr_weight=5.0, max_epochs=2,
                                enable_amp=False, scheduler=True, valid_every=-1, profile_nvtx=False, valid_metrics=metrics)
        log_dir = str(tmp_path / "-".join(metrics))
        tr = ImageTrainer(cfg, Pipeline(nef=nef), ds, tracker=_Tracker(log_dir), device=DEV)
        results[metrics] = tr.validate()
        assert tr.return_dict == results[metrics]
        files[metrics] = [open(os.path.join(log_dir, n), "rb").read() for n in ("img_pred.png", "img_gts.png")]
    with_ssim, without = results[("psnr", "ssim")], results[("psnr",)]
    assert list(without) == ["psnr"] and list(with_ssim) == ["psnr", "ssim"] and with_ssim["psnr"] == without["psnr"]
    assert files[("psnr", "ssim")] == files[("psnr",)]
    img = render_image(nef, h, w, out='f32').reshape(h, w, 3)
    gts = ds.image_u8.to(DEV).reshape(h, w, 3) / 255.0
    want = ref.ssim(img.cpu().numpy(), gts.cpu().numpy())[0]
    assert type(with_ssim["ssim"]) is float and abs(with_ssim["ssim"] - float(want)) <= BOUND and abs(with_ssim["ssim"]) < 1.0


def test_train_image_script_reports_ssim(tmp_path):
    img_path, log_dir = str(tmp_path / "test.png"), str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_image.py"), "--write-test-image", img_path, "--size", "128", "128",
           "--epochs", "2", "--log-dir", log_dir, "--valid-metrics", "psnr", "ssim"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    print(rec)
    assert 0.0 < rec["ssim"] <= 1.0 and np.isfinite(rec["psnr"])
    assert re.search(r"^ssim: \d\.\d\d$", run.stderr, flags=re.M), run.stderr[-2000:]
