"""CPU: SSIM without a GPU.
  * tests/ssim_ref.py (the float64 restatement over scipy.ndimage.gaussian_filter that the GPU tests compare the kernel with)
    against an explicit long-double 2-D weighted sum, so that its own error is known: 1e-12 on the map, 1e-13 on the mean;
  * the window weights against scipy's own kernel;
  * wisp_ssim: declared, bound, exported alike; every argument check answers before a launch; the kernel's resources;
  * wisp.ops.image.ssim / structural_similarity refuse host tensors; the trainers refuse 'ssim' on a host device and 'lpips'
    everywhere, before anything is rendered; the scripts' --valid-metrics."""
import ctypes
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch
from scipy import ndimage

import kernel_meta
import ssim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
SHAPES = ((11, 11), (12, 37), (67, 130))


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ref.KINDS)
def test_restatement_agrees_with_a_long_double_direct_sum(kind, shape):
    """measured when this was written: map within 4.3e-13, mean within 5.1e-14 (the near-flat pairs; 3e-15 on the others)"""
    x, y = ref.pair(kind, *shape)
    mean, channel, smap = ref.expected(kind, *shape)
    want_mean, want_channel, want_map = ref.direct(x, y)
    map_err = float(np.abs(smap.astype(np.longdouble) - want_map).max())
    mean_err = float(abs(np.longdouble(mean) - want_mean))
    print(f"{kind} {shape}: map {map_err:.2e} mean {mean_err:.2e}")
    assert smap.dtype == np.float64 and smap.shape == shape + (3,) and channel.shape == (3,)
    assert map_err <= 1e-12 and mean_err <= 1e-13
    # (a channel's score is a mean of map values, so it is as good as the map; at 11 x 11 it is ONE map value)
    assert float(np.abs(channel.astype(np.longdouble) - want_channel).max()) <= 1e-12
    if shape == (11, 11):                                 # one cropped pixel: the mean IS the centre of the map
        assert np.array_equal(channel, smap[5, 5])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identical_images_give_exactly_one(shape):
    mean, channel, smap = ref.expected("identical", *shape)
    assert mean == 1.0 and np.all(channel == 1.0) and np.all(smap == 1.0)


def test_fp32_arithmetic_is_not_enough_on_flat_regions():
    """why the kernel computes in fp64: the same restatement in fp32 is off by about 1e-4 where the variance cancels against C2,
    five orders above the 1e-9 the GPU tests hold the kernel to"""
    x, y = ref.pair("near_flat", 67, 130)
    r, cov_norm, c1, c2 = ref.constants()
    f = lambda a: ndimage.gaussian_filter(a.astype(np.float32), sigma=1.5, truncate=3.5, mode='reflect', output=np.float32)   # noqa: E731
    a, b = x[..., 0], y[..., 0]
    n = np.float32
    got = ref._statistic(f(a), f(b), f(a * a), f(b * b), f(a * b), n(cov_norm), n(c1), n(c2))
    assert got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - ref.expected("near_flat", 67, 130)[2][..., 0]).max())
    print(f"fp32 restatement: {err:.2e}")
    assert err > 1e-6


@pytest.mark.parametrize("sigma,radius", [(1.5, 5), (0.5, 2), (2.0, 7), (4.2, 15)])
def test_window_weights_are_scipys(sigma, radius):
    from wisp.ops.image import gaussian_window
    w = gaussian_window(sigma)
    impulse = np.zeros(4 * radius + 1)
    impulse[2 * radius] = 1.0
    scipys = ndimage.gaussian_filter1d(impulse, sigma, truncate=3.5, mode='constant')[radius:3 * radius + 1]
    assert w.dtype == np.float64 and w.size == 2 * radius + 1 == 2 * ref.radius_of(sigma) + 1
    assert np.array_equal(w, scipys) and np.array_equal(w, w[::-1])
    assert np.count_nonzero(ndimage.gaussian_filter1d(impulse, sigma, truncate=3.5, mode='constant')) == w.size
    assert np.abs(w - ref.weights(sigma)).max() <= 1e-15 and abs(w.sum() - 1.0) <= 1e-15


# ------------------------------------------------------------------------------------------------ entry point and kernel
SSIM_ARGS = ["x", "x_row_stride", "x_pix_stride", "y", "y_row_stride", "y_pix_stride", "H", "W", "C", "radius", "weights", "cov_norm",
             "c1", "c2", "out", "map", "scratch", "scratch_bytes", "stream"]


def test_ssim_entry_point_is_declared_bound_and_exported_alike():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    assert "wisp/ops/image/metrics.py:70-90" in header
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+wisp_ssim\s*\(([^)]*)\)\s*;", header)
    assert m, "wisp_ssim is not declared in include/wisp_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[1].lstrip("*") for a in args] == SSIM_ARGS
    kinds = ["ptr" if ("*" in a or a.startswith("wisp_stream_t")) else {"int64_t": "i64", "int": "i32", "double": "f64"}[a.rsplit(" ", 1)[0]]
             for a in args]
    bound = [{ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int32: "i32", ctypes.c_double: "f64"}[c]
             for c in C.SIGNATURES["wisp_ssim"]]
    assert kinds == bound
    assert re.search(r"\bint64_t\s+wisp_ssim_scratch_bytes\s*\(\s*int H,\s*int W,\s*int C\s*\)\s*;", header)
    assert C.SIGNATURES["wisp_ssim_scratch_bytes"] == [ctypes.c_int32] * 3 and C._RESTYPES["wisp_ssim_scratch_bytes"] is ctypes.c_int64
    raw = ctypes.CDLL(LIB)
    assert hasattr(raw, "wisp_ssim") and hasattr(raw, "wisp_ssim_scratch_bytes")
    assert C.lib.wisp_abi_version() == 4 == C.ABI_VERSION                 # an added entry point does not bump the version
    # one double per channel and 16 x 16 tile
    assert C.lib.wisp_ssim_scratch_bytes(16, 16, 1) == 8 and C.lib.wisp_ssim_scratch_bytes(17, 33, 3) == 8 * 3 * 2 * 3
    assert C.lib.wisp_ssim_scratch_bytes(800, 800, 3) == 8 * 3 * 2500 and C.lib.wisp_ssim_scratch_bytes(0, 5, 3) == 0


def test_ssim_argument_checks_answer_before_any_launch():
    """Every refusal comes back as an error code with a message, on a machine without a GPU: nothing was launched."""
    import wisp._C as C
    fn = C.lib.wisp_ssim
    P = ctypes.c_void_p
    buf = (ctypes.c_uint8 * 256)()
    p = P(ctypes.addressof(buf))                                          # a non-null address; never dereferenced by a refused call
    null = P(0)
    big = 1 << 40

    def call(x=p, xr=64 * 3, xp=3, y=p, yr=64 * 3, yp=3, H=64, W=64, C_=3, radius=5, weights=p, out=p, smap=null, scratch=p,
             scratch_bytes=big):
        return fn(x, xr, xp, y, yr, yp, H, W, C_, radius, weights, 121 / 120, 1e-4, 9e-4, out, smap, scratch, scratch_bytes, null)

    refusals = (
        (dict(x=null), "null pointer"), (dict(y=null), "null pointer"), (dict(weights=null), "null pointer"),
        (dict(out=null), "null pointer"), (dict(scratch=null), "null pointer"),
        (dict(C_=0), "C must be 1..4"), (dict(C_=5), "C must be 1..4"), (dict(C_=-1), "C must be 1..4"),
        (dict(radius=0), "radius must be 1..15"), (dict(radius=16), "radius must be 1..15"), (dict(radius=-3), "radius must be 1..15"),
        (dict(H=10), "smaller than the window"), (dict(W=10), "smaller than the window"), (dict(H=0, W=0), "smaller than the window"),
        (dict(H=30, W=64, radius=15), "smaller than the window"), (dict(H=-5), "smaller than the window"),
        (dict(xp=2), "pixel stride smaller than C"), (dict(yp=0), "pixel stride smaller than C"), (dict(xp=-3), "pixel stride smaller than C"),
        (dict(xr=64 * 3 - 1), "row stride"), (dict(yr=3), "row stride"), (dict(yp=4), "row stride"),
        (dict(xr=2 ** 31 // 64), "below 2^31"), (dict(yr=2 ** 31 // 64), "below 2^31"), (dict(H=2 ** 20, xr=2 ** 11, yr=2 ** 11), "below 2^31"),
        (dict(scratch_bytes=0), "scratch smaller"), (dict(scratch_bytes=8 * 3 * 16 - 1), "scratch smaller"),
    )
    for kw, msg in refusals:
        assert call(**kw) == -1, kw
        assert msg in C.last_error() and C.last_error().startswith("wisp_ssim: "), (kw, C.last_error())


def test_ops_refuse_host_tensors_small_images_and_wide_windows():
    from wisp.ops import image as ops
    import wisp._C as C
    a = torch.rand(16, 16, 3)
    for fn in (ops.ssim, ops.structural_similarity):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            fn(a, a)
        with pytest.raises(RuntimeError, match="GPU tensor"):
            fn(a.numpy(), a.numpy())
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.ssim(a, a, 3, ops.gaussian_window(), 121 / 120, 1e-4, 9e-4)
    assert ops.SSIM_MAX_RADIUS == 15 and ops.gaussian_window().size == 11
    # what is refused by value is refused before a device is needed: 'meta' tensors claim to be on a GPU only in the next test


def test_shape_and_window_errors_are_value_errors(monkeypatch):
    """the ValueErrors of structural_similarity do not depend on a device: tensors whose is_cuda is true are enough"""
    from wisp.ops import image as ops

    class OnGpu(torch.Tensor):
        is_cuda = True
    img = lambda *shape: torch.zeros(*shape).as_subclass(OnGpu)          # noqa: E731
    for a, b, kw, msg in ((img(10, 40, 3), img(10, 40, 3), {}, "smaller than the 11 x 11 window"),
                          (img(40, 10, 3), img(40, 10, 3), {}, "smaller than the 11 x 11 window"),
                          (img(0, 0, 3), img(0, 0, 3), {}, "smaller than"),
                          (img(30, 30, 3), img(30, 30, 3), dict(sigma=4.2), "smaller than the 31 x 31 window"),
                          (img(64, 64, 3), img(64, 64, 3), dict(sigma=4.5), "radius of 16"),
                          (img(64, 64, 3), img(64, 64, 3), dict(sigma=0.1), "radius of 0"),
                          (img(64, 64, 3), img(64, 65, 3), {}, "one size"),
                          (img(64, 64, 3), img(64, 64, 4), {}, "channels"),
                          (img(64, 64, 5), img(64, 64, 5), {}, "channels must be 1..4"),
                          (img(64, 64, 2), img(64, 64, 2), dict(channels=3), "channels must be 1..4"),
                          (img(64, 64), img(64, 64, 1), {}, "one size")):
        with pytest.raises(ValueError, match=msg):
            ops.structural_similarity(a, b, **kw)


@pytest.mark.skipif(not kernel_meta.available(LIB), reason="library or llvm-readelf missing")
def test_ssim_kernel_resources():
    """No scratch memory in any of the three kernels.  LDS of the tile kernel, for its largest radius R (5 in the instance compiled
    for the reference's window, 15 in the general one): both images' halo of a 16 x 16 tile as floats, 16 + 2 R rows of 48 (padded
    so that two rows in one LDS lane group share no bank); the five row sums of every halo row as doubles; the 2 R + 1 weights as
    doubles.  26712 and 47352 bytes: under the 64 KB the kernel may use.  The sum kernel: one double per thread."""
    meta = {n: v for n, v in kernel_meta.kernels(LIB).items() if "ssim" in n}
    names = kernel_meta.demangled(list(meta))
    by = {names[n].split("(")[0].replace("void ", ""): v for n, v in meta.items()}
    assert sorted(by) == ["ssim_sum_kernel", "ssim_tile_kernel<0>", "ssim_tile_kernel<5>"], sorted(by)
    tile, halo_stride = 16, 48
    for name, radius in (("ssim_tile_kernel<5>", 5), ("ssim_tile_kernel<0>", 15)):
        k, halo = by[name], tile + 2 * radius
        assert k["scratch"] == 0 and k["wg"] == tile * tile == 256
        assert k["lds"] == 2 * halo * halo_stride * 4 + 5 * halo * tile * 8 + (2 * radius + 1) * 8 <= 64 * 1024
        assert k["vgpr"] + k["agpr"] <= 128                              # (no spill, and LDS - not registers - bounds the occupancy)
    assert by["ssim_tile_kernel<5>"]["lds"] == 26712 and by["ssim_tile_kernel<0>"]["lds"] == 47352
    assert by["ssim_sum_kernel"]["scratch"] == 0 and by["ssim_sum_kernel"]["lds"] == 256 * 8 and by["ssim_sum_kernel"]["wg"] == 256


def test_kernel_source_states_the_formula_once():
    """one __device__ statement of the per-pixel formula, used by the mean and the map alike; no floating-point atomics"""
    src = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "ssim.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert len(re.findall(r"\bssim_pixel\s*\(", code)) == 2               # the definition and ONE call
    assert code.count("c2)) /") == 1
    assert "atomicAdd" not in code and "unsafeAtomicAdd" not in code
    assert "ssim.hip" in open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "Makefile")).read()


# ------------------------------------------------------------------------------------------------ trainers
def _multiview_stub(device, valid_metrics):
    seen = []

    class Visualizer:
        def render(self, *a, **k):
            seen.append(a)
            raise AssertionError("rendered")
    ds = types.SimpleNamespace(img_shape=torch.Size([16, 16]), data=dict(rays=None, rgb=torch.zeros(1, 256, 3)))
    me = types.SimpleNamespace(tracker=types.SimpleNamespace(log_dir="unused", visualizer=Visualizer()),
                               cfg=types.SimpleNamespace(valid_metrics=tuple(valid_metrics), save_valid_imgs=False),
                               validation_dataset=ds, pipeline=types.SimpleNamespace(tracer=object()), epoch=1, max_epochs=1,
                               return_dict={}, device=device)
    return me, ds, seen


@pytest.mark.parametrize("device,metric", [("cpu", "ssim"), (torch.device("cpu"), "ssim"), ("cpu", "lpips"), ("cuda", "lpips"),
                                           ("cuda:0", "lpips")])
def test_trainers_refuse_what_they_cannot_compute_before_rendering(device, metric):
    from wisp.trainers import ImageTrainer, MultiviewTrainer
    me, ds, seen = _multiview_stub(device, ("psnr", metric))
    with pytest.raises(NotImplementedError, match=metric):
        MultiviewTrainer.evaluate_metrics(me, ds, None)
    assert seen == [] and me.return_dict == {}
    me = types.SimpleNamespace(cfg=types.SimpleNamespace(valid_metrics=("psnr", metric)), device=device)   # (nothing else is reached)
    with pytest.raises(NotImplementedError, match=metric):
        ImageTrainer.validate(me)


def test_multiview_validate_routes_extra_metrics_through_evaluate_metrics():
    """validate(): 'psnr' alone keeps its fast path; anything more goes view by view through evaluate_metrics"""
    from wisp.trainers import MultiviewTrainer
    calls = []
    nef = types.SimpleNamespace(grid=types.SimpleNamespace(num_lods=4))
    pipeline = types.SimpleNamespace(nef=nef, eval=lambda: calls.append("eval"), train=lambda: calls.append("train"))
    me = types.SimpleNamespace(validation_dataset=object(), cfg=types.SimpleNamespace(valid_metrics=("psnr", "ssim"), save_valid_imgs=False),
                               pipeline=pipeline, return_dict={"psnr": 1.0, "ssim": 0.5},
                               evaluate_metrics=lambda ds, lod, name=None: calls.append((lod, name)))
    assert MultiviewTrainer.validate(me) == {"psnr": 1.0, "ssim": 0.5}
    assert calls == ["eval", (3, "lod3"), "train"]


# ------------------------------------------------------------------------------------------------ scripts
def _script(name):
    spec = importlib.util.spec_from_file_location("script_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name,positional", [("train_image", ["some.png"]), ("train_nerf_synthetic", ["some_dir"])])
def test_scripts_take_valid_metrics(name, positional, capsys):
    ap = _script(name).build_parser()
    assert ap.parse_args(positional).valid_metrics == ["psnr"]
    assert ap.parse_args(positional + ["--valid-metrics", "psnr", "ssim"]).valid_metrics == ["psnr", "ssim"]
    with pytest.raises(SystemExit):
        ap.parse_args(positional + ["--valid-metrics", "lpips"])
    capsys.readouterr()


def test_image_script_config_carries_the_metrics():
    mod = _script("train_image")
    assert mod.trainer_config(1).valid_metrics == ("psnr",)
    assert mod.trainer_config(1, valid_metrics=["psnr", "ssim"]).valid_metrics == ("psnr", "ssim")
