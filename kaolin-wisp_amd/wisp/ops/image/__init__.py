"""Image metrics of the validation loop (wisp/ops/image/metrics.py:19-37, 70-90)."""
import functools

import numpy as np
import torch


def psnr(rgb, gts):
    """10 log10(1 / mse) for images in [0,1], shapes [..., 3]."""
    assert (rgb.max() <= 1.05 and rgb.min() >= -0.05)
    assert (gts.max() <= 1.05 and gts.min() >= -0.05)
    assert (rgb.shape[-1] == 3) and (gts.shape[-1] == 3)
    mse = torch.mean((rgb[..., :3] - gts[..., :3]) ** 2).item()
    return 10 * np.log10(1.0 / mse)


SSIM_MAX_RADIUS = 15                    # csrc/ssim.hip stages the halo of a 16 x 16 tile for windows up to 31 x 31


@functools.lru_cache(maxsize=16)
def gaussian_window(sigma=1.5, truncate=3.5):
    """The 1-D weights of scipy.ndimage.gaussian_filter1d, in float64: radius = int(truncate * sigma + 0.5),
    w[i] = exp(-0.5 (i / sigma)^2) for i = -radius..radius, divided by their sum.  (Cached, hence read-only.)"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    w = w / w.sum()
    w.setflags(write=False)
    return w


def structural_similarity(a, b, *, sigma=1.5, truncate=3.5, data_range=1.0, K1=0.01, K2=0.03, use_sample_covariance=True,
                          full=False, channels=None):
    """Mean structural similarity of two [H, W, C] images on the GPU (C = `channels` leading channels, all of them by default,
    at most 4; an [H, W] image is one channel) under the Gaussian window scikit-image's
    structural_similarity(gaussian_weights=True, channel_axis=-1) uses: 2 r + 1 taps with r = int(truncate * sigma + 0.5),
    boundary mode 'reflect', the mean over the image cropped by r, the mean over channels.  use_sample_covariance keeps that
    function's NP / (NP - 1) factor, NP = (2 r + 1)^2.  fp16 / bf16 images are upcast to fp32; all arithmetic on the pixels is fp64,
    in two launches (csrc/ssim.hip: 16 x 16 tiles, then their sum in a fixed order).
    Returns a 0-d float64 tensor on the images' device - nothing is read back, so callers can accumulate over views - and with
    full=True also the float64 map [H, W, C] (its border sees the reflected pixels; the mean does not).
    ValueError: an image smaller than the window, a radius outside 1..15, shapes that do not match."""
    import wisp._C as _C
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"wisp HIP op: `{name}` must be a GPU tensor (the hot path has no CPU fallback); got "
                               f"{type(t).__name__} on {getattr(t, 'device', None)}")
    if a.dim() == 2 and b.dim() == 2:
        a, b = a[..., None], b[..., None]
    if a.dim() != 3 or b.dim() != 3 or tuple(a.shape[:2]) != tuple(b.shape[:2]):
        raise ValueError(f"structural_similarity: needs two [H, W, C] images of one size, got {tuple(a.shape)} / {tuple(b.shape)}")
    if channels is None:
        if a.shape[2] != b.shape[2]:
            raise ValueError(f"structural_similarity: {a.shape[2]} and {b.shape[2]} channels; say how many to compare with channels=")
        channels = a.shape[2]
    channels = int(channels)
    if not 1 <= channels <= 4 or min(a.shape[2], b.shape[2]) < channels:
        raise ValueError(f"structural_similarity: channels must be 1..4 and present in both images, got {channels}")
    weights = gaussian_window(sigma, truncate)
    radius = (weights.size - 1) // 2
    if not 1 <= radius <= SSIM_MAX_RADIUS:
        raise ValueError(f"structural_similarity: sigma {sigma} and truncate {truncate} give a window radius of {radius}; "
                         f"1..{SSIM_MAX_RADIUS} is served")
    if a.shape[0] < weights.size or a.shape[1] < weights.size:
        raise ValueError(f"structural_similarity: a {a.shape[0]} x {a.shape[1]} image is smaller than the "
                         f"{weights.size} x {weights.size} window")
    num = weights.size ** 2
    cov_norm = num / (num - 1.0) if use_sample_covariance else 1.0
    c1, c2 = (K1 * float(data_range)) ** 2, (K2 * float(data_range)) ** 2
    out, smap = _C.ssim(a, b, channels, weights, cov_norm, c1, c2, want_map=bool(full))
    return (out[channels], smap) if full else out[channels]


def ssim(rgb, gts):
    """The reference's SSIM of two images in [0,1], shapes [H, W, >= 3] (the first three channels count): what its call of
    skimage.metrics.structural_similarity(data_range=1, gaussian_weights=True, sigma=1.5, channel_axis=-1) defines, computed on
    the GPU.  Returns a Python float, as the reference does (one read-back)."""
    for name, t in (("rgb", rgb), ("gts", gts)):         # (before the range asserts: those would run on the host)
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"wisp HIP op: `{name}` must be a GPU tensor (the hot path has no CPU fallback); got "
                               f"{type(t).__name__} on {getattr(t, 'device', None)}")
    assert (rgb.max() <= 1.05 and rgb.min() >= -0.05)
    assert (gts.max() <= 1.05 and gts.min() >= -0.05)
    return float(structural_similarity(rgb, gts, channels=3))


from .io import load_rgb, load_u8, save_u8, read_png, write_png          # noqa: E402
