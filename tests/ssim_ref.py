"""Test infrastructure: the structural similarity that wisp.ops.image.ssim computes, restated in float64 on the host.

It is the definition that the reference's call selects (wisp/ops/image/metrics.py:84-90:
skimage.metrics.structural_similarity(data_range=1, gaussian_weights=True, sigma=1.5, channel_axis=-1)), written out over
scipy.ndimage.gaussian_filter - scikit-image itself is not a dependency and is not compared against.  `direct` is the same
quantity as an explicit 2-D weighted sum in long double over np.pad(mode='symmetric'): the yardstick of the restatement's own
error (tests/test_ssim_host.py).  Plain data and helpers, no GPU."""
import functools

import numpy as np
from scipy import ndimage

TRUNCATE = 3.5


def radius_of(sigma, truncate=TRUNCATE):
    return int(truncate * sigma + 0.5)


def weights(sigma, truncate=TRUNCATE):
    """1-D weights: exp(-0.5 (i / sigma)^2), i = -r..r, over their sum, in double"""
    r = radius_of(sigma, truncate)
    i = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * (i / sigma) ** 2)
    return w / w.sum()


def constants(sigma=1.5, truncate=TRUNCATE, data_range=1.0, K1=0.01, K2=0.03, use_sample_covariance=True):
    r = radius_of(sigma, truncate)
    num = (2 * r + 1) ** 2
    cov_norm = num / (num - 1.0) if use_sample_covariance else 1.0
    return r, cov_norm, (K1 * data_range) ** 2, (K2 * data_range) ** 2


def _statistic(ux, uy, uxx, uyy, uxy, cov_norm, c1, c2):
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def _finish(maps, r):
    """[H, W, C] map -> (mean over channels of the cropped means, channel means, map)"""
    smap = np.stack(maps, axis=-1)
    h, w = smap.shape[:2]
    channel = np.array([m[r:h - r, r:w - r].mean(dtype=m.dtype) for m in maps])
    return channel.mean(), channel, smap


def ssim(x, y, sigma=1.5, truncate=TRUNCATE, **kw):
    """x, y: [H, W, C] arrays (fp32 images; computed in float64) -> (mean, channel means [C], map [H, W, C]), all float64"""
    r, cov_norm, c1, c2 = constants(sigma, truncate, **kw)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape[0] < 2 * r + 1 or x.shape[1] < 2 * r + 1:
        raise ValueError("image smaller than the window")
    f = functools.partial(ndimage.gaussian_filter, sigma=sigma, truncate=truncate, mode='reflect')
    maps = []
    for c in range(x.shape[2]):
        a, b = x[..., c], y[..., c]
        maps.append(_statistic(f(a), f(b), f(a * a), f(b * b), f(a * b), cov_norm, c1, c2))
    return _finish(maps, r)


def direct(x, y, sigma=1.5, truncate=TRUNCATE, **kw):
    """the same in long double, every window an explicit 2-D weighted sum over the symmetric padding"""
    r, cov_norm, c1, c2 = constants(sigma, truncate, **kw)
    L = np.longdouble
    i = np.arange(-r, r + 1).astype(L)
    w = np.exp(L(-0.5) * (i / L(sigma)) ** 2)
    w = w / w.sum()
    w2 = np.outer(w, w)
    x, y = np.asarray(x).astype(L), np.asarray(y).astype(L)
    h, wd = x.shape[:2]

    def f(img):
        p = np.pad(img, r, mode='symmetric')
        out = np.zeros((h, wd), dtype=L)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                out += w2[dy, dx] * p[dy:dy + h, dx:dx + wd]
        return out
    maps = []
    for c in range(x.shape[2]):
        a, b = x[..., c], y[..., c]
        maps.append(_statistic(f(a), f(b), f(a * a), f(b * b), f(a * b), L(cov_norm), L(c1), L(c2)))
    return _finish(maps, r)


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("random", "near_flat", "identical")


@functools.lru_cache(maxsize=None)
def pair(kind, h, w, c=3, seed=0):
    """two fp32 [h, w, c] images in [0, 1]: independent noise; 0.7 + 1e-3 * noise (where uxx - ux ux cancels against C2, the
    case fp32 arithmetic gets wrong by 1e-4); one random image twice"""
    rng = np.random.default_rng([seed, h, w, c, KINDS.index(kind)])
    if kind == "random":
        a, b = rng.uniform(size=(h, w, c)), rng.uniform(size=(h, w, c))
    elif kind == "near_flat":
        a, b = 0.7 + 1e-3 * rng.normal(size=(h, w, c)), 0.7 + 1e-3 * rng.normal(size=(h, w, c))
    else:
        a = rng.uniform(size=(h, w, c))
        b = a
    a, b = a.astype(np.float32), b.astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def expected(kind, h, w, c=3, seed=0, sigma=1.5, data_range=1.0, use_sample_covariance=True):
    """the restatement of pair(...), computed once and shared"""
    out = ssim(*pair(kind, h, w, c, seed), sigma=sigma, data_range=data_range, use_sample_covariance=use_sample_covariance)
    out[1].setflags(write=False)
    out[2].setflags(write=False)
    return out
