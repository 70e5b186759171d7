"""A float64 restatement of the radiance-field query over a triplanar grid (test infrastructure; the subject is
csrc/nerf_triplane_query.hip), put together from two existing pieces that are imported as they are: the triplanar encoder of
tests/triplane_sdf_eval_ref.py (fp32 source coordinates of wisp_reflect_source_index, everything behind them in float64; its
generator of exactly representable positions) and the decoder of tests/nerf_octree_query_ref.py (NeuralRadianceField.rgba after the
lookup, wisp/models/nefs/nerf.py:245-264).  Host only.

A field here is a NeuralRadianceField over a TriplanarGrid; `planes_of` turns its grid into the encoder reference's dict (planes
[F, R, R]: x, y, z of level 0, then level 1, ...; multiscale)."""
import numpy as np
import torch

import triplane_sdf_eval_ref as tri
from nerf_octree_query_ref import decoder64, decoder_params, view_code64          # noqa: F401 (view_code64: re-exported)
from triplane_sdf_eval_ref import exact_points, generic_points, source_index      # noqa: F401 (re-exported for the tests)


def planes_of(grid, lod_idx=None):
    """the encoder reference's field dict for levels 0..lod_idx of a TriplanarGrid ('cat' takes them all)"""
    num = grid.num_lods if lod_idx is None else lod_idx + 1
    planes = []
    for i in range(num):
        v = grid.features[i]
        for p in (v.fmx, v.fmy, v.fmz):
            planes.append(p.detach().float().cpu().reshape(p.shape[-3], p.shape[-2], p.shape[-1]))
    return dict(planes=planes, multiscale=grid.multiscale_type)


def features64(nef, coords, lod_idx=None):
    """float64 [n, K]: what TriplanarGrid.interpolate(coords, lod_idx) returns, from the fp32 source coordinates"""
    return tri.features(planes_of(nef.grid, lod_idx), torch.as_tensor(coords).detach().float().cpu()).numpy()


def field64(nef, coords, dirs=None, lod_idx=None):
    """(rgb [n,3] or None, density [n,1]) in float64, on the CPU"""
    d = None if dirs is None else torch.as_tensor(dirs).detach().cpu().numpy()
    return decoder64(decoder_params(nef), features64(nef, coords, lod_idx), d)


def exact_bits(sizes, b=1):
    """fraction bits of the quantum of exact_points(b=b) on planes of these sizes"""
    return tri._bits(b, sizes)


def exact_planes(F, sizes, seed):
    """3 per size, integers in [-1, 1], f32 [F, R, R]"""
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(-1, 2, size=(F, R, R)).astype(np.float32)) for R in sizes for _ in range(3)]


def check_exact_features(fld, coords, bits):
    """the feature half of triplane_sdf_eval_ref.check_exact for the query of `fld` (planes, multiscale) at `coords`: on every level
    the fp32 source coordinate IS the exact one, every blend factor lies on the grid of 2^-(bits / 2), the planes hold -1 / 0 / 1,
    every feature is a multiple of q = 2^-bits and every level sum stays below 2^24 quanta - so a float32 evaluation in any order
    equals the float64 one bit for bit.  A failure here blames the inputs, not the kernel."""
    q = 2.0 ** -bits
    c = coords.float().numpy()
    for l in range(tri.num_lods(fld)):
        R = int(fld["planes"][3 * l].shape[-1])
        assert R == 1 or (R - 1) & (R - 2) == 0, "the span is no power of two: the reflection is not exact"
        ix = tri.source_index(c, R)
        assert np.array_equal(ix.astype(np.float64), tri.exact_source_index(c.astype(np.float64), R)), \
            "a source coordinate is not exact in fp32"
        t = (ix - np.floor(ix)).astype(np.float64)
        assert np.array_equal(np.round(t / 2.0 ** -(bits // 2)) * 2.0 ** -(bits // 2), t), "a blend factor is off the quantum grid"
    for p in fld["planes"]:
        assert bool(torch.equal(torch.round(p), p)) and float(p.abs().max()) <= 1.0, "a plane holds more than -1 / 0 / 1"
    x = tri.features(fld, coords)
    assert bool(torch.equal(torch.round(x / q) * q, x)), "a feature is off the quantum grid"
    lev = tri.level_features(fld, coords).abs().sum(1)
    assert float(lev.max()) / q < 2.0 ** 24, "level sum: the partial sums leave fp32"


# the exact cases of tests/test_gpu_nerf_triplane_query.py (and of the host file, which checks that they are exact):
# name -> (features per plane, multiscale, log2 of the first span, levels); planes of 5 / 9 / 17 / 33 texels a side
EXACT_CASES = {"f4_sum4": (4, 'sum', 2, 4), "f1_sum1": (1, 'sum', 5, 1), "f10_sum2": (10, 'sum', 2, 2), "f5_cat2": (5, 'cat', 4, 2),
               "f4_cat2": (4, 'cat', 3, 2)}
COUNTS = (1, 63, 65, 700)                 # a partial tile, a tile boundary, more than one workgroup of 4 x 64


def exact_case_inputs(name, n):
    """(planes, sizes, coords, bits) of one exact case at one sample count; the planes depend on the name alone"""
    F, multiscale, base, lods = EXACT_CASES[name]
    sizes = [2 ** (base + i) + 1 for i in range(lods)]
    planes = exact_planes(F, sizes, seed=sum(map(ord, name)))
    return planes, sizes, exact_points(n, b=1, seed=40 + n), exact_bits(sizes, b=1)
