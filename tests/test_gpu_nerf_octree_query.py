"""GPU: the fused field query of the octree family (csrc/nerf_octree_query.hip, wisp.ops.nerf_mlp.fused_nerf_octree_query) and what is
built on it - PackedRFTracer's `fused_query` attribute on OctreeGrid / CodebookOctreeGrid fields, MultiviewTrainer.evaluate_metrics,
scripts/render_nerf.py --grid - against the modular path (the octree query's chain, the multi-level trilinear lookup, the exact-fp32
decoder, index_select of the ray directions).  The contract is equality of bits: torch.equal on rgb and density and on every channel
of a traced RenderBuffer.  One case cannot be held to bits: a codebook grid's 'sum' over three or more levels, which the modular
path adds with torch.sum in torch's own order; there the fused result's error against a float64 restatement
(tests/nerf_octree_query_ref.py) must not exceed twice the modular path's own error against it."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nerf_octree_query_ref as ref
from gpu_helpers import DEV, cuda, make_rays, margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "WISP_NERF_OCTREE_QUERY_FUSED"

COUNTS = (1, 63, 65, 700)                 # a partial tile, a tile boundary, more than one workgroup of 4 x 64
# tree -> (octree level, LODs); feature shape -> (feature_dim, multiscale)
TREES = {"dense2": (2, 2), "chain4": (4, 4), "sparse4": (4, 4)}
FEATURES = {"f5_sum": (5, 'sum'), "f1_sum": (1, 'sum'), "f16_sum": (16, 'sum'), "f5_cat": (5, 'cat'), "f8_cat": (8, 'cat')}
CHAIN_CELL = (11, 3, 6)                   # the one occupied level-4 cell of the one-child-per-node tree


def make_blas(tree):
    from wisp.accelstructs import OctreeAS
    level = TREES[tree][0]
    if tree == "dense2":
        return OctreeAS.make_dense(level)
    if tree == "chain4":
        cells = np.array([CHAIN_CELL])
    else:
        cells = np.random.default_rng(4).integers(0, 2 ** level, size=(150, 3))
    return OctreeAS.from_quantized_points(torch.from_numpy(cells).short().to(DEV), level)


def make_nef(tree, feature_dim, multiscale, bias=True, hidden=64, codebook=False, seed=0, std=0.5):
    from wisp.models.grids import CodebookOctreeGrid, OctreeGrid
    from wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(seed)
    level, lods = TREES[tree]
    blas = make_blas(tree)
    shape = dict(feature_dim=feature_dim, num_lods=lods, interpolation_type='linear', multiscale_type=multiscale, feature_std=std)
    grid = CodebookOctreeGrid(blas, codebook_bitwidth=4, **shape) if codebook else OctreeGrid(blas, **shape)
    nef = NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=hidden, num_layers=1, bias=bias,
                              prune_density_decay=None, prune_min_density=None).to(DEV)
    with torch.no_grad():
        for n, p in nef.named_parameters():
            if 'decoder' in n:
                p.mul_(2.0)            # wider activations so relu masks and the sigmoid are exercised
        if not bias:
            nef.decoder_density.lout.weight[0].abs_()          # (without the output bias most density logits are negative)
    nef.eval()
    return nef


@functools.lru_cache(maxsize=None)
def field(tree, feats, bias=True):
    """one octree field per shape for the whole file; tests that change a table's dtype put the fp32 values back"""
    return make_nef(tree, *FEATURES[feats], bias=bias)


@functools.lru_cache(maxsize=None)
def codebook_field(tree, multiscale, ties=False):
    nef = make_nef(tree, 5, multiscale, bias=False, codebook=True, seed=3)
    if ties:
        plant_ties(nef.grid)
    return nef


def plant_ties(grid):
    """every third logits row gets its maximum at two or three entries; the dictionary rows differ, so the first-index rule shows"""
    with torch.no_grad():
        for f in grid.features:
            rows = torch.arange(0, f.shape[0], 3, device=f.device)
            top = f[rows].max(dim=1).values + 1.0
            f[rows, 9] = top
            f[rows, 2] = top
            f[rows[::2], 13] = top[::2]


@functools.lru_cache(maxsize=None)
def positions(tree, n, seed):
    """n positions: uniform in the cube, most of them replaced - as far as n allows - by points in occupied cells, and the special
    ones: outside the cube, exactly on cell faces, at -1 and +1.  Also returns unit view directions."""
    level = TREES[tree][0]
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(n, 3, generator=g) * 2.0 - 1.0
    if tree != "dense2":
        # half of the points into occupied cells of the finest level (a sparse tree leaves most of the cube empty)
        cells = np.array([CHAIN_CELL]) if tree == "chain4" else np.random.default_rng(4).integers(0, 2 ** level, size=(150, 3))
        pick = torch.from_numpy(cells[np.random.default_rng(seed).integers(0, len(cells), size=n)]).float()
        inside = (pick + torch.rand(n, 3, generator=g)) / 2 ** (level - 1) - 1.0
        half = torch.rand(n, generator=g) < 0.6
        c[half] = inside[half]
    res = 2 ** level
    cx, cy, cz = (v % res for v in CHAIN_CELL)
    special = torch.tensor([[2.0 * cx / res - 1.0, 2.0 * (cy + 0.5) / res - 1.0, 2.0 * (cz + 0.25) / res - 1.0],   # on a cell face
                            [1.3, -0.7, 0.2], [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [-2.0, 0.0, 5.0],
                            [2.0 * (cx + 1) / res - 1.0, 2.0 * (cy + 1) / res - 1.0, 2.0 * cz / res - 1.0],      # on three faces
                            [0.0, 0.0, 0.0], [1.0, -1.0, 0.25], [0.5, -0.5, 0.25], [float("nan"), 0.0, 0.0],
                            # the sibling of CHAIN_CELL: occupied down to the level above, empty below (one-child-per-node tree)
                            [2.0 * ((cx ^ 1) + 0.5) / res - 1.0, 2.0 * (cy + 0.5) / res - 1.0, 2.0 * (cz + 0.5) / res - 1.0]])
    k = min(n, special.shape[0])
    if n > 1:
        idx = torch.randperm(n, generator=g)[:k]
        c[idx] = special[:k]
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    return c.to(DEV), d.to(DEV)


def modular(nef, coords, dirs, lod_idx=None):
    """lookup + decoder as the modular path launches them"""
    from wisp.ops.nerf_mlp import fused_nerf_decoder
    if lod_idx is None:
        lod_idx = len(nef.grid.active_lods) - 1
    with torch.no_grad():
        feats = nef.grid.interpolate(coords, lod_idx).reshape(coords.shape[0], nef.effective_feature_dim())
        assert feats.dtype == torch.float32
        return fused_nerf_decoder(nef, feats, dirs)


@pytest.fixture
def count_native(monkeypatch):
    """counts the launches of the fused octree query"""
    import wisp._C as C
    calls = []
    inner = C.nerf_octree_query

    def spy(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)
    monkeypatch.setattr(C, "nerf_octree_query", spy)
    monkeypatch.setenv(SWITCH, "1")                             # the switch's default is off
    return calls


# ------------------------------------------------------------------------------------------------ the positions themselves
@pytest.mark.parametrize("tree", list(TREES))
def test_positions_hold_every_kind(tree):
    """on the CPU, with the oracle's query: points outside the cube, on cell faces, at -1 / +1, in occupied cells and (sparse trees)
    in unoccupied ones are all among the 700"""
    nef = field(tree, "f5_sum")
    level = TREES[tree][0]
    c = positions(tree, 700, 100 + 700)[0].cpu().numpy()
    t = ref.tree_of(nef.grid)
    leaf = ref.chain_of(t, c, level)[:, level]
    in_cube = np.all(np.abs(c) <= 1.0, axis=1)
    assert (~in_cube).sum() >= 3 and np.isnan(c).any()
    assert (leaf[~in_cube] == -1).all() and (leaf[in_cube] >= 0).sum() > 100
    cellpos = (0.5 * c[in_cube] + 0.5) * 2 ** level
    assert (cellpos == np.round(cellpos)).any(axis=1).sum() >= 4                       # exactly on a cell face
    assert (np.abs(c[in_cube]) == 1.0).all(axis=1).sum() >= 2                          # corners of the cube
    if tree != "dense2":
        assert (leaf[in_cube] == -1).sum() > 50                                        # unoccupied cells
        mid = ref.chain_of(t, c, level)[:, level - 2]
        assert ((mid >= 0) & (leaf == -1)).any()                                       # occupied above, empty below


# ------------------------------------------------------------------------------------------------ the query
def _lods(nef):
    L = nef.grid.num_lods
    return [L - 1] if nef.grid.multiscale_type == 'cat' else sorted({0, L // 2, L - 1})


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("feats", list(FEATURES))
@pytest.mark.parametrize("tree", list(TREES))
def test_query_equals_lookup_plus_decoder(tree, feats, bias, count_native):
    """every sample count, tables in f32 / f16 / bf16, half_features on and off, lod_idx 0 / middle / last: both outputs, bit for bit"""
    from wisp.ops.nerf_mlp import fused_nerf_octree_query, nerf_octree_query_supported, nerf_query_supported
    nef = field(tree, feats, bias)
    grid = nef.grid
    master = [f.data.clone() for f in grid.features]
    with torch.no_grad():
        assert nerf_octree_query_supported(nef) and not nerf_query_supported(nef)
    assert nef.effective_feature_dim() == {"f5_sum": 5, "f1_sum": 1, "f16_sum": 16, "f5_cat": 5 * grid.num_lods,
                                           "f8_cat": 8 * grid.num_lods}[feats]
    nonzero = 0
    try:
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            for f, m in zip(grid.features, master):
                f.data = m.to(dtype)
            for half in (True, False):
                grid.half_features = half
                for n in COUNTS:
                    coords, dirs = positions(tree, n, 100 + n)
                    for lod_idx in _lods(nef):
                        want_rgb, want_den = modular(nef, coords, dirs, lod_idx)
                        before = len(count_native)
                        with torch.no_grad():
                            rgb, den = fused_nerf_octree_query(nef, coords, ray_d=dirs, lod_idx=lod_idx)
                        assert len(count_native) == before + 1
                        assert rgb.shape == (n, 3) and den.shape == (n, 1) and rgb.dtype == den.dtype == torch.float32
                        case = (tree, feats, bias, dtype, half, n, lod_idx)
                        assert torch.equal(den, want_den), case + ("density",)
                        assert torch.equal(rgb, want_rgb), case + ("rgb",)
                        nonzero += int((den > 0).sum())
        assert nonzero > 0 and float(rgb.std()) > 0.0
    finally:
        grid.half_features = True
        for f, m in zip(grid.features, master):
            f.data = m


# ------------------------------------------------------------------------------------------------ codebook grids
def _err(got, want64):
    return np.abs(got.detach().cpu().double().numpy() - want64)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("tree", ["chain4", "sparse4"])
def test_codebook_bit_for_bit_where_the_sum_has_no_order(tree, ties, count_native):
    """'cat' at the last LOD, 'sum' at lod_idx 0 and 1 against the modular path; and - every lod_idx - against the same kernel called
    on an OctreeGrid whose tables are the decoded rows"""
    from wisp.models.grids import OctreeGrid
    from wisp.ops.nerf_mlp import fused_nerf_octree_query, nerf_octree_query_supported, nerf_query_supported
    import wisp._C as C
    for multiscale in ('cat', 'sum'):
        nef = codebook_field(tree, multiscale, ties)
        grid = nef.grid
        assert not grid.training and nerf_octree_query_supported(nef) and not nerf_query_supported(nef)
        if ties:
            # the first-index rule, checked on the decoded rows themselves: a tied row selects its FIRST maximum's vector
            f, d = grid.features[0].detach(), grid.dictionary[0].detach()
            tied = (f == f.max(dim=1, keepdim=True).values).sum(1) >= 2
            assert int(tied.sum()) >= f.shape[0] // 3 and not torch.equal(d[2], d[9]) and not torch.equal(d[2], d[13])
            rows = C.codebook_decode_rows(f, d, False)
            assert torch.equal(rows[tied], d[2].expand(int(tied.sum()), -1))
        twin = OctreeGrid(grid.blas, feature_dim=5, num_lods=grid.num_lods, multiscale_type=multiscale, feature_std=0.0).to(DEV)
        twin.half_features = False
        for i in range(grid.num_lods):
            twin.features[i].data = C.codebook_decode_rows(grid.features[i].detach(), grid.dictionary[i].detach(), False)
        exact = [grid.num_lods - 1] if multiscale == 'cat' else [0, 1]
        every = [grid.num_lods - 1] if multiscale == 'cat' else list(range(grid.num_lods))
        for n in COUNTS:
            coords, dirs = positions(tree, n, 400 + n)
            for lod_idx in every:
                with torch.no_grad():
                    rgb, den = fused_nerf_octree_query(nef, coords, ray_d=dirs, lod_idx=lod_idx)
                    nef.grid = twin
                    try:
                        rgb_t, den_t = fused_nerf_octree_query(nef, coords, ray_d=dirs, lod_idx=lod_idx)
                    finally:
                        nef.grid = grid
                assert torch.equal(rgb, rgb_t) and torch.equal(den, den_t), (tree, multiscale, n, lod_idx, "decoded twin")
                if lod_idx in exact:
                    want_rgb, want_den = modular(nef, coords, dirs, lod_idx)
                    assert torch.equal(den, want_den) and torch.equal(rgb, want_rgb), (tree, multiscale, n, lod_idx)
        assert len(count_native) > 0


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("tree", ["chain4", "sparse4"])
def test_codebook_sum_of_three_and_four_levels_within_twice_the_modular_error(tree, ties):
    """the modular path adds the levels with torch.sum; per output, the fused query's error against the float64 reference is at most
    twice the modular path's own (both are float32 evaluations of the same expression in different orders)"""
    from wisp.ops.nerf_mlp import fused_nerf_octree_query
    nef = codebook_field(tree, 'sum', ties)
    coords, dirs = positions(tree, 700, 500)
    ok = ~torch.isnan(coords).any(dim=1)                    # (the reference has no opinion on NaN positions)
    coords, dirs = coords[ok], dirs[ok]
    for lod_idx in (2, 3):
        want_rgb, want_den = ref.field64(nef, coords, dirs, lod_idx)
        mod_rgb, mod_den = modular(nef, coords, dirs, lod_idx)
        with torch.no_grad():
            rgb, den = fused_nerf_octree_query(nef, coords, ray_d=dirs, lod_idx=lod_idx)
        for name, got, mod, want in (("rgb", rgb, mod_rgb, want_rgb), ("density", den, mod_den, want_den)):
            e_f, e_m = float(_err(got, want).max()), float(_err(mod, want).max())
            assert e_m > 0.0
            margin(f"nerf_octree_query codebook sum {lod_idx + 1} levels {tree} ties={ties} {name}: fused error vs twice the modular "
                   f"error", e_f, 2.0 * e_m)


# ------------------------------------------------------------------------------------------------ density alone, directions
@pytest.mark.parametrize("which", [("sparse4", "f5_sum", True), ("chain4", "f8_cat", True), ("dense2", "f16_sum", False), "codebook"])
def test_density_alone_guards_and_repeatability(which):
    """want_rgb=False against the density of the full call; all outputs inside NaN-guarded buffers whose guard rows (in front of
    the first sample and behind the last) stay NaN; two runs give the same bits"""
    from wisp.ops.nerf_mlp import fused_nerf_octree_query
    nef = codebook_field("sparse4", 'sum') if which == "codebook" else field(*which)
    tree = "sparse4" if which == "codebook" else which[0]
    for n in COUNTS:
        coords, dirs = positions(tree, n, 300 + n)
        with torch.no_grad():
            rgb, den = fused_nerf_octree_query(nef, coords, ray_d=dirs)
            none, den_only = fused_nerf_octree_query(nef, coords, want_rgb=False)
            rgb_g, den_g = fused_nerf_octree_query(nef, coords, ray_d=dirs, pad_rows=70)
            none_g, den_only_g = fused_nerf_octree_query(nef, coords, want_rgb=False, pad_rows=70)
            rgb2, den2 = fused_nerf_octree_query(nef, coords, ray_d=dirs)
        assert none is None and none_g is None and torch.equal(den_only, den)
        assert torch.equal(rgb2, rgb) and torch.equal(den2, den)
        assert rgb_g.shape == (n + 140, 3) and den_g.shape == (n + 140, 1)
        for guarded, plain in ((rgb_g, rgb), (den_g, den), (den_only_g, den)):
            assert bool(torch.isnan(guarded[:70]).all()) and bool(torch.isnan(guarded[70 + n:]).all())
            assert torch.equal(guarded[70:70 + n], plain) and not bool(torch.isnan(plain).any())


@pytest.mark.parametrize("R", [1, 37])
@pytest.mark.parametrize("which", [("sparse4", "f5_sum", True), "codebook"])
def test_ray_directions_through_the_ray_index(which, R):
    """ray_dirs + ridx against per-sample dirs = ray_dirs.index_select(0, ridx): repeated and unsorted indices; indices outside
    [0, R) are clamped"""
    from wisp.ops.nerf_mlp import fused_nerf_octree_query
    nef = codebook_field("sparse4", 'cat') if which == "codebook" else field(*which)
    g = torch.Generator().manual_seed(R)
    for n in (1, 33, 65, 700):
        coords, _ = positions("sparse4", n, 200 + n)
        ray_dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=1).to(DEV)
        ridx = torch.randint(0, R, (n,), generator=g).to(DEV)
        if R > 1 and n > 2:
            ridx[0], ridx[1], ridx[2] = R - 1, 0, R - 1                              # unsorted and repeated, whatever was drawn
            assert not bool((ridx[1:] >= ridx[:-1]).all()) and ridx.unique().numel() < n
        per_sample = ray_dirs.index_select(0, ridx)
        wild = ridx.clone()
        wild[::3] += R * 5                                                           # past the last ray: clamped to R - 1
        wild[1::3] -= R * 7                                                          # negative: clamped to 0
        clamped = ray_dirs.index_select(0, wild.clamp(0, R - 1))
        with torch.no_grad():
            a = fused_nerf_octree_query(nef, coords, ray_dirs=ray_dirs, ridx=ridx)
            b = fused_nerf_octree_query(nef, coords, ray_d=per_sample)
            c = fused_nerf_octree_query(nef, coords, ray_dirs=ray_dirs, ridx=wild)
            d = fused_nerf_octree_query(nef, coords, ray_d=clamped)
        want = modular(nef, coords, per_sample)
        for x, y, z in zip(a, b, want):
            assert torch.equal(x, y) and torch.equal(x, z)
        for x, y in zip(c, d):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ the tracer
def _rays(n, seed, miss=False):
    from wisp.core import Rays
    o, d = make_rays(max(n, 1), seed)
    o, d = o[:n], d[:n]
    if miss:
        d = -d                                                  # away from the cube
    return Rays(cuda(o), cuda(d), dist_min=1.0, dist_max=5.0)


def _trace(nef, rays, march, channels, fused, steps):
    from wisp.tracers import PackedRFTracer
    tracer = PackedRFTracer(raymarch_type=march, num_steps=steps, bg_color=(0.2, 0.4, 0.6))
    if fused is not None:
        tracer.fused_query = fused
    torch.manual_seed(77)                                       # (the march's jitter seeds follow torch's CPU generator)
    with torch.no_grad():
        rb = tracer(nef, rays=rays, channels=channels)
    return rb, tracer.get_prev_num_samples()


def _same_buffers(a, b, channels):
    for ch in channels:
        x, y = getattr(a, ch), getattr(b, ch)
        assert x is not None and x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), ch


@functools.lru_cache(maxsize=None)
def traced_field(kind):
    """the YAML shapes (F = 5, 4 LODs, bias-free) on a shell-shaped level-5 octree that rays from outside meet"""
    from gpu_helpers import shell_blas
    from wisp.models.grids import CodebookOctreeGrid, OctreeGrid
    from wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(11)
    _, blas = shell_blas(5, 0.6, 0.12)
    multiscale = 'cat' if kind.endswith("_cat") else 'sum'
    shape = dict(feature_dim=5, num_lods=4, interpolation_type='linear', multiscale_type=multiscale, feature_std=0.5)
    grid = CodebookOctreeGrid(blas, codebook_bitwidth=4, **shape) if kind.startswith("codebook") else OctreeGrid(blas, **shape)
    nef = NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=64, num_layers=1, bias=False,
                              prune_density_decay=None, prune_min_density=None).to(DEV)
    with torch.no_grad():
        for n, p in nef.named_parameters():
            if 'decoder' in n:
                p.mul_(2.0)
        nef.decoder_density.lout.weight[0].abs_()
    nef.eval()
    return nef


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("march", ["ray", "voxel"])
@pytest.mark.parametrize("n", [1, 33, 700])
@pytest.mark.parametrize("kind", ["octree", "octree_cat", "codebook_cat", "codebook"])
def test_tracer_with_fused_query_equals_the_tracer_without(kind, n, march, depth, count_native):
    """bit-identical RenderBuffer; for the codebook 'sum' field (four levels: torch's order of the level sum) every channel of every
    ray within twice the modular tracer's own error against a float64 evaluation of the same samples"""
    nef = traced_field(kind)
    channels = ["rgb", "alpha", "hit"] + (["depth"] if depth else [])
    steps = 24 if march == "ray" else 16
    rays = _rays(n, 500 + n)
    off, s_off = _trace(nef, rays, march, channels, None, steps)
    assert len(count_native) == 0
    on, s_on = _trace(nef, rays, march, channels, True, steps)
    assert len(count_native) == 1 and s_on == s_off and (s_on > 0 or n == 1)
    if kind != "codebook":
        _same_buffers(on, off, channels)
    else:
        assert torch.equal(on.hit, off.hit)
        want = _composite64(nef, rays, march, steps, s_off, depth)
        for ch in [c for c in channels if c != "hit"]:
            # the bound of the codebook 'sum' query carried to the rays: over the batch, the fused tracer's largest error against
            # the float64 evaluation of the same samples is at most twice the modular tracer's, plus one float32 spacing of the
            # channel's largest value - what storing either result in float32 costs, and all there is when a one-ray batch leaves
            # the modular error at zero
            e_on, e_off = float(_err(getattr(on, ch), want[ch]).max()), float(_err(getattr(off, ch), want[ch]).max())
            slack = float(np.spacing(np.float32(np.abs(want[ch]).max())))
            margin(f"nerf_octree_query tracer codebook sum {march} n={n} depth={depth} {ch}: fused error vs twice the modular error "
                   f"plus one float32 spacing", e_on, 2.0 * e_off + slack)
    if n > 1:
        assert bool(on.hit.any()) and float(on.rgb.std()) > 0.0


def _composite64(nef, rays, march, steps, num_samples, depth, bg=(0.2, 0.4, 0.6)):
    """the tracer's channels from a float64 field evaluation of the tracer's own samples (same seed), composited in float64 by the
    oracle's compositing block"""
    from oracle import render as orender
    torch.manual_seed(77)
    with torch.no_grad():
        rm = nef.grid.raymarch(rays, level=nef.grid.active_lods[-1], num_samples=steps, raymarch_type=march)
    assert rm.samples.shape[0] == num_samples
    N = rays.origins.shape[0]
    ridx = rm.ridx.long().cpu()
    rgb, den = ref.field64(nef, rm.samples, rays.dirs.index_select(0, rm.ridx.long()))
    boundary = torch.ones(num_samples, dtype=torch.bool)
    boundary[1:] = ridx[1:] != ridx[:-1]
    out = orender.composite(torch.from_numpy(rgb), torch.from_numpy(den), rm.deltas.reshape(-1, 1).cpu().double(),
                            rm.depth_samples.reshape(-1, 1).cpu().double(), ridx, boundary, N, bg, with_depth=depth)
    return {k: v.numpy() for k, v in out.items() if k in ("rgb", "alpha", "depth") and v is not None}


def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:                                                          # noqa: BLE001
        return ("raised", type(e).__name__, str(e)[:120])


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("march", ["ray", "voxel"])
@pytest.mark.parametrize("kind", ["octree", "codebook"])
def test_tracer_on_an_all_miss_batch_and_an_empty_batch(kind, march, depth, count_native):
    """no sample at all: the fused query is called with n = 0 and launches nothing, and the tracer ends as it does without it"""
    nef = traced_field(kind)
    channels = ["rgb", "alpha", "hit"] + (["depth"] if depth else [])
    for rays in (_rays(33, 601, miss=True), _rays(0, 602)):
        off = _outcome(lambda: _trace(nef, rays, march, channels, False, 8))
        before = len(count_native)
        on = _outcome(lambda: _trace(nef, rays, march, channels, True, 8))
        assert len(count_native) == before + 1
        assert on[0] == off[0]
        if on[0] == "ok":
            (rb_on, s_on), (rb_off, s_off) = on[1], off[1]
            assert s_on == s_off == 0
            _same_buffers(rb_on, rb_off, channels)
            assert not bool(rb_on.hit.any())
        else:
            assert on[1:] == off[1:] and depth
        if not depth:
            assert on[0] == "ok"


@pytest.mark.parametrize("case", ["grad", "extra_channel", "autocast", "bf16_compute", "switch", "switch_unset", "codebook_training"])
def test_calls_that_stay_modular(case, count_native, monkeypatch):
    """fused_query = True changes nothing for these: no launch of the fused query, and the buffers of the same tracer without it"""
    from wisp.tracers import PackedRFTracer
    nef = make_nef("sparse4", 5, 'sum', bias=False, codebook=(case == "codebook_training"), seed=5)
    if case == "bf16_compute":
        nef.decoder_compute = 'bf16'
    if case == "switch":
        monkeypatch.setenv(SWITCH, "0")
    if case == "switch_unset":
        monkeypatch.delenv(SWITCH)
    if case == "codebook_training":
        nef.train()
    rays = _rays(200, 700)
    channels = ["rgb", "alpha"] + (["density"] if case == "extra_channel" else [])
    out = []
    for fused in (True, False):
        tracer = PackedRFTracer(raymarch_type='ray', num_steps=16, bg_color=(0.0, 0.0, 0.0))
        tracer.fused_query = fused
        torch.manual_seed(78)
        with torch.set_grad_enabled(case == "grad"), torch.autocast('cuda', dtype=torch.bfloat16, enabled=(case == "autocast")):
            out.append(tracer(nef, rays=rays, channels=channels))
        assert tracer.get_prev_num_samples() > 0
    assert len(count_native) == 0
    if case == "grad":
        assert out[0].rgb.requires_grad                          # the training path: still differentiable
        assert torch.allclose(out[0].rgb, out[1].rgb, atol=1e-6)
    else:
        _same_buffers(out[0], out[1], channels)


# ------------------------------------------------------------------------------------------------ the decoded-table cache
def test_cache_is_rebuilt_after_an_optimizer_step_and_a_load(count_native):
    """after an optimizer step on a codebook field - torch's, and the raw-pointer step of MultiviewTrainStep's flat buffer, which
    leaves the version counters alone - and after load_state_dict, the next fused query equals a fresh modular evaluation"""
    import wisp._C as C
    from wisp.ops.nerf_mlp import fused_nerf_octree_query
    nef = make_nef("sparse4", 5, 'cat', bias=False, codebook=True, seed=8)
    coords, dirs = positions("sparse4", 700, 900)
    decodes = []
    inner = C.codebook_decode_rows

    def query():
        with torch.no_grad():
            return fused_nerf_octree_query(nef, coords, ray_d=dirs)

    def check(moved):
        rgb, den = query()
        want_rgb, want_den = modular(nef, coords, dirs)
        assert torch.equal(rgb, want_rgb) and torch.equal(den, want_den)
        return rgb

    first = check(False)
    tables = nef.grid.decoded_tables()
    assert all(a is b for a, b in zip(tables, nef.grid.decoded_tables()))             # nothing changed: the same tensors
    assert "_decoded_cache" not in nef.state_dict() and not any("decoded" in k for k in nef.state_dict())
    state = {k: v.clone() for k, v in nef.state_dict().items()}
    opt = torch.optim.SGD(nef.grid.parameters(), lr=50.0)
    nef.train()
    loss = (nef.grid.interpolate(coords[:200], 3) ** 2).sum()
    loss.backward()
    opt.step()
    nef.eval()
    second = check(True)
    assert not torch.equal(first, second)                                             # the step moved argmaxes
    assert not any(a is b for a, b in zip(tables, nef.grid.decoded_tables()))
    nef.load_state_dict(state)
    assert torch.equal(check(True), first)
    # a write that leaves the version counters alone, as the trainers' raw-pointer optimizer kernels do, announced the way
    # FlatParams announces theirs
    from wisp.ops.grid import note_raw_parameter_write
    f = nef.grid.features[0]
    version, ptr = f._version, f.data_ptr()
    f.data.copy_(torch.flip(f.detach(), dims=[1]))
    assert f._version == version and f.data_ptr() == ptr
    note_raw_parameter_write()
    assert not torch.equal(check(True), first)


# ------------------------------------------------------------------------------------------------ the evaluation surface
@pytest.mark.parametrize("kind", ["octree", "codebook_cat"])
def test_evaluate_metrics_on_two_views(kind, tmp_path, count_native, monkeypatch):
    """PSNR equal to evaluate_psnr's; the PNGs of a fused and of a modular evaluation are the same bytes"""
    from gpu_helpers import _dropin_trainer
    from wisp.datasets import MultiviewTensorDataset
    from wisp.models import Pipeline
    from wisp.ops.image import read_png
    from wisp.tracers import PackedRFTracer
    from wisp.trainers.validation import evaluate_psnr
    nef = traced_field(kind)
    pipe = Pipeline(nef, PackedRFTracer(raymarch_type='voxel', num_steps=16, bg_color=(0.0, 0.0, 0.0)))
    trainer = _dropin_trainer(pipe, amp=False)
    views = []
    for v in range(2):
        o, d = make_rays(32 * 32, 800 + v)
        views.append((cuda(o), cuda(d)))
    origins, dirs = torch.stack([v[0] for v in views]), torch.stack([v[1] for v in views])
    gts = torch.rand(2, 32 * 32, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    ds = MultiviewTensorDataset(origins, dirs, gts, 1.0, 5.0, img_shape=torch.Size([32, 32]))
    trainer.validation_dataset = ds
    trainer.cfg.save_valid_imgs = True
    files = {}
    for mode in ("fused", "modular"):
        monkeypatch.setenv(SWITCH, "1" if mode == "fused" else "0")
        trainer.tracker.log_dir = str(tmp_path / mode)
        trainer.return_dict = {}
        before = len(count_native)
        torch.manual_seed(3)
        got = trainer.validate()
        pipe.eval()
        assert (len(count_native) > before) == (mode == "fused")
        assert not hasattr(pipe.tracer, "fused_query")
        names = sorted(os.listdir(tmp_path / mode / "val"))
        assert names == ["0-lod3.png", "1-lod3.png"]
        files[mode] = [open(tmp_path / mode / "val" / f, "rb").read() for f in names]
        assert read_png(str(tmp_path / mode / "val" / names[0])).shape == (32, 32, 3)
        torch.manual_seed(3)
        rays = ds.data["rays"]
        mean, _ = evaluate_psnr(pipe, [(rays[i], gts[i]) for i in range(2)])
        assert float(got["psnr"]) == float(mean), (mode, got, mean)
    assert files["fused"] == files["modular"]
    assert len(np.unique(np.frombuffer(files["fused"][0], np.uint8))) > 16


def test_render_script_end_to_end_on_a_codebook_field(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_nerf.py"), "--write-synlego", str(tmp_path / "scene"),
                          "--grid", "codebook", "--octree-level", "5", "--cloud-rays", "16384", "--steps", "20", "--train-views", "4",
                          "--train-res", "32", "--views", "2", "--res", "32", "32", "--render-batch", "500",
                          "--out", str(tmp_path / "out")], capture_output=True, text=True, timeout=300, env=dict(os.environ, **{SWITCH: "1"}))
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["frames"] == 2 and rec["grid"] == "codebook" and rec["fused_octree_query"] is True and rec["fused_query"] is False
    assert rec["ms_per_frame"] > 0 and rec["samples_per_frame"] > 0
    assert rec["field"]["grid"] == "CodebookOctreeGrid" and rec["field"]["num_lods"] == 4 and rec["field"]["feature_dim"] == 5
    from wisp.ops.image import read_png
    for k in range(2):
        for kind, ch in (("rgb", 3), ("depth", 3), ("alpha", 1)):
            img = read_png(str(tmp_path / "out" / f"{kind}_{k:03d}.png"))
            assert img.shape == (32, 32, ch) and img.dtype == np.uint8, (kind, img.shape)
