"""GPU: the fused field query of a triplanar radiance field (csrc/nerf_triplane_query.hip,
wisp.ops.nerf_mlp.fused_nerf_triplane_query) and what is built on it - PackedRFTracer's `fused_query` attribute on TriplanarGrid
fields, MultiviewTrainer.evaluate_metrics, scripts/render_nerf.py --grid triplanar.

What is held to bits: the feature rows against the float64 reference on exactly representable cases (tests/nerf_triplane_query_ref.py;
tests/test_nerf_triplane_query_host.py shows that they are exact); rgb and density against the exact-fp32 decoder launched on the
kernel's own feature rows; the tracer against the modular tracer fed those rows.  What cannot be: the feature rows against the modular
lookup (triplane_kernel leaves its contraction to the compiler) - there the fused query's error against the float64 reference is at
most twice the modular path's own.

The positions of the generic cases hold one row each of NaN, +1e30, -1e30 and 0.  wisp_reflect_source_index (csrc/grid_sample_dev.h)
was read for them: fabsf / floorf carry a NaN to `extra`, fminf bounds `flips` before the cast to int, and the closing
fminf(fmaxf(x, 0), span) returns a coordinate in [0, size - 1] for a NaN (fmaxf drops it) and for any finite overshoot of 1e30 * span
(no infinity arises below 2^127 / 257), so x0, y0 lie inside the plane and the +1 corners are guarded by x0 + 1 < size.

Every measured margin is appended to the file WISP_NERF_TRIPLANE_QUERY_MARGINS names (profiles/nerf_triplane_query_test_margins.jsonl
is such a run)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nerf_triplane_query_ref as ref
import triplane_sdf_eval_ref as tri
from gpu_helpers import DEV, cuda, make_rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "WISP_NERF_TRIPLANE_QUERY_FUSED"
COUNTS = ref.COUNTS
# generic fields: name -> (features per plane, multiscale, log2 of the first span, levels); "yaml" is nerf_triplanar.yaml's own
# shape (planes of 33 / 65 / 129 / 257 texels a side)
GENERIC = {"yaml": (4, 'sum', 5, 4), "f10_sum2": (10, 'sum', 2, 2), "f5_cat2": (5, 'cat', 4, 2)}
SPECIAL_ROWS = {10: [float("nan"), 0.3, -0.2], 11: [1e30, -0.5, 0.25], 12: [0.1, -1e30, 1e30], 13: [0.0, 0.0, 0.0]}


def record(name, value, limit=None):
    path = os.environ.get("WISP_NERF_TRIPLANE_QUERY_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, value=float(value), limit=None if limit is None else float(limit))) + "\n")


def make_nef(F, multiscale, base, lods, bias=True, hidden=64, seed=0, std=0.5, interpolation='linear', pos_embedder='none'):
    from wisp.accelstructs import AxisAlignedBBoxAS
    from wisp.models.grids import TriplanarGrid
    from wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(seed)
    grid = TriplanarGrid(AxisAlignedBBoxAS(), feature_dim=F, log_base_resolution=base, num_lods=lods, interpolation_type=interpolation,
                         multiscale_type=multiscale, feature_std=std)
    nef = NeuralRadianceField(grid, pos_embedder=pos_embedder, view_embedder='positional', view_multires=4, hidden_dim=hidden,
                              num_layers=1, bias=bias, prune_density_decay=None, prune_min_density=None).to(DEV)
    with torch.no_grad():
        for n, p in nef.named_parameters():
            if 'decoder' in n:
                p.mul_(2.0)            # wider activations so relu masks and the sigmoid are exercised
        if not bias:
            nef.decoder_density.lout.weight[0].abs_()          # (without the output bias most density logits are negative)
    nef.eval()
    return nef


@functools.lru_cache(maxsize=None)
def exact_field(name, bias=True):
    """an exact case's field: the planes of ref.exact_case_inputs (integers in [-1, 1]) under a random decoder"""
    F, multiscale, base, lods = ref.EXACT_CASES[name]
    nef = make_nef(F, multiscale, base, lods, bias=bias, seed=3)
    planes, sizes, _, _ = ref.exact_case_inputs(name, 1)
    with torch.no_grad():
        for i, v in enumerate(nef.grid.features):
            assert v.fmx.shape[-1] == sizes[i]
            for p, src in zip((v.fmx, v.fmy, v.fmz), planes[3 * i:3 * i + 3]):
                p.copy_(src.reshape(p.shape))
    return nef


@functools.lru_cache(maxsize=None)
def generic_field(name, bias=True):
    return make_nef(*GENERIC[name], bias=bias, seed=5)


@functools.lru_cache(maxsize=None)
def directions(n, seed=0):
    g = torch.Generator().manual_seed(900 + n + seed)
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).to(DEV)


@functools.lru_cache(maxsize=None)
def generic_positions(n):
    """ref.generic_points plus - where n allows - the rows of SPECIAL_ROWS"""
    c = ref.generic_points(n, seed=60 + n).clone()
    for row, value in SPECIAL_ROWS.items():
        if row < n:
            c[row] = torch.tensor(value)
    return c.to(DEV)


def ordinary(coords):
    """the rows a float64 reference has an opinion on"""
    return (torch.isfinite(coords).all(dim=1) & (coords.abs() < 1e29).all(dim=1)).cpu()


def _lods(nef):
    return list(range(nef.grid.num_lods)) if nef.grid.multiscale_type == 'sum' else [nef.grid.num_lods - 1]


def modular(nef, coords, dirs, lod_idx=None):
    """lookup + decoder as the modular path launches them -> (rgb, density, feats)"""
    from wisp.ops.nerf_mlp import fused_nerf_decoder
    if lod_idx is None:
        lod_idx = nef.grid.num_lods - 1
    with torch.no_grad():
        feats = nef.grid.interpolate(coords, lod_idx).reshape(coords.shape[0], nef.effective_feature_dim())
        assert feats.dtype == torch.float32
        return fused_nerf_decoder(nef, feats, dirs) + (feats,)


def query(nef, coords, **kw):
    from wisp.ops.nerf_mlp import fused_nerf_triplane_query
    with torch.no_grad():
        return fused_nerf_triplane_query(nef, coords, **kw)


def ulps(a, b):
    """largest distance of two finite float32 tensors in units in the last place"""
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


def _err(got, want64):
    return float(np.abs(got.detach().cpu().double().numpy() - want64).max())


@pytest.fixture
def count_native(monkeypatch):
    """counts the launches of the fused triplanar query; the tests set the switch themselves, whatever its default"""
    import wisp._C as C
    calls = []
    inner = C.nerf_triplane_query

    def spy(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)
    monkeypatch.setattr(C, "nerf_triplane_query", spy)
    monkeypatch.setenv(SWITCH, "1")
    return calls


# ------------------------------------------------------------------------------------------------ 1. feature rows, exact
@pytest.mark.parametrize("name", list(ref.EXACT_CASES))
def test_feature_rows_equal_the_float64_reference_bit_for_bit(name, count_native):
    """every sample count, every valid lod_idx: feats_out is the float64 features(...) of the same planes and positions"""
    from wisp.ops.nerf_mlp import nerf_octree_query_supported, nerf_query_supported, nerf_triplane_query_supported
    nef = exact_field(name)
    with torch.no_grad():
        assert nerf_triplane_query_supported(nef) and not nerf_query_supported(nef) and not nerf_octree_query_supported(nef)
    F, multiscale, base, lods = ref.EXACT_CASES[name]
    nonzero = 0
    for n in COUNTS:
        planes, sizes, coords, bits = ref.exact_case_inputs(name, n)
        c = coords.to(DEV)
        for lod_idx in _lods(nef):
            want = ref.features64(nef, coords, lod_idx)
            before = len(count_native)
            rgb, den, feats = query(nef, c, ray_d=directions(n), lod_idx=lod_idx, want_feats=True)
            assert len(count_native) == before + 1
            assert feats.shape == want.shape == (n, nef.effective_feature_dim()) and feats.dtype == torch.float32
            assert rgb.shape == (n, 3) and den.shape == (n, 1)
            got = feats.cpu().double().numpy()
            assert np.array_equal(got, want), (name, n, lod_idx, float(np.abs(got - want).max()))
            nonzero += int((got != 0).sum())
    assert nonzero > 1000 * (1 if F > 1 else 0)
    record(f"nerf_triplane_query exact feature rows {name}: nonzero entries compared", nonzero)


# ------------------------------------------------------------------------------------------------ 2. the decoder stage
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name", ["exact:" + k for k in ref.EXACT_CASES] + ["generic:" + k for k in GENERIC])
def test_rgb_and_density_equal_the_decoder_on_the_kernels_own_rows(name, bias):
    from wisp.ops.nerf_mlp import fused_nerf_decoder
    kind, key = name.split(":")
    nef = exact_field(key, bias) if kind == "exact" else generic_field(key, bias)
    lit = 0
    for n in COUNTS:
        coords = ref.exact_case_inputs(key, n)[2].to(DEV) if kind == "exact" else generic_positions(n)
        dirs = directions(n)
        for lod_idx in _lods(nef)[-2:]:
            rgb, den, feats = query(nef, coords, ray_d=dirs, lod_idx=lod_idx, want_feats=True)
            with torch.no_grad():
                want_rgb, want_den = fused_nerf_decoder(nef, feats, dirs)
            assert torch.equal(den, want_den), (name, bias, n, lod_idx, "density")
            assert torch.equal(rgb, want_rgb), (name, bias, n, lod_idx, "rgb")
            assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(den).all())
            lit += int((den > 0).sum())
    assert lit > 0 and float(rgb.std()) > 0.0


# ------------------------------------------------------------------------------------------------ 3. generic error
@pytest.mark.parametrize("name", list(GENERIC))
def test_generic_error_within_twice_the_modular_error(name):
    """feats_out, rgb and density against the float64 reference: at most twice the modular path's own error (both are float32
    evaluations of one expression that round at different places).  The distance from the modular result in ulps is recorded."""
    nef = generic_field(name)
    for n in (65, 700):
        coords, dirs = generic_positions(n), directions(n)
        ok = ordinary(coords)
        assert int((~ok).sum()) == 3
        for lod_idx in _lods(nef):
            rgb, den, feats = query(nef, coords, ray_d=dirs, lod_idx=lod_idx, want_feats=True)
            m_rgb, m_den, m_feats = modular(nef, coords, dirs, lod_idx)
            c_ok, d_ok = coords[ok.to(DEV)], dirs[ok.to(DEV)]
            want_feats = ref.features64(nef, c_ok, lod_idx)
            want_rgb, want_den = ref.field64(nef, c_ok, d_ok, lod_idx)
            assert float(np.abs(want_feats).max()) > 0.1
            sel = ok.to(DEV)
            for what, got, mod, want in (("feats", feats, m_feats, want_feats), ("rgb", rgb, m_rgb, want_rgb),
                                         ("density", den, m_den, want_den)):
                e_f, e_m = _err(got[sel], want), _err(mod[sel], want)
                tag = f"nerf_triplane_query generic {name} n={n} lod_idx={lod_idx} {what}"
                record(f"{tag}: fused error vs twice the modular error", e_f, 2.0 * e_m)
                record(f"{tag}: distance from the modular result in ulps", ulps(got[sel], mod[sel]))
                assert e_m > 0.0 and e_f <= 2.0 * e_m, (tag, e_f, e_m)


@pytest.mark.parametrize("name", list(GENERIC))
def test_nan_and_huge_positions_leave_their_neighbours_alone(name):
    """a row of NaN, of +1e30 or of -1e30 is answered with a finite result that equals the same row queried alone, and the other rows
    equal those of a batch in which the four special rows are replaced by ordinary points"""
    nef = generic_field(name)
    n = 700
    coords, dirs = generic_positions(n), directions(n)
    plain = coords.clone()
    for row in SPECIAL_ROWS:
        plain[row] = torch.tensor([0.25, -0.5, 0.75], device=DEV)
    a = query(nef, coords, ray_d=dirs, want_feats=True)
    b = query(nef, plain, ray_d=dirs, want_feats=True)
    others = torch.ones(n, dtype=torch.bool, device=DEV)
    others[list(SPECIAL_ROWS)] = False
    for x, y in zip(a, b):
        assert torch.equal(x[others], y[others]) and bool(torch.isfinite(x).all())
    for row in SPECIAL_ROWS:
        alone = query(nef, coords[row:row + 1].contiguous(), ray_d=dirs[row:row + 1].contiguous(), want_feats=True)
        for x, y in zip(a, alone):
            assert torch.equal(x[row:row + 1], y), (name, row)
    zero = ref.features64(nef, torch.zeros(1, 3))
    assert np.allclose(a[2][13].cpu().double().numpy(), zero[0], rtol=0, atol=1e-5 * float(np.abs(zero).max()))


def test_planes_of_one_and_two_texels_through_the_c_wrapper():
    """sizes the grid class cannot build: a 1 x 1 plane (span 0: every position reads texel 0 with weight 1, no +1 corner) and a
    2 x 2 plane, 'cat' behind one another and summed - against the float64 reference, which is exact here for positions on the
    dyadic lattice"""
    import wisp._C as C
    from wisp.ops.nerf_mlp import _decoder_tensors, _pack, fused_nerf_decoder
    rng = np.random.default_rng(12)
    F, sizes = 2, [1, 2]
    planes = [torch.from_numpy(rng.integers(-1, 2, size=(F, R, R)).astype(np.float32)) for R in sizes for _ in range(3)]
    planes[0][:] = 1.0                                          # (a 1 x 1 plane that is not zero)
    dev_planes = [p.to(DEV) for p in planes]
    for multiscale, lods in (('sum', 2), ('cat', 2), ('sum', 1)):
        nef = make_nef(F, multiscale, 2, lods, seed=9)          # (its own planes are not used: the decoder is what is borrowed)
        I, H = nef.effective_feature_dim(), 64
        shapes = ((H, I), (H,), (16, H), (16,), (H, 42), (H,), (H, H), (H,), (3, H), (3,))
        packed = _pack(_decoder_tensors(nef), shapes)
        fld = dict(planes=planes[:3 * lods], multiscale=multiscale)
        for n in COUNTS:
            coords = ref.exact_points(n, b=1, seed=70 + n)
            ref.check_exact_features(fld, coords, ref.exact_bits([2], b=1))
            dirs = directions(n)
            with torch.no_grad():
                rgb, den, feats = C.nerf_triplane_query(coords.to(DEV), dirs, None, dev_planes[:3 * lods], sizes[:lods], F,
                                                        multiscale == 'sum', packed, I, H, want_feats=True)
                want_rgb, want_den = fused_nerf_decoder(nef, feats, dirs)
            assert np.array_equal(feats.cpu().double().numpy(), tri.features(fld, coords).numpy()), (multiscale, lods, n)
            assert torch.equal(rgb, want_rgb) and torch.equal(den.reshape(-1, 1), want_den)
            if lods == 1:
                assert bool((feats[:, :F] == 1.0).all())       # plane x: texel 0 with weight 1 wherever the position lies


# ------------------------------------------------------------------------------------------------ 4. density alone, guards
@pytest.mark.parametrize("name", ["exact:f4_sum4", "exact:f5_cat2", "generic:yaml", "generic:f10_sum2"])
def test_density_alone_guards_and_repeatability(name):
    """want_rgb=False against the density of the full call; all outputs inside NaN-guarded buffers whose guard rows (in front of
    the first sample and behind the last) stay NaN; two runs give the same bits"""
    kind, key = name.split(":")
    nef = exact_field(key) if kind == "exact" else generic_field(key)
    for n in COUNTS:
        coords = ref.exact_case_inputs(key, n)[2].to(DEV) if kind == "exact" else generic_positions(n)
        dirs = directions(n)
        rgb, den, feats = query(nef, coords, ray_d=dirs, want_feats=True)
        none, den_only, feats_only = query(nef, coords, want_rgb=False, want_feats=True)
        rgb_g, den_g, feats_g = query(nef, coords, ray_d=dirs, pad_rows=70, want_feats=True)
        none_g, den_only_g = query(nef, coords, want_rgb=False, pad_rows=70)
        rgb2, den2, feats2 = query(nef, coords, ray_d=dirs, want_feats=True)
        rgb3, den3 = query(nef, coords, ray_d=dirs)
        assert none is None and none_g is None and torch.equal(den_only, den) and torch.equal(feats_only, feats)
        assert torch.equal(rgb2, rgb) and torch.equal(den2, den) and torch.equal(feats2, feats)
        assert torch.equal(rgb3, rgb) and torch.equal(den3, den)                     # with and without the feature rows
        assert rgb_g.shape == (n + 140, 3) and den_g.shape == (n + 140, 1) and feats_g.shape == (n + 140, feats.shape[1])
        for guarded, plain in ((rgb_g, rgb), (den_g, den), (den_only_g, den), (feats_g, feats)):
            assert bool(torch.isnan(guarded[:70]).all()) and bool(torch.isnan(guarded[70 + n:]).all())
            assert torch.equal(guarded[70:70 + n], plain) and not bool(torch.isnan(plain).any())


# ------------------------------------------------------------------------------------------------ 5. the ray index
@pytest.mark.parametrize("R", [1, 37])
@pytest.mark.parametrize("name", ["generic:yaml", "exact:f5_cat2"])
def test_ray_directions_through_the_ray_index(name, R):
    """ray_dirs + ridx against per-sample dirs = ray_dirs.index_select(0, ridx): repeated and unsorted indices; indices outside
    [0, R) are clamped"""
    kind, key = name.split(":")
    nef = exact_field(key) if kind == "exact" else generic_field(key)
    g = torch.Generator().manual_seed(R)
    for n in (1, 33, 65, 700):
        coords = generic_positions(n)
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
        a = query(nef, coords, ray_dirs=ray_dirs, ridx=ridx)
        b = query(nef, coords, ray_d=per_sample)
        c = query(nef, coords, ray_dirs=ray_dirs, ridx=wild)
        d = query(nef, coords, ray_d=clamped)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        for x, y in zip(c, d):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 6. live parameters
def test_the_planes_are_read_at_every_call():
    """nothing is cached: an in-place change of one plane and a load_state_dict show in the next call"""
    nef = make_nef(4, 'sum', 3, 3, seed=21)
    coords, dirs = generic_positions(700), directions(700)
    ok = ordinary(coords).to(DEV)
    first = query(nef, coords, ray_d=dirs, want_feats=True)
    state = {k: v.clone() for k, v in nef.state_dict().items()}
    with torch.no_grad():
        nef.grid.features[1].fmy.mul_(-3.0)                     # in place: the storage stays, its contents move
    second = query(nef, coords, ray_d=dirs, want_feats=True)
    assert not torch.equal(second[2], first[2]) and not torch.equal(second[0], first[0])
    want = ref.features64(nef, coords[ok])
    assert _err(second[2][ok], want) <= 1e-5 * float(np.abs(want).max())             # ... to what the field now is
    cols = second[2][ok] != first[2][ok]
    assert bool(cols[:, 4:8].any()) and not bool(cols[:, :4].any()) and not bool(cols[:, 8:].any())    # plane y's columns alone
    moved = {k: v + 0.25 if "fmz" in k else v for k, v in state.items()}
    nef.load_state_dict(moved)
    third = query(nef, coords, ray_d=dirs, want_feats=True)
    assert bool((third[2][ok][:, 8:] != first[2][ok][:, 8:]).any()) and torch.equal(third[2][:, :8], first[2][:, :8])
    nef.load_state_dict(state)
    again = query(nef, coords, ray_d=dirs, want_feats=True)
    for x, y in zip(again, first):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 7, 8. the tracer
def _rays(n, seed, miss=False):
    from wisp.core import Rays
    o, d = make_rays(max(n, 1), seed)
    o, d = o[:n], d[:n]
    if miss:
        d = -d                                                  # away from the cube
    return Rays(cuda(o), cuda(d), dist_min=1.0, dist_max=5.0)


def _trace(nef, rays, channels, fused, steps, **kw):
    from wisp.tracers import PackedRFTracer
    tracer = PackedRFTracer(raymarch_type='voxel', num_steps=steps, bg_color=(0.2, 0.4, 0.6))
    if fused is not None:
        tracer.fused_query = fused
    torch.manual_seed(77)                                       # (the march's jitter seeds follow torch's CPU generator)
    with torch.no_grad():
        rb = tracer(nef, rays=rays, channels=channels, **kw)
    return rb, tracer.get_prev_num_samples()


def _same_buffers(a, b, channels):
    for ch in channels:
        x, y = getattr(a, ch), getattr(b, ch)
        assert x is not None and x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), ch


def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:                                                          # noqa: BLE001
        return ("raised", type(e).__name__, str(e)[:120])


@pytest.fixture
def kernel_rows_as_lookup(monkeypatch):
    """nef.grid.interpolate replaced by the kernel's own feats_out rows: what is left of the modular tracer is the index_select of
    the directions, the decoder launch and the compositing"""
    def patch(nef):
        def interpolate(coords, lod_idx):
            return query(nef, coords.reshape(-1, 3).contiguous(), want_rgb=False, lod_idx=lod_idx, want_feats=True)[2]
        monkeypatch.setattr(nef.grid, "interpolate", interpolate)
    return patch


@functools.lru_cache(maxsize=None)
def traced_field():
    """nerf_triplanar.yaml's shape with planes that give the rays something to see"""
    return make_nef(4, 'sum', 5, 4, bias=False, seed=11)


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("steps", [8, 64])
@pytest.mark.parametrize("n", [1, 33, 700])
def test_tracer_with_fused_query_equals_the_tracer_on_the_kernels_rows(n, steps, depth, count_native, kernel_rows_as_lookup):
    """bit-identical RenderBuffer against the modular tracer fed the kernel's feature rows; against the unpatched modular tracer the
    largest colour difference stays inside the project's fp32 colour parity bound, 1e-4"""
    nef = traced_field()
    channels = ["rgb", "alpha", "hit"] + (["depth"] if depth else [])
    rays = _rays(n, 500 + n)
    plain, s_plain = _trace(nef, rays, channels, None, steps)
    assert len(count_native) == 0
    on, s_on = _trace(nef, rays, channels, True, steps)
    assert len(count_native) == 1 and s_on == s_plain and s_on > 0
    kernel_rows_as_lookup(nef)
    off, s_off = _trace(nef, rays, channels, False, steps)
    assert s_off == s_on and len(count_native) >= 2             # (the patched lookup launches the kernel for its rows)
    _same_buffers(on, off, channels)
    diff = float((on.rgb - plain.rgb).abs().max())
    record(f"nerf_triplane_query tracer n={n} steps={steps} depth={depth}: largest colour difference from the modular tracer", diff, 1e-4)
    assert diff <= 1e-4 and torch.equal(on.hit, plain.hit)
    assert bool(on.hit.any()) and (n == 1 or float(on.rgb.std()) > 0.0)


@pytest.mark.parametrize("depth", [False, True])
def test_tracer_on_an_all_miss_batch_and_an_empty_batch(depth, count_native):
    """no sample at all: the fused query is called with n = 0 and launches nothing, and the tracer ends as it does without it"""
    nef = traced_field()
    channels = ["rgb", "alpha", "hit"] + (["depth"] if depth else [])
    for rays in (_rays(33, 601, miss=True), _rays(0, 602)):
        off = _outcome(lambda: _trace(nef, rays, channels, False, 8))
        before = len(count_native)
        on = _outcome(lambda: _trace(nef, rays, channels, True, 8))
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


# ------------------------------------------------------------------------------------------------ 9. calls that stay modular
@pytest.mark.parametrize("case", ["switch", "grad", "extra_channel", "autocast", "hidden128", "closest", "pos_embedder", "columns33",
                                  "cat_below_last", "half_planes"])
def test_calls_that_stay_modular(case, count_native, monkeypatch):
    """fused_query = True changes nothing for these: no launch of the fused query, and the outcome - buffers, or the error the
    modular path raises for a field it does not cover either - of the same tracer without it"""
    from wisp.tracers import PackedRFTracer
    shape = dict(F=4, multiscale='sum', base=3, lods=3, bias=False, seed=5)
    if case == "hidden128":
        shape["hidden"] = 128
    if case == "closest":
        shape["interpolation"] = 'closest'
    if case == "pos_embedder":
        shape["pos_embedder"] = 'positional'
    if case == "columns33":
        shape["F"] = 11
    if case == "cat_below_last":
        shape.update(multiscale='cat', lods=2)
    nef = make_nef(**shape)
    if case == "half_planes":
        for v in nef.grid.features:
            for p in (v.fmx, v.fmy, v.fmz):
                p.data = p.data.half()
    if case == "switch":
        monkeypatch.setenv(SWITCH, "0")
    rays = _rays(200, 700)
    channels = ["rgb", "alpha"] + (["density"] if case == "extra_channel" else [])
    kw = dict(lod_idx=0) if case == "cat_below_last" else {}
    out = []
    for fused in (True, False):
        def run():
            tracer = PackedRFTracer(raymarch_type='voxel', num_steps=16, bg_color=(0.0, 0.0, 0.0))
            tracer.fused_query = fused
            torch.manual_seed(78)
            with torch.set_grad_enabled(case == "grad"), torch.autocast('cuda', dtype=torch.bfloat16, enabled=(case == "autocast")):
                rb = tracer(nef, rays=rays, channels=channels, **kw)
            assert tracer.get_prev_num_samples() > 0
            return rb
        out.append(_outcome(run))
    assert len(count_native) == 0
    assert out[0][0] == out[1][0], out
    if out[0][0] == "raised":
        assert out[0][1:] == out[1][1:] and case in ("closest", "cat_below_last"), out
    elif case == "grad":
        assert out[0][1].rgb.requires_grad                       # the training path: still differentiable
        assert torch.allclose(out[0][1].rgb, out[1][1].rgb, atol=1e-6)
    else:
        _same_buffers(out[0][1], out[1][1], channels)


# ------------------------------------------------------------------------------------------------ 10. the evaluation surface
def test_evaluate_metrics_on_two_views(tmp_path, count_native, monkeypatch):
    """MultiviewTrainer's validation on two 16 x 16 views launches the query and writes the PNGs; its PSNR is within 0.1 dB of the
    modular run's, the project's PSNR parity bound"""
    from gpu_helpers import _dropin_trainer
    from wisp.datasets import MultiviewTensorDataset
    from wisp.models import Pipeline
    from wisp.ops.image import read_png
    from wisp.tracers import PackedRFTracer
    nef = traced_field()
    pipe = Pipeline(nef, PackedRFTracer(raymarch_type='voxel', num_steps=16, bg_color=(0.0, 0.0, 0.0)))
    trainer = _dropin_trainer(pipe, amp=False)
    views = []
    for v in range(2):
        o, d = make_rays(16 * 16, 800 + v)
        views.append((cuda(o), cuda(d)))
    origins, dirs = torch.stack([v[0] for v in views]), torch.stack([v[1] for v in views])
    gts = torch.rand(2, 16 * 16, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    ds = MultiviewTensorDataset(origins, dirs, gts, 1.0, 5.0, img_shape=torch.Size([16, 16]))
    trainer.validation_dataset = ds
    trainer.cfg.save_valid_imgs = True
    psnr = {}
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
        img = read_png(str(tmp_path / mode / "val" / names[0]))
        assert img.shape == (16, 16, 3) and len(np.unique(img)) > 16
        psnr[mode] = float(got["psnr"])
    gap = abs(psnr["fused"] - psnr["modular"])
    record("nerf_triplane_query evaluate_metrics: PSNR distance from the modular run in dB", gap, 0.1)
    assert np.isfinite(psnr["fused"]) and gap <= 0.1, psnr


# ------------------------------------------------------------------------------------------------ 11. the render script
def test_render_script_end_to_end_on_a_triplanar_field(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_nerf.py"), "--write-synlego", str(tmp_path / "scene"),
                          "--grid", "triplanar", "--steps", "6", "--train-views", "4", "--train-res", "32", "--num-steps", "64",
                          "--views", "2", "--res", "48", "48", "--render-batch", "1000", "--out", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, **{SWITCH: "1"}))
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["frames"] == 2 and rec["grid"] == "triplanar" and rec["fused_query_route"] == "triplanar"
    assert rec["fused_triplane_query"] is True and rec["fused_query"] is False and rec["fused_octree_query"] is False
    assert rec["ms_per_frame"] > 0 and rec["samples_per_frame"] > 0
    assert rec["field"]["grid"] == "TriplanarGrid" and rec["field"]["num_lods"] == 4 and rec["field"]["feature_dim"] == 12
    assert rec["field"]["multiscale_type"] == "sum" and rec["field"]["hidden_dim"] == 64
    from wisp.ops.image import read_png
    for k in range(2):
        for kind, ch in (("rgb", 3), ("depth", 3), ("alpha", 1)):
            img = read_png(str(tmp_path / "out" / f"{kind}_{k:03d}.png"))
            assert img.shape == (48, 48, ch) and img.dtype == np.uint8, (kind, img.shape)
