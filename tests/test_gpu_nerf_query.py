"""GPU: the fused field query (csrc/nerf_query.hip, wisp.ops.nerf_mlp.fused_nerf_query) and what is built on it - PackedRFTracer's
`fused_query` attribute, MultiviewTrainer.evaluate_metrics, scripts/render_nerf.py - against the modular path (hashgrid_interpolate
on the fp32 table, the exact-fp32 decoder, index_select of the ray directions).  The contract is equality of bits: torch.equal on
rgb and density and on every channel of a traced RenderBuffer.  One check leaves the package: the CPU oracle, at the project's fp32
parity bound for colours."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_helpers import DEV, cuda, make_rays, margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NERF_HASH = dict(kind="geometric", num_lods=16, bitwidth=19, min_res=16, max_res=512)       # nerf_hash.yaml: 15 of 16 levels live
SMALL = dict(kind="geometric", num_lods=6, bitwidth=12, min_res=4, max_res=64)              # in_dim 12: dense and hashed levels
WRAP = dict(kind="geometric", num_lods=16, bitwidth=10, min_res=16, max_res=512)            # 2^10 rows: every level is hashed and wraps
NARROW = dict(kind="geometric", num_lods=4, bitwidth=12, min_res=8, max_res=64)             # in_dim 8, 3 live levels
# res 65536 at bitwidth 17: res^2 and res^3 wrap to 0 in the reference's int32 test, so the level counts as DENSE with res >= 258
# on a table of 2^17 rows - its corner indices leave the level and are pinned to the table's last row
PINNED = dict(kind="resolutions", resolutions=[4, 8, 65536, 16], bitwidth=17)
ONE = dict(kind="resolutions", resolutions=[16], bitwidth=12)                               # one level alone: lod_idx 0 zeroes it
SHAPES = {"nerf_hash": (NERF_HASH, True), "small": (SMALL, True), "wrap": (WRAP, True), "narrow": (NARROW, True),
          "pinned": (PINNED, True), "one_level": (ONE, True), "no_bias": (SMALL, False)}
COUNTS = (1, 31, 32, 33, 63, 64, 65, 1000)                                                  # tile and half-tile edges, several tiles


def make_nef(level, spec, bias=True, hidden=64, multiscale='cat', device=DEV, seed=0):
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(seed)
    blas = OctreeAS.make_dense(level)
    if spec["kind"] == "geometric":
        grid = HashGrid.from_geometric(blas, feature_dim=2, num_lods=spec["num_lods"], multiscale_type=multiscale, feature_std=0.1,
                                       codebook_bitwidth=spec["bitwidth"], min_grid_res=spec["min_res"], max_grid_res=spec["max_res"])
    else:
        grid = HashGrid.from_resolutions(blas, feature_dim=2, resolutions=spec["resolutions"], multiscale_type=multiscale,
                                         feature_std=0.1, codebook_bitwidth=spec["bitwidth"])
    nef = NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=hidden, num_layers=1, bias=bias,
                              prune_density_decay=0.95, prune_min_density=0.5).to(device)
    with torch.no_grad():
        for n, p in nef.named_parameters():
            if 'decoder' in n:
                p.mul_(2.0)            # wider activations so relu masks and the sigmoid are exercised
        if not bias:
            nef.decoder_density.lout.weight[0].abs_()          # (without the output bias most density logits are negative)
    return nef


@functools.lru_cache(maxsize=None)
def field(name):
    """one field per shape for the whole file; nothing changes it"""
    spec, bias = SHAPES[name]
    return make_nef(2, spec, bias=bias)


def positions(n, seed):
    """n positions: uniform in the cube, and - as far as n allows - the corners -1 and +1, points on cell faces of resolutions 4,
    16 and 64, and points outside the cube (the lookup clamps them)"""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(n, 3, generator=g) * 2.0 - 1.0
    special = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, 0.25], [1.3, -1.7, 0.2], [-2.0, 0.0, 5.0],
                            [0.5, -0.5, 0.25], [2.0 * 3 / 16 - 1.0, 2.0 * 7 / 16 - 1.0, 2.0 * 15 / 16 - 1.0], [0.0, 0.0, 0.0],
                            [2.0 * 63 / 64 - 1.0, 2.0 * 1 / 64 - 1.0, 0.3], [1.0, -1.0, 1.0]])
    k = min(n, special.shape[0])
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
    """counts the launches of the fused query"""
    import wisp._C as C
    calls = []
    inner = C.nerf_query

    def spy(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)
    monkeypatch.setattr(C, "nerf_query", spy)
    monkeypatch.delenv("WISP_NERF_QUERY_FUSED", raising=False)
    return calls


# ------------------------------------------------------------------------------------------------ the query
@pytest.mark.parametrize("name", list(SHAPES))
def test_query_equals_lookup_plus_decoder(name, count_native):
    """every sample count, the last LOD and a middle one; both outputs, bit for bit"""
    from wisp.ops.nerf_mlp import fused_nerf_query, nerf_query_supported
    nef = field(name)
    L = nef.grid.num_lods
    with torch.no_grad():
        assert nerf_query_supported(nef)
    if name == "pinned":
        assert int(nef.grid.codebook.num_feats[2]) == 2 ** 17
    nonzero = 0
    for n in COUNTS:
        coords, dirs = positions(n, 100 + n)
        for lod_idx in sorted({None, L // 2}, key=str):
            want_rgb, want_den = modular(nef, coords, dirs, lod_idx)
            before = len(count_native)
            with torch.no_grad():
                rgb, den = fused_nerf_query(nef, coords, ray_d=dirs, lod_idx=lod_idx)
            assert len(count_native) == before + 1
            assert rgb.shape == (n, 3) and den.shape == (n, 1) and rgb.dtype == den.dtype == torch.float32
            assert torch.equal(den, want_den), (name, n, lod_idx, "density")
            assert torch.equal(rgb, want_rgb), (name, n, lod_idx, "rgb")
            nonzero += int((den > 0).sum())
    assert nonzero > 0 and float(rgb.std()) > 0.0


@pytest.mark.parametrize("name", ["nerf_hash", "small"])
@pytest.mark.parametrize("R", [1, 37])
def test_ray_directions_through_the_ray_index(name, R, count_native):
    """ray_dirs + ridx against per-sample dirs = ray_dirs.index_select(0, ridx): repeated and unsorted indices"""
    from wisp.ops.nerf_mlp import fused_nerf_query
    nef = field(name)
    g = torch.Generator().manual_seed(R)
    for n in (1, 33, 65, 1000):
        coords, _ = positions(n, 200 + n)
        ray_dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=1).to(DEV)
        ridx = torch.randint(0, R, (n,), generator=g).to(DEV)
        if R > 1 and n > 2:
            ridx[0], ridx[1], ridx[2] = R - 1, 0, R - 1                              # unsorted and repeated, whatever was drawn
            assert not bool((ridx[1:] >= ridx[:-1]).all()) and ridx.unique().numel() < n
        per_sample = ray_dirs.index_select(0, ridx)
        with torch.no_grad():
            a = fused_nerf_query(nef, coords, ray_dirs=ray_dirs, ridx=ridx)
            b = fused_nerf_query(nef, coords, ray_d=per_sample)
        want = modular(nef, coords, per_sample)
        for x, y, z in zip(a, b, want):
            assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("name", ["nerf_hash", "narrow", "no_bias"])
def test_density_alone_guards_and_repeatability(name):
    """want_rgb=False against the density of the full call; all outputs inside NaN-guarded buffers whose guard rows (in front of
    the first sample and behind the last) stay NaN; two runs give the same bits"""
    from wisp.ops.nerf_mlp import fused_nerf_query
    nef = field(name)
    for n in COUNTS:
        coords, dirs = positions(n, 300 + n)
        with torch.no_grad():
            rgb, den = fused_nerf_query(nef, coords, ray_d=dirs)
            none, den_only = fused_nerf_query(nef, coords, want_rgb=False)
            rgb_g, den_g = fused_nerf_query(nef, coords, ray_d=dirs, pad_rows=70)
            none_g, den_only_g = fused_nerf_query(nef, coords, want_rgb=False, pad_rows=70)
            rgb2, den2 = fused_nerf_query(nef, coords, ray_d=dirs)
        assert none is None and none_g is None and torch.equal(den_only, den)
        assert torch.equal(rgb2, rgb) and torch.equal(den2, den)
        assert rgb_g.shape == (n + 140, 3) and den_g.shape == (n + 140, 1)
        for guarded, plain in ((rgb_g, rgb), (den_g, den), (den_only_g, den)):
            assert bool(torch.isnan(guarded[:70]).all()) and bool(torch.isnan(guarded[70 + n:]).all())
            assert torch.equal(guarded[70:70 + n], plain) and not bool(torch.isnan(plain).any())


def test_against_the_cpu_oracle():
    """the one check against something other than the package: oracle/ (float32 torch on the CPU, the reference's arithmetic
    restated) on the SMALL field, colours within the project's fp32 parity bound of 1e-4 (smoke(), tests/test_gpu_0_parity.py)"""
    from oracle import nerf as onerf
    from wisp.ops.nerf_mlp import fused_nerf_query
    nef = field("small")
    grid = nef.grid
    onef = onerf.OracleNeRF(grid.resolutions, 2, grid.codebook_bitwidth, 'cat', 0.1, 64, 1, True, 4)
    sd = {k: v.detach().cpu() for k, v in nef.state_dict().items() if k in onef.state_dict()}
    assert any("codebook" in k for k in sd) and any("decoder_color" in k for k in sd)
    onef.load_state_dict(sd, strict=False)
    g = torch.Generator().manual_seed(9)
    coords = torch.rand(1000, 3, generator=g) * 1.98 - 0.99
    dirs = torch.nn.functional.normalize(torch.randn(1000, 3, generator=g), dim=1)
    with torch.no_grad():
        want = onef.rgba(coords, dirs)
        rgb, den = fused_nerf_query(nef, coords.to(DEV), ray_d=dirs.to(DEV))
    margin("nerf_query rgb vs oracle (SMALL)", float((rgb.cpu() - want["rgb"]).abs().max()), 1e-4)
    scale = max(float(want["density"].abs().max()), 1.0)
    margin("nerf_query density vs oracle (SMALL), relative to the largest", float((den.cpu() - want["density"]).abs().max()) / scale, 1e-4)
    assert float(want["density"].max()) > 0.0


# ------------------------------------------------------------------------------------------------ the tracer
def _rays(n, seed, miss=False):
    from wisp.core import Rays
    o, d = make_rays(max(n, 1), seed)
    o, d = o[:n], d[:n]
    if miss:
        d = -d                                                  # away from the cube
    return Rays(cuda(o), cuda(d), dist_min=1.0, dist_max=5.0)


def _trace(nef, rays, march, channels, fused, steps=24):
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


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("march", ["ray", "voxel"])
@pytest.mark.parametrize("n", [1, 33, 700])
def test_tracer_with_fused_query_equals_the_tracer_without(n, march, depth, count_native):
    nef = field("small")
    channels = ["rgb", "alpha", "hit"] + (["depth"] if depth else [])
    steps = 24 if march == "ray" else 3
    rays = _rays(n, 500 + n)
    off, s_off = _trace(nef, rays, march, channels, None, steps)
    assert len(count_native) == 0
    on, s_on = _trace(nef, rays, march, channels, True, steps)
    assert len(count_native) == 1 and s_on == s_off and (s_on > 0 or n == 1)
    _same_buffers(on, off, channels)
    if n > 1:
        assert bool(on.hit.any()) and float(on.rgb.std()) > 0.0


def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:                                                          # noqa: BLE001
        return ("raised", type(e).__name__, str(e)[:120])


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("march", ["ray", "voxel"])
def test_tracer_on_an_all_miss_batch_and_an_empty_batch(march, depth, count_native):
    """no sample at all: the fused query is called with n = 0 and launches nothing, and the tracer ends as it does without it -
    the background everywhere; with `depth` requested today's compositing refuses a batch without samples (its depth input is
    an empty tensor), and so does the tracer with fused_query on, with the same error"""
    nef = field("small")
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


@pytest.mark.parametrize("case", ["grad", "extra_channel", "autocast", "bf16_compute", "sum_grid", "switch"])
def test_calls_that_stay_modular(case, count_native, monkeypatch):
    """fused_query = True changes nothing for these: no launch of the fused query, and the buffers of the same tracer without it"""
    from wisp.tracers import PackedRFTracer
    nef = make_nef(2, SMALL, multiscale='sum') if case == "sum_grid" else make_nef(2, SMALL)
    if case == "bf16_compute":
        nef.decoder_compute = 'bf16'
    if case == "switch":
        monkeypatch.setenv("WISP_NERF_QUERY_FUSED", "0")
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


# ------------------------------------------------------------------------------------------------ the evaluation surface
def test_evaluate_metrics_on_two_views(tmp_path, count_native, monkeypatch):
    """PSNR equal to evaluate_psnr's; the PNGs of a fused and of a modular evaluation are the same bytes"""
    from gpu_helpers import _dropin_trainer
    from wisp.datasets import MultiviewTensorDataset
    from wisp.models import Pipeline
    from wisp.ops.image import read_png
    from wisp.tracers import PackedRFTracer
    from wisp.trainers.validation import evaluate_psnr
    nef = make_nef(3, SMALL)
    pipe = Pipeline(nef, PackedRFTracer(raymarch_type='ray', num_steps=32, bg_color=(0.0, 0.0, 0.0)))
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
        monkeypatch.setenv("WISP_NERF_QUERY_FUSED", "1" if mode == "fused" else "0")
        trainer.tracker.log_dir = str(tmp_path / mode)
        trainer.return_dict = {}
        before = len(count_native)
        torch.manual_seed(3)
        got = trainer.validate()
        assert (len(count_native) > before) == (mode == "fused")
        assert not hasattr(pipe.tracer, "fused_query")
        names = sorted(os.listdir(tmp_path / mode / "val"))
        assert names == ["0-lod5.png", "1-lod5.png"]
        files[mode] = [open(tmp_path / mode / "val" / f, "rb").read() for f in names]
        assert read_png(str(tmp_path / mode / "val" / names[0])).shape == (32, 32, 3)
        torch.manual_seed(3)
        rays = ds.data["rays"]
        mean, _ = evaluate_psnr(pipe, [(rays[i], gts[i]) for i in range(2)])
        assert float(got["psnr"]) == float(mean), (mode, got, mean)
    assert files["fused"] == files["modular"]
    assert len(np.unique(np.frombuffer(files["fused"][0], np.uint8))) > 16


def test_render_script_end_to_end(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_nerf.py"), "--write-synlego", str(tmp_path / "scene"),
                          "--steps", "40", "--train-views", "4", "--train-res", "32", "--num-steps", "128", "--views", "2",
                          "--res", "32", "32", "--render-batch", "500", "--out", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["frames"] == 2 and rec["fused_query"] is True and rec["ms_per_frame"] > 0 and rec["samples_per_frame"] > 0
    assert rec["field"]["num_lods"] == 16 and rec["field"]["hidden_dim"] == 64
    from wisp.ops.image import read_png
    for k in range(2):
        for kind, ch in (("rgb", 3), ("depth", 3), ("alpha", 1)):
            img = read_png(str(tmp_path / "out" / f"{kind}_{k:03d}.png"))
            assert img.shape == (32, 32, ch) and img.dtype == np.uint8, (kind, img.shape)
