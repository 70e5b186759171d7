"""GPU: the fused density query of the prune (csrc/prune_query.hip, NeuralRadianceField._prune_fused) against the modular path
(position arithmetic in torch, hashgrid_interpolate on the fp32 table, the exact-fp32 decoder, maximum, >).  The contract is
equality of bits: torch.equal on the occupancy and on every tensor of the rebuilt octree, for two successive prunes per shape
(so that a non-zero previous occupancy and the decay take part), on tables drawn at std 0.1 with the threshold at the median
density of the first prune (cells are kept and cells are dropped)."""
import copy

import numpy as np
import pytest
import torch

from gpu_helpers import DEV, cuda, make_rays, _build_pair

pytestmark = pytest.mark.gpu

NERF_HASH = dict(kind="geometric", num_lods=16, bitwidth=19, min_res=16, max_res=512)       # nerf_hash.yaml: 15 of 16 levels live
SMALL = dict(kind="geometric", num_lods=6, bitwidth=12, min_res=4, max_res=64)              # in_dim 12: dense and hashed levels
WRAP = dict(kind="geometric", num_lods=16, bitwidth=10, min_res=16, max_res=512)            # 2^10 rows: every level is hashed and wraps
NARROW = dict(kind="geometric", num_lods=4, bitwidth=12, min_res=8, max_res=64)             # in_dim 8, 3 live levels
# res 65536 at bitwidth 17: res^2 and res^3 wrap to 0 in the reference's int32 test, so the level counts as DENSE with res >= 258
# on a table of 2^17 rows - its corner indices leave the level and are pinned to the table's last row
PINNED = dict(kind="resolutions", resolutions=[4, 8, 65536, 16], bitwidth=17)


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
    assert grid.dense_points.shape[0] == 8 ** level
    if not bias:
        # without the output bias (1.0 at construction) the density logit is negative for most cells and relu leaves a handful of
        # positive densities; a non-negative output row makes it positive wherever a hidden unit is active
        with torch.no_grad():
            nef.decoder_density.lout.weight[0].abs_()
    return nef


def draws(cells, seed, device=DEV):
    g = torch.Generator().manual_seed(seed)
    unit = torch.rand(cells, 3, generator=g)
    views = torch.nn.functional.normalize(torch.randn(cells, 3, generator=g), dim=1)
    return unit.to(device), views.to(device)


def modular_density(nef, unit):
    """the density the modular path computes for these draws (a plain forward query: nothing is pruned)"""
    pts = nef.grid.dense_points.to(unit.device)
    samples = ((pts.float() + unit) / (2.0 ** nef.grid.blas.max_level)) * 2.0 - 1.0
    views = torch.zeros_like(samples)
    views[:, 2] = 1.0
    with torch.no_grad():
        return nef.forward(coords=samples, ray_d=views, channels="density")[:, 0].float(), samples


def median_threshold(nef, unit):
    d, _ = modular_density(nef, unit)
    thr = float(d.median())
    frac = float((d > thr).float().mean())
    assert 0.1 < frac < 0.9 or d.numel() <= 8, frac              # densities straddle the threshold
    return thr


@pytest.fixture
def count_native(monkeypatch):
    """counts the launches of the fused query"""
    import wisp._C as C
    calls = []
    inner = C.nerf_prune_query

    def spy(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)
    monkeypatch.setattr(C, "nerf_prune_query", spy)
    return calls


def prune_with(nef, fused, unit, views, monkeypatch):
    monkeypatch.setenv("WISP_PRUNE_FUSED", "1" if fused else "0")
    nef.prune(unit_samples=unit, view_dirs=views)


def assert_same_state(a, b):
    assert torch.equal(a.grid.occupancy, b.grid.occupancy)
    for name in ("octree", "points", "pyramid", "prefix"):
        x, y = getattr(a.grid.blas, name), getattr(b.grid.blas, name)
        assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()), name
    assert a.grid.blas.max_level == b.grid.blas.max_level


def two_prunes_equal(nef, monkeypatch, count_native, seed=3):
    cells = nef.grid.dense_points.shape[0]
    u1, v1 = draws(cells, seed)
    u2, v2 = draws(cells, seed + 1)
    nef.prune_min_density = median_threshold(nef, u1)
    ref = copy.deepcopy(nef)
    monkeypatch.setenv("WISP_PRUNE_FUSED", "1")
    assert nef.prune_fused()
    for k, (u, v) in enumerate(((u1, v1), (u2, v2))):
        prune_with(ref, False, u, v, monkeypatch)
        assert len(count_native) == k
        prune_with(nef, True, u, v, monkeypatch)
        assert len(count_native) == k + 1                       # the fused path ran, and only for `nef`
        assert_same_state(nef, ref)
        kept = int(nef.grid.blas.pyramid[0, nef.grid.blas.max_level])
        assert 0 < kept < cells or cells <= 8, kept
    assert float(nef.grid.occupancy.max()) > 0.0
    return nef, ref


@pytest.mark.parametrize("level", [1, 2, 3, 5])
def test_fused_prune_equals_modular_on_small_levels(level, monkeypatch, count_native):
    """dense levels 1 (8 cells: one partial tile), 2 (one full tile), 3 (one workgroup), 5 (several workgroups)"""
    two_prunes_equal(make_nef(level, SMALL), monkeypatch, count_native)


def test_fused_prune_equals_modular_over_several_rounds_of_the_persistent_loop(monkeypatch, count_native):
    """level 6: 262 144 cells = 4096 wave tiles, more than the 8 waves of every workgroup of a full grid take in one round"""
    two_prunes_equal(make_nef(6, SMALL), monkeypatch, count_native)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name,spec,level", [("nerf_hash", NERF_HASH, 4), ("wrap", WRAP, 3), ("narrow", NARROW, 3),
                                             ("pinned", PINNED, 3)])
def test_fused_prune_equals_modular_on_the_grid_shapes(name, spec, level, bias, monkeypatch, count_native):
    nef = make_nef(level, spec, bias=bias)
    grid = nef.grid
    if name == "nerf_hash":
        assert grid.num_lods == 16 and grid.codebook_bitwidth == 19 and nef.effective_feature_dim() == 32
    if name == "wrap":
        assert all(int(r) ** 3 >= 2 ** 10 for r in grid.resolutions)
    if name == "narrow":
        assert nef.effective_feature_dim() == 8
    if name == "pinned":
        assert int(grid.codebook.num_feats[2]) == 2 ** 17 and 65536 >= 258
    two_prunes_equal(nef, monkeypatch, count_native)


@pytest.mark.parametrize("name,spec,level", [("nerf_hash", NERF_HASH, 5), ("narrow", NARROW, 3), ("pinned", PINNED, 2)])
def test_lookup_half_and_decoder_half_separately(name, spec, level):
    """wisp_nerf_prune_query_debug writes the decoder's input tile and the density: the first against hashgrid_interpolate on the
    positions torch computes, the second against the density of the exact-fp32 decoder on THOSE features - a mismatch names its half"""
    import wisp._C as C
    from wisp.ops.nerf_mlp import fused_prune_query, _decoder_tensors, _flat_view, _pack
    nef = make_nef(level, spec)
    grid = nef.grid
    cells = grid.dense_points.shape[0]
    unit, views = draws(cells, 11)
    grid.occupancy = torch.zeros(cells, device=DEV)
    grid.dense_points = grid.dense_points.to(DEV)
    occ, keep, feats, density = fused_prune_query(nef, unit, debug=True)
    samples = ((grid.dense_points.float() + unit) / (2.0 ** grid.blas.max_level)) * 2.0 - 1.0
    cb = grid.codebook
    res = [int(r) for r in cb.resolutions.reshape(-1).tolist()]
    want_feats = C.hashgrid_interpolate(samples, cb.feats.detach(), cb.begin_idxes, res, grid.codebook_bitwidth,
                                        (grid.num_lods - 1) * grid.feature_dim)
    assert feats.shape == want_feats.shape and torch.equal(feats, want_feats), "lookup half"
    assert int((feats != 0).sum()) > cells
    I, H = nef.effective_feature_dim(), 64
    shapes = ((H, I), (H,), (16, H), (16,), (H, 42), (H,), (H, H), (H,), (3, H), (3,))
    prm = _decoder_tensors(nef)
    packed = _flat_view([p.detach() for p in prm]) if all(p is not None for p in prm) else None
    packed = packed if packed is not None else _pack(prm, shapes)
    _, want_density = C.nerf_mlp_forward(want_feats, views, packed, I, H, 4, False)
    assert torch.equal(density, want_density[:, 0]), "decoder half"
    assert float(density.max()) > 0.0 and torch.equal(occ, density) and torch.equal(keep, density > nef.prune_min_density)


def _preimage(target, decay):
    """a float32 x with fl32(x * decay) == target"""
    x = np.float32(target) / np.float32(decay)
    for _ in range(8):
        for cand in (x, np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(2))):
            if np.float32(cand) * np.float32(decay) == np.float32(target):
                return np.float32(cand)
        x = np.nextafter(x, np.float32(0))
    raise AssertionError(f"no float32 pre-image of {target} under x * {decay}")


def test_threshold_is_compared_in_float32(monkeypatch, count_native):
    """density 0 everywhere (zero row 0 of layer 2 and its bias), so the new occupancy is fl32(occ_in * decay): entries that land
    exactly on float32(min_density), one ulp below and one ulp above.  min_density itself (0.3) is not a float32."""
    nef = make_nef(2, SMALL)
    with torch.no_grad():
        nef.decoder_density.lout.weight[0].zero_()
        nef.decoder_density.lout.bias[0] = 0.0
    cells = 64
    decay = np.float32(0.95)
    nef.prune_min_density = 0.3
    t = np.float32(0.3)
    targets = [t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))]
    occ0 = np.random.default_rng(5).uniform(0.0, 0.6, cells).astype(np.float32)
    for k, tg in enumerate(targets):
        occ0[k] = occ0[32 + k] = _preimage(tg, decay)
    unit, views = draws(cells, 13)
    ref = copy.deepcopy(nef)
    nef.grid.occupancy = torch.from_numpy(occ0).to(DEV)
    ref.grid.occupancy = torch.from_numpy(occ0).to(DEV)
    prune_with(ref, False, unit, views, monkeypatch)
    prune_with(nef, True, unit, views, monkeypatch)
    assert len(count_native) == 1
    assert_same_state(nef, ref)
    got = nef.grid.occupancy.cpu().numpy()
    assert [got[k] for k in range(3)] == targets and [got[32 + k] for k in range(3)] == targets
    assert np.array_equal(got, occ0 * decay)                                        # density 0: the decayed occupancy survives
    keep = torch.from_numpy(got > t)
    assert keep[:3].tolist() == [False, False, True]
    from wisp.accelstructs import OctreeAS
    assert torch.equal(nef.grid.blas.octree.cpu(), OctreeAS.from_leaf_mask(keep.to(DEV), 2).octree.cpu())


@pytest.mark.parametrize("level", [1, 3])
def test_rows_behind_the_last_cell_are_left_alone(level):
    from wisp.ops.nerf_mlp import fused_prune_query
    nef = make_nef(level, SMALL)
    cells = 8 ** level
    unit, _ = draws(cells, 17)
    nef.grid.occupancy = torch.rand(cells, device=DEV)
    nef.grid.dense_points = nef.grid.dense_points.to(DEV)
    occ, keep = fused_prune_query(nef, unit, pad_rows=200)
    plain_occ, plain_keep = fused_prune_query(nef, unit)
    assert occ.shape == (cells + 200,) and keep.shape == (cells + 200,)
    assert bool(torch.isnan(occ[cells:]).all()) and bool((keep[cells:] == 255).all())
    assert torch.equal(occ[:cells], plain_occ) and torch.equal(keep[:cells].bool(), plain_keep)
    assert not bool(torch.isnan(occ[:cells]).any()) and int(keep[:cells].max()) <= 1


def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:                                                          # noqa: BLE001
        return ("raised", type(e).__name__, str(e)[:80])


@pytest.mark.parametrize("case", ["sum", "hidden128", "cpu", "not_dense"])
def test_other_shapes_keep_the_modular_path(case, monkeypatch, count_native):
    """'sum' grids, hidden 128, a model on the CPU and dense_points that are not every cell of the level (the 1 241-cell case of
    test_prune_rebuilds_identical_octree) take the present code whatever the switch says, with the results it gives today"""
    if case == "sum":
        nef = make_nef(3, SMALL, multiscale='sum')
    elif case == "hidden128":
        nef = make_nef(3, SMALL, hidden=128)
    elif case == "cpu":
        nef = make_nef(2, SMALL, device="cpu")
    else:
        nef, _, _ = _build_pair(level=4, dense=False)
        assert nef.grid.dense_points.shape[0] == 1241
    dev = "cpu" if case == "cpu" else DEV
    cells = nef.grid.dense_points.shape[0]
    unit, views = draws(cells, 19, device=dev)
    monkeypatch.setenv("WISP_PRUNE_FUSED", "1")
    assert not nef.prune_fused()
    ref = copy.deepcopy(nef)

    def run(model, fused):
        prune_with(model, fused, unit, views, monkeypatch)
        return model.grid.occupancy.clone(), model.grid.blas.octree.clone()
    a, b = _outcome(lambda: run(nef, True)), _outcome(lambda: run(ref, False))
    assert len(count_native) == 0
    assert a[0] == b[0]
    if a[0] == "ok":
        assert torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1].cpu(), b[1][1].cpu())
        assert float(a[1][0].max()) > 0.0
    else:
        assert a[1:] == b[1:] and case == "cpu"                                     # (the hot path has no CPU fallback: today's refusal)


# ------------------------------------------------------------------------------------------------ trainer level
def _steps(tr, batches, gts, steps, seed):
    from wisp.core import Rays
    torch.manual_seed(seed)                                   # the jitter seeds follow torch's CPU generator (OctreeAS._draw_seed)
    rays = [Rays(cuda(o), cuda(d), dist_min=1.0, dist_max=5.0) for o, d in batches]
    losses, counts = [], []
    for i in range(steps):
        nxt = rays[(i + 1) % len(rays)] if i + 1 < steps else None
        loss, S = tr.step(rays[i % len(rays)], gts[i % len(rays)], prefetch=nxt)
        losses.append(loss.clone())
        counts.append(S)
    tr.wait_for_parameters()
    torch.cuda.synchronize()
    return [float(l) for l in losses], counts


def _close(l1, l2, rel=1e-5):
    return len(l1) == len(l2) and all(abs(a - b) <= rel * max(1.0, abs(b)) for a, b in zip(l1, l2))


def test_trainer_prunes_to_the_same_octree_and_leaves_the_generator_where_it_was(monkeypatch, count_native):
    """Three MultiviewTrainSteps from the same seed - one fused, two with the switch off - run 3 steps, the prune of the 4th step's
    pre_step (prune_every = 3) and 3 steps more, at 3000 rays.  The steps are not order-free (float atomics on the coarse levels), so
    the tables of two runs differ in their last bits after three steps: the threshold is put into the widest gap of the central
    half of the densities the prune is about to see (as test_prune_rebuilds_identical_octree does), then the octrees must be
    equal byte for byte, the prune generators in the same state, and the losses after the prune as close as the suite asks of
    two runs of the same step (1e-5, test_native_step_equals_the_python_issued_step) - for fused against off AND off against off."""
    from wisp.models import Pipeline
    from wisp.tracers import PackedRFTracer
    from wisp.trainers import MultiviewTrainStep
    nef0, _, _ = _build_pair(level=4, lods=16, dense=True)
    trainers = []
    for fused in (True, False, False):
        tr = MultiviewTrainStep(Pipeline(copy.deepcopy(nef0), PackedRFTracer(raymarch_type='ray', num_steps=96, bg_color=(0, 0, 0))),
                                prune_every=3, enable_amp=True, target_sample_size=2 ** 17, seed=7)
        trainers.append((tr, fused))
    rng = np.random.default_rng(411)
    batches = [make_rays(3000, 412 + k) for k in range(2)]
    gts = [cuda(rng.uniform(size=(3000, 3)).astype(np.float32)) for _ in range(2)]
    for tr, fused in trainers:
        monkeypatch.setenv("WISP_PRUNE_FUSED", "1" if fused else "0")
        _steps(tr, batches, gts, 3, seed=91)
    assert len(count_native) == 0
    # the draws the prune will make, from a copy of the generator; the threshold into the widest central gap of those densities
    tr_ref = trainers[1][0]
    g = torch.Generator(device=tr_ref._prune_gen.device)
    g.set_state(tr_ref._prune_gen.get_state())
    unit = torch.rand(4096, 3, generator=g, device=g.device)
    monkeypatch.setenv("WISP_PRUNE_FUSED", "0")
    d, _ = modular_density(tr_ref.pipeline.nef, unit)
    srt = np.sort(d.cpu().numpy().astype(np.float64))
    gaps = srt[1025:3073] - srt[1024:3072]
    j = int(np.argmax(gaps))
    assert gaps[j] > 1e-5, gaps[j]                           # far wider than the last-bit differences between two runs
    thr = float(0.5 * (srt[1024 + j] + srt[1025 + j]))
    out = []
    for tr, fused in trainers:
        tr.pipeline.nef.prune_min_density = thr
        monkeypatch.setenv("WISP_PRUNE_FUSED", "1" if fused else "0")
        assert tr.pipeline.nef.prune_fused() == fused
        out.append(_steps(tr, batches, gts, 3, seed=92))
    assert len(count_native) == 1                            # one prune, fused for the first trainer only
    (tf, _), (t1, _), (t2, _) = trainers
    for other in (t1, t2):
        assert_same_state_blas(tf, other)
        assert torch.equal(tf._prune_gen.get_state(), other._prune_gen.get_state())
    kept = int(tf.pipeline.nef.grid.blas.pyramid[0, 4])
    assert 1024 <= kept <= 3072, kept
    (lf, cf), (l1, c1), (l2, c2) = out
    print("losses after the prune: fused", lf, "off", l1, "off again", l2)
    assert cf == c1 == c2
    assert _close(l1, l2), (l1, l2)
    assert _close(lf, l1), (lf, l1)


def assert_same_state_blas(ta, tb):
    a, b = ta.pipeline.nef.grid.blas, tb.pipeline.nef.grid.blas
    for name in ("octree", "points", "pyramid", "prefix"):
        assert torch.equal(getattr(a, name).cpu(), getattr(b, name).cpu()), name
