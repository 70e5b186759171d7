"""GPU: the fused textured SDF step (wisp_sdf_tex_train_step, csrc/spc_grad.hip), SDFTrainStep over a NeuralSDFTex (eager and
graph-captured) and the fused marching of a NeuralSDFTex - against the CPU oracle, against the modular launches, against
torch.optim.Adam, against the one-output step (bit for bit) and end to end through scripts/train_sdf_tex.py --fused-step."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_helpers import DEV, _assert_same_adam_trajectory, cuda, make_rays, margin, snapshot_first_grad
from oracle import nerf as onerf, spc as ospc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tex_field(blas, pos, lods=4, hidden=128, seed=7, std=0.05, half=None):
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDFTex
    torch.manual_seed(seed)
    grid = OctreeGrid(blas, feature_dim=16, num_lods=lods, multiscale_type='sum', feature_std=std)
    if half is not None:
        grid.half_features = half
    return NeuralSDFTex(grid, embedder_type='identity' if pos else 'none', hidden_dim=hidden, num_layers=1).to(DEV)


def _random_cells(seed):
    from wisp.accelstructs import OctreeAS
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 32, size=(4000, 3))
    return rng, P, OctreeAS.from_quantized_points(cuda(P.astype(np.int16)), 5)


# ------------------------------------------------------------------------------------------------ 1. the CPU oracle
@pytest.fixture(scope="module")
def shell():
    """level-5 shell octree |r - 0.55| < 0.12 with its oracle twin and trinkets (built once)"""
    from wisp.accelstructs import OctreeAS
    idx = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing='ij'), -1).reshape(-1, 3)
    ctr = (idx + 0.5) / 16 - 1
    keep = np.abs(np.linalg.norm(ctr, axis=1) - 0.55) < 0.12
    P = idx[keep]
    blas = OctreeAS.from_quantized_points(torch.from_numpy(P).short().to(DEV), 5)
    oblas = onerf.OracleBLAS(ospc.points_to_octree(P, 5))
    pd, pyd = ospc.make_dual(oblas.points, oblas.pyramid)
    tr, _ = ospc.make_trinkets(oblas.points, oblas.pyramid, pd, pyd)
    return dict(P=P, ctr=ctr[keep], blas=blas, oblas=oblas, tr=tr)


@pytest.mark.parametrize("B,lods,H,pos", [(700, 3, 128, True), (1, 1, 16, False), (37, 3, 24, False), (6, 1, 16, True)])
def test_fused_textured_step_matches_the_cpu_oracle(shell, B, lods, H, pos):
    """wisp_sdf_tex_train_step against autograd through the CPU oracle: oracle.octree_grid.octree_grid_interpolate ('sum', the
    reference's fp16 rounding) -> [position, features] or the features alone -> Linear -> relu -> Linear(H, 4) -> sigmoid on the
    first three -> (sum (rgb - rgb_gt)^2 + sum (sdf - gt)^2) / B: the loss, the two un-normalised sums and every gradient.
    (37 coordinates over 3 levels: 5 samples per pass with an idle lane group; 24 hidden units: no multiple of 16.)
    The tolerances here scale with a tensor's largest entry; element-wise correctness is owned by tests/test_gpu_sdf_step_exact.py."""
    from oracle import octree_grid as og
    from wisp.trainers import SDFTrainStep
    nef = _tex_field(shell["blas"], pos, lods=lods, hidden=H, seed=13)
    grid = nef.grid
    P, ctr = shell["P"], shell["ctr"]
    rng = np.random.default_rng(222 + B)
    c = (ctr[rng.integers(0, P.shape[0], B)] + rng.uniform(-0.02, 0.02, (B, 3))).astype(np.float32)
    c[::13] = rng.uniform(-1.1, 1.1, (c[::13].shape[0], 3))                       # some outside every cell / the unit cube
    gt = rng.normal(size=(B, 1)).astype(np.float32) * 0.1
    col = rng.uniform(size=(B, 3)).astype(np.float32)
    in_dim = (3 if pos else 0) + 16
    feats_cpu = [f.detach().cpu().clone().requires_grad_(True) for f in grid.features]
    dec = onerf.OracleDecoder(in_dim, 4, H, 1, True)
    dec.load_state_dict({k: v.detach().cpu() for k, v in nef.decoder.state_dict().items()})
    f = og.octree_grid_interpolate(shell["oblas"], shell["tr"], feats_cpu, torch.from_numpy(c), lods - 1, grid.base_lod, grid.active_lods,
                                   'sum', 16, True)
    y = dec(torch.cat([torch.from_numpy(c), f], -1) if pos else f)
    want_rgb = ((torch.sigmoid(y[:, :3]) - torch.from_numpy(col)) ** 2).sum()
    want_l2 = ((y[:, 3:4] - torch.from_numpy(gt)) ** 2).sum()
    want_loss = (want_rgb + want_l2) / B
    want_loss.backward()
    want_loss, want_l2, want_rgb = want_loss.detach(), want_l2.detach(), want_rgb.detach()
    step = SDFTrainStep(nef, lr=1e-3, eps=1e-15)
    assert step._fused_field() is not None and step._fused_field()["pos"] == int(pos)
    loss = step._forward_backward(cuda(c), cuda(gt), cuda(col))
    tag = f"B={B} lods={lods} H={H} pos={int(pos)}"
    for name, got, want in (("loss", loss, want_loss), ("l2 sum", step.last_l2, want_l2), ("rgb sum", step.last_rgb, want_rgb)):
        margin(f"tex step vs oracle {name} {tag}", abs(float(got) - float(want)), 2e-5 * max(1.0, abs(float(want))))
    for i in range(lods):
        g1, g2 = grid.features[i].grad.cpu().numpy(), feats_cpu[i].grad.numpy()
        assert np.abs(g2).max() > 0 or B == 1
        margin(f"tex step vs oracle features[{i}] {tag}", float(np.max(np.abs(g1 - g2) - 2e-3 * np.abs(g2))), 2e-5)
        np.testing.assert_allclose(g1, g2, rtol=2e-3, atol=2e-5)
    for (n1, p1), (n2, p2) in zip(nef.decoder.named_parameters(), dec.named_parameters()):
        sc = float(p2.grad.abs().max())
        margin(f"tex step vs oracle {n1} {tag}", float((p1.grad.cpu() - p2.grad).abs().max()), 2e-4 * sc + 1e-7)


# ------------------------------------------------------------------------------------------------ 2. fused against modular
@pytest.mark.parametrize("batch,pos,lods,half", [(512, True, 4, True), (512, False, 4, None), (37, True, 4, None), (37, False, 4, None),
                                                 (5000, True, 4, None), (5000, False, 4, None), (512, True, 5, None),
                                                 (512, False, 4, False)])
def test_fused_textured_step_equals_the_modular_launches_and_repeats_bitwise(batch, pos, lods, half, monkeypatch):
    """SDFTrainStep's fused textured step against the modular one it replaces (query, multi-level lookup, torch Linear modules,
    sigmoid, torch loss, their backward passes) from the same parameters: same loss, same gradient in every parameter - and the
    same bits when run again; then 30 real steps train.
    The 30 steps run at the learning rates the tracer tests fit their fields with (3e-3, grid x 10), not at the 1e-3 / x 2 of the
    comparison above: the colour targets are independent uniform numbers, so the colour term (0.25 of the initial 0.27) falls only
    as fast as the feature tables memorise them, and Adam moves a parameter by at most its learning rate per step.  torch
    autograd + torch.optim.Adam over the CPU oracle on these very inputs end at 0.65 - 0.88 x the first loss after 30 steps of
    1e-3 / x 2 (0.76 at B = 512 with the position, 0.88 at B = 5000) and at 0.04 - 0.18 x at 3e-3 / x 10: below 0.7 x is a
    statement about the rates, which this test therefore fixes beforehand, not about the kernel
    (tests/test_sdf_tex_step_host.py::test_thirty_adam_steps_on_the_oracle_need_the_higher_rates repeats that study at B = 512).
    half_features is on by default (the first case names it), so the one case that differs is the one with it off."""
    from wisp.trainers import SDFTrainStep
    rng, P, blas = _random_cells(240 + batch)
    nef_a = _tex_field(blas, pos, lods=lods, half=half)
    nef_b = copy.deepcopy(nef_a)
    fused = SDFTrainStep(nef_a, lr=1e-3, eps=1e-15, grid_lr_weight=2.0)
    assert fused._fused_field() is not None
    monkeypatch.setenv("WISP_SDF_TRAIN_FUSED", "0")
    modular = SDFTrainStep(nef_b, lr=1e-3, eps=1e-15, grid_lr_weight=2.0)
    assert modular._fused_field() is None
    inside = ((P[rng.integers(0, P.shape[0], batch)] + rng.uniform(0.02, 0.98, (batch, 3))) / 16 - 1).astype(np.float32)
    inside[::11] = rng.uniform(-1.2, 1.2, (inside[::11].shape[0], 3))                 # some outside every cell / the unit cube
    coords = cuda(inside)
    gts = cuda(rng.normal(size=(batch, 1)).astype(np.float32) * 0.1)
    col = cuda(rng.uniform(size=(batch, 3)).astype(np.float32))
    la = fused._forward_backward(coords, gts, col)
    sums_a = (fused.last_l2.clone(), fused.last_rgb.clone())
    lb = modular._forward_backward(coords, gts, col)
    tag = f"B={batch} pos={int(pos)} lods={lods} half={half}"
    margin(f"fused tex step loss {tag}", abs(float(la) - float(lb)), 1e-5 * max(1.0, abs(float(lb))))
    margin(f"fused tex step l2 sum {tag}", abs(float(sums_a[0]) - float(modular.last_l2)), 1e-5 * max(1.0, abs(float(modular.last_l2))))
    margin(f"fused tex step rgb sum {tag}", abs(float(sums_a[1]) - float(modular.last_rgb)), 1e-5 * max(1.0, abs(float(modular.last_rgb))))
    ga, gb = fused.flat.grad.clone(), modular.flat.grad.clone()
    for (n1, p1), (n2, p2) in zip(nef_a.named_parameters(), nef_b.named_parameters()):
        sc = max(float(p2.grad.abs().max()), 1e-12)
        margin(f"fused tex step grad {n1} {tag}", float((p1.grad - p2.grad).abs().max()), 2e-5 * sc)
    assert float(gb.abs().max()) > 0 and float(ga.abs().max()) > 0
    for _ in range(5):                                        # same inputs, same bits
        fused.flat.grad.zero_()
        l2 = fused._forward_backward(coords, gts, col)
        assert torch.equal(fused.flat.grad, ga) and float(l2) == float(la)
        assert torch.equal(fused.last_l2, sums_a[0]) and torch.equal(fused.last_rgb, sums_a[1])
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED")
    trainer = SDFTrainStep(nef_a, lr=3e-3, eps=1e-15, grid_lr_weight=10.0)
    assert trainer._fused_field() is not None
    losses = [float(trainer.step(coords, gts, col)) for _ in range(30)]
    assert losses[-1] < 0.7 * losses[0], (losses[0], losses[-1])


# ------------------------------------------------------------------------------------------------ 3. torch.optim.Adam
@pytest.mark.parametrize("pos", [True, False])
def test_textured_sdf_train_step_matches_torch_adam(pos, monkeypatch):
    """The textured SDFTrainStep (fused step + Adam over the flat buffer in one launch) against the same field stepped through
    autograd with torch.optim.Adam."""
    from wisp.trainers import SDFTrainStep
    rng, P, blas = _random_cells(140)
    nef = _tex_field(blas, pos, lods=3, seed=5)
    ref = copy.deepcopy(nef)
    groups = [{"params": [p for n, p in ref.named_parameters() if 'decoder' in n], "lr": 1e-3},
              {"params": [p for n, p in ref.named_parameters() if 'decoder' not in n and 'grid' in n], "lr": 2e-3},
              {"params": [p for n, p in ref.named_parameters() if 'decoder' not in n and 'grid' not in n], "lr": 1e-3}]
    opt = torch.optim.Adam([g for g in groups if g["params"]], eps=1e-15)
    tr = SDFTrainStep(nef, lr=1e-3, eps=1e-15, grid_lr_weight=2.0)
    assert tr._fused_field() is not None
    cells = cuda(((P[rng.integers(0, P.shape[0], 512)] + rng.uniform(0.05, 0.95, (512, 3))) / 16 - 1).astype(np.float32))
    gts = cuda(rng.normal(size=(512, 1)).astype(np.float32) * 0.1)
    col = cuda(rng.uniform(size=(512, 3)).astype(np.float32))
    grads = []
    snapshot_first_grad(tr, grads)
    for it in range(4):
        l1 = tr.step(cells, gts, col)
        opt.zero_grad()
        rgb, sdf = ref(coords=cells, lod_idx=2, channels=["rgb", "sdf"])
        l2 = (((rgb - col) ** 2).sum() + ((sdf - gts) ** 2).sum()) / 512
        l2.backward()
        if it == 0:
            flat = grads[0]
            for (n1, p1), (n2, p2) in zip(nef.named_parameters(), ref.named_parameters()):
                off = (p1.grad.data_ptr() - tr.flat.grad.data_ptr()) // 4
                g1 = flat[off:off + p1.numel()].view_as(p1)
                sc = max(float(p2.grad.abs().max()), 1e-12)
                margin(f"tex sdf step grad {n1} pos={int(pos)}", float((g1 - p2.grad).abs().max()), 1e-4 * sc)
        opt.step()
        assert abs(float(l1) - float(l2)) <= 1e-5 * max(1.0, abs(float(l2)))
    for (n1, p1), (n2, p2) in zip(sorted(nef.named_parameters()), sorted(ref.named_parameters())):
        _assert_same_adam_trajectory(p1, p2, n1, steps=4, max_lr=2e-3)


# ------------------------------------------------------------------------------------------------ 4. captured graph
def test_textured_step_from_captured_graph_equals_eager_steps():
    """capture(512) for a NeuralSDFTex: a third static buffer for the colours; replayed steps walk the eager trajectory, another
    batch size falls back to eager issue."""
    from wisp.trainers import SDFTrainStep
    rng, P, blas = _random_cells(141)
    nef_a = _tex_field(blas, True, lods=3, seed=6)
    nef_b = copy.deepcopy(nef_a)
    eager = SDFTrainStep(nef_a, lr=1e-3, eps=1e-15, grid_lr_weight=2.0)
    graph = SDFTrainStep(nef_b, lr=1e-3, eps=1e-15, grid_lr_weight=2.0).capture(512)
    assert eager.static_inputs() is None
    static = graph.static_inputs()
    assert len(static) == 3 and [tuple(t.shape) for t in static] == [(512, 3), (512, 1), (512, 3)]
    assert graph._fused_field() is not None
    before = {n: p.detach().clone() for n, p in nef_b.named_parameters()}
    for n, p in nef_a.named_parameters():                      # capturing (warm-up passes included) moved no parameter
        assert torch.equal(p.detach(), before[n]), n
    for it in range(6):
        cells = cuda(((P[rng.integers(0, P.shape[0], 512)] + rng.uniform(0.05, 0.95, (512, 3))) / 16 - 1).astype(np.float32))
        gts = cuda(rng.normal(size=(512, 1)).astype(np.float32) * 0.1)
        col = cuda(rng.uniform(size=(512, 3)).astype(np.float32))
        la, lb = eager.step(cells, gts, col), graph.step(cells, gts, col)
        assert abs(float(la) - float(lb)) <= 1e-6 * max(1.0, abs(float(la))), it
        assert abs(float(eager.last_l2) - float(graph.last_l2)) <= 1e-6 * max(1.0, abs(float(eager.last_l2)))
        assert abs(float(eager.last_rgb) - float(graph.last_rgb)) <= 1e-6 * max(1.0, abs(float(eager.last_rgb)))
    moved = 0.0
    for (n1, p1), (n2, p2) in zip(sorted(nef_a.named_parameters()), sorted(nef_b.named_parameters())):
        _assert_same_adam_trajectory(p1, p2, n1, steps=6, max_lr=2e-3)
        moved = max(moved, float((p2.detach() - before[n2]).abs().max()))
    assert moved > 1e-3                                        # the replayed steps did train
    cells = cuda(((P[rng.integers(0, P.shape[0], 100)] + 0.5) / 16 - 1).astype(np.float32))
    assert torch.isfinite(graph.step(cells, cuda(np.zeros((100, 1), np.float32)), cuda(np.full((100, 3), 0.5, np.float32))))
    with pytest.raises(ValueError, match="rgb"):
        graph.step(cells, cuda(np.zeros((100, 1), np.float32)))


# ------------------------------------------------------------------------------------------------ 5. the one-output step
@pytest.mark.parametrize("batch", [512, 37])
def test_inert_colour_rows_give_the_one_output_steps_bits(batch):
    """A NeuralSDFTex whose colour rows are inert (W2[0:3] = 0, b2[0:3] = 0, colour target 0.5: sigmoid(0) - 0.5 = 0, so no colour
    gradient reaches the hidden layer) next to a NeuralSDF with the same W1, b1 and w2 = W2[3], b2 = b2[3]: the feature-table
    gradients, dW1 and db1 of the two fused steps are bitwise equal - the shared walk, the lookup and phase 3's order."""
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDF
    from wisp.trainers import SDFTrainStep
    rng, P, blas = _random_cells(250 + batch)
    tex = _tex_field(blas, True, lods=4)
    torch.manual_seed(7)
    grid1 = OctreeGrid(blas, feature_dim=16, num_lods=4, multiscale_type='sum', feature_std=0.05)
    one = NeuralSDF(grid1, pos_embedder='none', position_input=True, hidden_dim=128, num_layers=1).to(DEV)
    with torch.no_grad():
        tex.decoder.lout.weight[:3].zero_()
        tex.decoder.lout.bias[:3].zero_()
        for a, b in zip(one.grid.features, tex.grid.features):
            a.copy_(b)
        one.decoder.layers[0].weight.copy_(tex.decoder.layers[0].weight)
        one.decoder.layers[0].bias.copy_(tex.decoder.layers[0].bias)
        one.decoder.lout.weight.copy_(tex.decoder.lout.weight[3:4])
        one.decoder.lout.bias.copy_(tex.decoder.lout.bias[3:4])
    s_tex, s_one = SDFTrainStep(tex), SDFTrainStep(one)
    assert s_tex._fused_field() is not None and s_one._fused_field() is not None
    inside = ((P[rng.integers(0, P.shape[0], batch)] + rng.uniform(0.02, 0.98, (batch, 3))) / 16 - 1).astype(np.float32)
    inside[::11] = rng.uniform(-1.2, 1.2, (inside[::11].shape[0], 3))
    coords = cuda(inside)
    gts = cuda(rng.normal(size=(batch, 1)).astype(np.float32) * 0.1)
    l_tex = s_tex._forward_backward(coords, gts, torch.full((batch, 3), 0.5, device=DEV))
    l_one = s_one._forward_backward(coords, gts)
    assert float(s_tex.last_rgb) == 0.0 and float(l_tex) == float(l_one)
    for a, b in zip(tex.grid.features, one.grid.features):
        assert float(a.grad.abs().max()) > 0 and torch.equal(a.grad, b.grad)
    for a, b in zip(tex.decoder.layers[0].parameters(), one.decoder.layers[0].parameters()):
        assert float(a.grad.abs().max()) > 0 and torch.equal(a.grad, b.grad)
    assert not tex.decoder.lout.weight.grad[:3].any() and not tex.decoder.lout.bias.grad[:3].any()
    assert float(tex.decoder.lout.weight.grad[3].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 6. tracer
@pytest.mark.parametrize("pos", [True, False])
def test_sdf_tracer_marches_a_textured_field_through_the_fused_iteration(pos, monkeypatch):
    """wisp_sdf_trace_step_fused on the fourth output row of a NeuralSDFTex fitted (300 fused steps) to a sphere whose colour is
    the normalised position mapped to [0,1] - against the modular marching loop: same packs hit, same depths and positions up to
    the summation order of the decoder's dot products; the colour queried at the hits is a colour.
    The fit runs at lr 1e-2, grid x 3, 16384 coordinates per step.  The depth bound is a statement about the FIELD as much as
    about the march: a ray whose convergence test flips between the two summation orders goes on for one more step of 0.8 x
    its distance, which stays under 6e-4 only where the field's slope along the ray is close to 1 - and further where the step
    leaves the cell.  The CPU oracle's sphere tracer over the oracle's field (same weights, decoder in fp32 against float64
    rounded to fp32, and against fp32 in another summation order) shows it without any of this package's kernels: the
    one-output field of the test this one follows never moves a ray by more than 2.2e-4 over eight seeds, a textured field fitted
    at that test's 3e-3 / x 10 / 2048 moves 1 - 4 of 1600 rays by 7e-4 to 1.4e-2 (on the MI355X: 1.44e-2 with the position, 9.9e-4
    without), and of the settings tried (1e-3 to 1e-2, x 3 to x 100, 512 to 16384) this one leaves the most accurate distance
    (rms 1.1 - 1.4e-3) and the smallest moves - yet one run in three there still had a ray past 6e-4.  The settings were chosen from
    that study, before this test ran with them; the bounds are the issue's."""
    from wisp.accelstructs import OctreeAS
    from wisp.core import Rays
    from wisp.tracers import PackedSDFTracer
    from wisp.trainers import SDFTrainStep
    idx = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing='ij'), -1).reshape(-1, 3)
    ctr = (idx + 0.5) / 16 - 1
    P = idx[np.abs(np.linalg.norm(ctr, axis=1) - 0.55) < 0.15]
    blas = OctreeAS.from_quantized_points(torch.from_numpy(P).short().to(DEV), 5)
    nef = _tex_field(blas, pos, lods=3, seed=11, std=0.01)
    tr = SDFTrainStep(nef, lr=1e-2, grid_lr_weight=3.0)
    assert tr._fused_field() is not None
    g = torch.Generator(device=DEV).manual_seed(12)
    cells = cuda(P.astype(np.float32))
    B = 16384
    for _ in range(300):
        pick = torch.randint(0, cells.shape[0], (B,), device=DEV, generator=g)
        xs = (cells[pick] + torch.rand(B, 3, device=DEV, generator=g)) / 16 - 1
        tr.step(xs, xs.norm(dim=-1, keepdim=True) - 0.55, torch.nn.functional.normalize(xs, dim=-1) * 0.5 + 0.5)
    o, d = make_rays(3000, 151, radius=2.5, spread=0.7)
    rays = Rays(cuda(o), cuda(d), dist_min=0.0, dist_max=6.0)
    tracer = PackedSDFTracer(num_steps=40, step_size=0.8, min_dis=0.0003)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("WISP_SDF_FUSED", fused)
        assert (PackedSDFTracer._fused_field(nef, 2) is not None) == (fused == "1")
        outs.append(tracer(nef, rays=rays, channels=["depth", "hit"], lod_idx=2))
    a, b = outs
    hits_a, hits_b = a.hit.reshape(-1), b.hit.reshape(-1)
    assert int(hits_b.sum()) > 500                                   # the fitted field is a surface the rays find
    differ = int((hits_a != hits_b).sum())
    assert differ <= max(2, int(0.002 * hits_b.numel())), differ
    both = hits_a & hits_b
    dd = (a.depth.reshape(-1)[both] - b.depth.reshape(-1)[both]).abs()
    margin(f"tex tracer depth max pos={int(pos)}", float(dd.max()), 6e-4)
    margin(f"tex tracer depth median pos={int(pos)}", float(dd.median()), 1e-6)
    margin(f"tex tracer xyz max pos={int(pos)}", float((a.xyz[both] - b.xyz[both]).abs().max()), 6e-4)
    # and the surface found is the sphere the field was fitted to (the one-output test's check of the fit itself)
    margin(f"tex tracer mean | |xyz| - 0.55 | pos={int(pos)}", float((b.xyz[both].norm(dim=-1) - 0.55).abs().mean()), 0.02)
    with torch.no_grad():
        rgb = nef(coords=a.xyz[hits_a], channels="rgb")
    assert rgb.shape == (int(hits_a.sum()), 3) and bool(torch.isfinite(rgb).all())
    assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_train_sdf_tex_script_trains_with_the_fused_step(tmp_path):
    """scripts/train_sdf_tex.py --fused-step on its procedural torus: both losses fall and the view finds the surface."""
    out = tmp_path / "out"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_sdf_tex.py"), "--write-test-mesh", str(tmp_path / "mesh"),
                          "--fused-step", "--epochs", "2", "--level", "5", "--num-samples", "20000", "--mesh-samples", "500000",
                          "--size", "48", "48", "--out-dir", str(out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    assert os.path.isfile(out / "albedo.png") and rec["albedo"] == str(out / "albedo.png")
    assert rec["hits"] > 100, rec
    assert rec["l2_last"] < rec["l2_first"] and rec["rgb_last"] < rec["rgb_first"], rec
