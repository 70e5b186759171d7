"""CPU: the host side of the fused textured SDF step (wisp_sdf_tex_train_step, csrc/spc_grad.hip; SDFTrainStep for a NeuralSDFTex):
declaration / binding / export agreement, argument checks that fail before any launch, the kernels' resources read from the code
objects, SDFTrainStep's modular textured loss against the reference's SDFTrainer.step body executed in place, and step()'s argument
rules."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
REF = "/root/reference/wisp"


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_sdf_tex_train_step_is_declared_bound_and_exported():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    assert "int wisp_sdf_tex_train_step(" in header and "int64_t wisp_sdf_tex_train_scratch_bytes(" in header
    assert len(C.SIGNATURES["wisp_sdf_tex_train_step"]) == 31 and len(C.SIGNATURES["wisp_sdf_tex_train_scratch_bytes"]) == 5
    # the one-output step's arguments plus rgb_gts and pos_input
    assert len(C.SIGNATURES["wisp_sdf_tex_train_step"]) == len(C.SIGNATURES["wisp_sdf_train_step"]) + 2
    lib = ctypes.CDLL(C.LIB_PATH)
    assert hasattr(lib, "wisp_sdf_tex_train_step") and hasattr(lib, "wisp_sdf_tex_train_scratch_bytes")
    assert C.lib.wisp_abi_version() == 4
    assert callable(C.sdf_tex_train_step)


def _base_args():
    """a call whose sizes are all valid and whose pointers are all null"""
    null = ctypes.c_void_p(0)
    #       coords gts  rgb   n  octree exsum points trinkets feats levels rows  L  C  half pos  w1    b1    w2    b2    H
    return [null, null, null, 8, null, null, null, null, null, null, null, 3, 16, 0, 1, null, null, null, null, 128,
            null, null, null, null, null, null, null, 0, null, 0, null]


def test_bad_sizes_and_null_pointers_fail_before_any_launch():
    import wisp._C as C
    f = C._cdll.wisp_sdf_tex_train_step
    #  null pointers alone; channels != 16; hidden 0 / 257; num_lods 17 / 0; pos_input 2 / -1; empty batch
    for patch in ({}, {12: 8}, {12: 32}, {19: 0}, {19: 257}, {11: 17}, {11: 0}, {14: 2}, {14: -1}, {3: 0}):
        args = _base_args()
        for k, v in patch.items():
            args[k] = v
        assert f(*args) == -1, patch                                           # WISP_ERR_INVALID
        assert C.lib.wisp_last_error()


def test_size_checks_come_first_with_real_host_pointers():
    """the same bad sizes with every pointer non-null (host memory: nothing may be dereferenced on the way to the refusal)"""
    import wisp._C as C
    f = C._cdll.wisp_sdf_tex_train_step
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for patch in ({12: 8}, {19: 0}, {19: 257}, {11: 17}, {14: 2}):
        args = [ptr if isinstance(a, ctypes.c_void_p) else a for a in _base_args()]
        args[-1] = ctypes.c_void_p(0)                                          # the stream stays the null stream
        for k, v in patch.items():
            args[k] = v
        assert f(*args) == -1, patch


def test_scratch_bytes_is_monotone_and_rejects_bad_arguments():
    import wisp._C as C
    g = C.lib.wisp_sdf_tex_train_scratch_bytes
    for pos in (0, 1):
        for lods in (1, 3, 5, 16):
            sizes = [int(g(n, lods, 16, 128, pos)) for n in (0, 1, 2, 37, 512, 513, 5000, 100000, 1 << 20)]
            assert sizes[0] >= 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[1] > 0, (pos, lods, sizes)
    assert int(g(512, 6, 16, 128, 1)) > int(g(512, 6, 16, 128, 0))            # three more input columns per hidden unit
    assert int(g(512, 6, 16, 256, 1)) > int(g(512, 6, 16, 128, 1))
    for bad in ((-1, 3, 16, 128, 1), (512, 0, 16, 128, 1), (512, 17, 16, 128, 1), (512, 3, 8, 128, 1), (512, 3, 32, 128, 1),
                (512, 3, 16, 0, 1), (512, 3, 16, 257, 1), (512, 3, 16, 128, 2), (512, 3, 16, 128, -1)):
        assert int(g(*bad)) == -1, bad


# ------------------------------------------------------------------------------------------------ 2. resources
@pytest.mark.skipif(not kernel_meta.available(LIB), reason="libwisp_hip.so not built or llvm-readelf missing")
def test_the_two_kernels_have_no_scratch_and_256_thread_workgroups():
    meta = kernel_meta.kernels(LIB)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    # both instantiations of the one train kernel (one output, four outputs) and the one reduce kernel both steps share
    for part in ("void sdf_train_kernel<1>(", "void sdf_train_kernel<4>(", "sdf_train_reduce_kernel("):
        hits = {n: v for n, v in kern.items() if n.startswith(part)}
        assert len(hits) == 1, (part, list(hits))
        for name, v in hits.items():
            assert v["scratch"] == 0 and v["wg"] == 256, (name, v)
            # dynamic LDS only (sized per call, raised past the 64 KB default through WISP_ALLOW_LDS)
            assert "reduce" in part or v["lds"] == 0, (name, v)
    assert not [n for n in kern if "sdf_tex_train" in n or n.startswith("sdf_train_kernel(")], "a per-field twin of the kernel"


# ------------------------------------------------------------------------------------------------ 3. step() arguments
class _Field(torch.nn.Module):
    """CPU stand-in for a textured field: a table per LOD + one Linear with four outputs, 'rgb' and 'sdf' answered together."""
    def __init__(self, textured=True):
        super().__init__()
        torch.manual_seed(8)
        self.grid = torch.nn.Module()
        self.grid.num_lods = 3
        self.grid.feats = torch.nn.Parameter(torch.randn(3, 32, 4) * 0.1)            # 'grid' in the name -> grid group
        self.decoder = torch.nn.Linear(4 + 3, 4 if textured else 1)
        self._forward_functions = {self.rgbsdf: {"rgb", "sdf"}} if textured else {self.rgbsdf: {"sdf"}}
        self.textured = textured

    def rgbsdf(self, coords, lod_idx):
        cell = ((coords[:, 0] * 0.5 + 0.5) * 31).long().clamp(0, 31)
        f = self.grid.feats[: lod_idx + 1, cell].sum(0)
        return self.decoder(torch.cat([f, coords], -1))

    def forward(self, coords=None, lod_idx=None, channels=None):
        y = self.rgbsdf(coords, lod_idx)
        if not self.textured:
            return [y] if isinstance(channels, (list, tuple)) else y
        out = dict(rgb=torch.sigmoid(y[..., :3]), sdf=y[..., 3:4])
        return [out[c] for c in channels] if isinstance(channels, (list, tuple)) else out[channels]


def test_step_raises_for_a_missing_or_a_superfluous_rgb_before_touching_a_device(monkeypatch):
    import wisp._C as C
    from wisp.trainers import SDFTrainStep

    def never(*a, **k):
        raise AssertionError("step() went on past its argument check")
    for name in ("sdf_train_step", "sdf_tex_train_step", "optim_step_groups"):
        monkeypatch.setattr(C, name, never)
    x, y, c = torch.rand(8, 3) * 2 - 1, torch.randn(8, 1), torch.rand(8, 3)
    tex = SDFTrainStep(_Field(True))
    assert tex.textured
    monkeypatch.setattr(tex, "_forward_backward", never)
    with pytest.raises(ValueError, match="rgb"):
        tex.step(x, y)
    with pytest.raises(ValueError, match="rgb"):
        tex.step(x, y, rgb=None)
    plain = SDFTrainStep(_Field(False))
    assert not plain.textured
    monkeypatch.setattr(plain, "_forward_backward", never)
    with pytest.raises(ValueError, match="rgb"):
        plain.step(x, y, c)
    with pytest.raises(ValueError, match="rgb"):
        plain.step(x, y, rgb=c)


def test_real_fields_are_told_apart_by_their_forward_functions():
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDF
    from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
    from wisp.trainers import SDFTrainStep
    blas = OctreeAS.make_dense(2)
    grid = OctreeGrid(blas, feature_dim=16, num_lods=2, multiscale_type='sum', feature_std=0.05)
    assert SDFTrainStep(NeuralSDFTex(grid, embedder_type='none', hidden_dim=16)).textured
    assert not SDFTrainStep(NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=16, num_layers=1)).textured
    # on the CPU nothing is fused: the modular launches stay
    assert SDFTrainStep(NeuralSDFTex(grid, embedder_type='none', hidden_dim=16))._fused_field() is None


# ------------------------------------------------------------------------------------------------ 4. the reference's step
@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not mounted")
@pytest.mark.parametrize("only_last", [True, False])
def test_modular_textured_loss_equals_the_reference_method(only_last):
    """SDFTrainer.step (trainers/sdf_trainer.py:65-124) with sample_tex, the method body compiled from the reference file, over
    the CPU stand-in field with torch.optim.Adam - next to SDFTrainStep.step(coords, gts, rgb) (fused optimizer replaced by its
    CPU restatement): the colour sum is accumulated inside the LOD loop on both sides; same loss, same parameters after three
    steps, and last_l2 / last_rgb are what the reference's tracker adds up.  (The reference hands each prediction to
    `preds.append(*...)`, which takes ONE argument: its field is given as a one-element list holding the (rgb, sdf) pair.)"""
    import wisp._C as C
    from test_reference_modules import _TorchWithoutNvtx, _reference_method, _torch_optim_groups
    from wisp.trainers import SDFTrainStep
    ref_step = _reference_method("trainers/sdf_trainer.py", "SDFTrainer", "step", dict(torch=_TorchWithoutNvtx()))
    g = torch.Generator().manual_seed(2)
    X, Y = torch.rand(3, 64, 3, generator=g) * 2 - 1, torch.randn(3, 64, 1, generator=g) * 0.1
    RGB = torch.rand(3, 64, 4, generator=g)                                   # (a fourth column, as a texture sample may carry)
    fr, fm = _Field(), _Field()
    lods = [2] if only_last else [0, 1, 2]
    named = dict(fr.named_parameters())
    opt = torch.optim.Adam([{"params": [p for n, p in named.items() if 'decoder' in n], "lr": 1e-3},
                            {"params": [p for n, p in named.items() if 'decoder' not in n], "lr": 2e-3}], eps=1e-15)
    metrics = types.SimpleNamespace(total_loss=0.0, l2_loss=0.0, rgb_loss=0.0, num_samples=0)
    nef_r = lambda coords=None, lod_idx=None, channels=None: [tuple(fr(coords=coords, lod_idx=lod_idx, channels=channels))]  # noqa: E731
    me = types.SimpleNamespace(pipeline=types.SimpleNamespace(nef=nef_r, zero_grad=fr.zero_grad), device='cpu', loss_lods=lods,
                               train_dataset=types.SimpleNamespace(sample_tex=True), tracker=types.SimpleNamespace(metrics=metrics),
                               optimizer=opt)
    saved = getattr(C, "optim_step_groups")
    C.optim_step_groups = _torch_optim_groups
    try:
        tr = SDFTrainStep(fm, lr=1e-3, eps=1e-15, grid_lr_weight=2.0, optimizer='adam', only_last=only_last)
        assert tr.textured and tr.loss_lods() == lods
        for x, y, c in zip(X, Y, RGB):
            before = (metrics.total_loss, metrics.l2_loss, metrics.rgb_loss)
            ref_step(me, {"coords": x, "sdf": y, "rgb": c})
            loss = tr.step(x, y, c)
            want = metrics.total_loss - before[0]
            assert abs(float(loss) * x.shape[0] - want) <= 2e-5 * max(1.0, want)
            assert abs(float(tr.last_l2) - (metrics.l2_loss - before[1])) <= 2e-5 * max(1.0, metrics.l2_loss - before[1])
            assert abs(float(tr.last_rgb) - (metrics.rgb_loss - before[2])) <= 2e-5 * max(1.0, metrics.rgb_loss - before[2])
            assert metrics.rgb_loss - before[2] > 0
    finally:
        C.optim_step_groups = saved
    for (n1, p1), (n2, p2) in zip(fr.named_parameters(), fm.named_parameters()):
        np.testing.assert_allclose(p2.detach().numpy(), p1.detach().numpy(), rtol=1e-5, atol=2e-7, err_msg=n1)


# ------------------------------------------------------------------------------------------------ 5. the rates of the 30-step check
@pytest.mark.parametrize("pos", [True, False])
def test_thirty_adam_steps_on_the_oracle_need_the_higher_rates(pos):
    """The study behind the learning rates of the GPU test's "30 real steps bring the loss below 0.7 x the first" check, on that
    test's inputs at B = 512 (4000 random level-5 cells, 4 LODs, every 11th coordinate outside, independent uniform colours): torch
    autograd through the CPU oracle's OctreeGrid lookup and decoder with torch.optim.Adam (eps 1e-15) - none of this package's
    kernels.  At 1e-3 / grid x 2, the rates of that test's gradient comparison, a CORRECT step does not reach 0.7 x in 30 steps; at
    3e-3 / grid x 10, the rates the tracer tests fit with, it gets far below.  (The initial weights are the oracle decoder's own
    draw, not the GPU test's: the statement is about the rates.)"""
    from oracle import nerf as onerf, octree_grid as og, spc as ospc
    rng = np.random.default_rng(240 + 512)
    P = rng.integers(0, 32, size=(4000, 3))
    oblas = onerf.OracleBLAS(ospc.points_to_octree(P, 5))
    pd, pyd = ospc.make_dual(oblas.points, oblas.pyramid)
    tr, _ = ospc.make_trinkets(oblas.points, oblas.pyramid, pd, pyd)
    active = [2, 3, 4, 5]
    inside = ((P[rng.integers(0, P.shape[0], 512)] + rng.uniform(0.02, 0.98, (512, 3))) / 16 - 1).astype(np.float32)
    inside[::11] = rng.uniform(-1.2, 1.2, (inside[::11].shape[0], 3))
    c = torch.from_numpy(inside)
    gt = torch.from_numpy(rng.normal(size=(512, 1)).astype(np.float32) * 0.1)
    col = torch.from_numpy(rng.uniform(size=(512, 3)).astype(np.float32))
    ratio = {}
    for lr, glw in ((1e-3, 2.0), (3e-3, 10.0)):
        torch.manual_seed(7)
        feats = [(torch.randn(int(pyd[0, l]), 16) * 0.05).requires_grad_(True) for l in active]
        dec = onerf.OracleDecoder((3 if pos else 0) + 16, 4, 128, 1, True)
        opt = torch.optim.Adam([{"params": list(dec.parameters()), "lr": lr}, {"params": feats, "lr": lr * glw}], eps=1e-15)
        losses = []
        for _ in range(30):
            opt.zero_grad()
            f = og.octree_grid_interpolate(oblas, tr, feats, c, 3, active[0], active, 'sum', 16, True)
            y = dec(torch.cat([c, f], -1) if pos else f)
            loss = (((torch.sigmoid(y[:, :3]) - col) ** 2).sum() + ((y[:, 3:4] - gt) ** 2).sum()) / 512
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert 0.2 < losses[0] < 0.35                       # 3 / 12 from the colours + the distance term
        ratio[lr] = losses[-1] / losses[0]
    assert ratio[1e-3] > 0.7, ratio
    assert ratio[3e-3] < 0.35, ratio
