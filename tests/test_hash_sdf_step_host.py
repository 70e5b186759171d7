"""CPU: the host side of the fused hash-grid SDF training step (wisp_hash_sdf_train_step, csrc/hash_sdf_train.hip;
SDFTrainStep(fused_hash=True)): declaration / binding / export agreement, argument checks that return before any launch, the two
kernels' resources, the float64 reference of tests/hash_sdf_step_ref.py against torch autograd and oracle/hashgrid.py, its
exact-case generator, the shape rules of SDFTrainStep._fused_field's hash branch, SDFTrainStep's modular loss on a hash field against
the reference's SDFTrainer.step body, and the script's option wiring."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import kernel_meta
import hash_sdf_eval_ref as R
import hash_sdf_step_ref as S
from oracle import hashgrid as ohg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
REF = "/root/reference/wisp"
STEP, BYTES = "wisp_hash_sdf_train_step", "wisp_hash_sdf_train_scratch_bytes"
LDS_LIMIT = 160 * 1024                                   # one workgroup may hold the whole LDS of a compute unit


# ------------------------------------------------------------------------------------------------ 1. ABI and argument checks
def test_the_two_entry_points_are_declared_bound_and_exported():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    assert f"int {STEP}(" in header and f"int64_t {BYTES}(" in header
    assert "sdf_trainer.py:65-124" in header[header.index(f"int64_t {BYTES}(") - 2500:header.index(f"int64_t {BYTES}(")]
    assert STEP in C.SIGNATURES and BYTES in C.SIGNATURES and len(C.SIGNATURES[BYTES]) == 5
    # coords, gts, n | the hash field of wisp_hash_sdf_query (14) | five gradients, loss, scratch, scratch_bytes, stream
    assert len(C.SIGNATURES[STEP]) == 3 + 14 + 9
    assert C.SIGNATURES[STEP][3:17] == C.SIGNATURES["wisp_hash_sdf_query"][2:16]
    kinds = {C.c_vp: "p", C.c_i64: "l", C.c_i32: "i", C.c_f32: "f"}
    for name, ret in ((STEP, "int"), (BYTES, "int64_t")):
        decl = header[header.index(f"{ret} {name}("):]
        decl = decl[decl.index("(") + 1:decl.index(");")]
        got = []
        for arg in decl.split(","):
            arg = arg.split("/*")[0].strip()
            got.append("p" if "*" in arg or arg.startswith("wisp_stream_t") else "l" if arg.startswith("int64_t") else
                       "f" if arg.startswith("float") else "i")
        assert got == [kinds[a] for a in C.SIGNATURES[name]], name
    lib = ctypes.CDLL(C.LIB_PATH)
    assert hasattr(lib, STEP) and hasattr(lib, BYTES)
    assert C.lib.wisp_abi_version() == 4 == C.ABI_VERSION
    assert callable(C.hash_sdf_train_step)
    mk = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "Makefile")).read()
    assert "hash_sdf_train.hip" in mk
    with pytest.raises(ValueError, match="kind"):
        C.hash_sdf_train_step(None, None, dict(kind="octree"), None, None, None, None, None)


# positions in the argument list
COORDS, GTS, N = 0, 1, 2
CODEBOOK, DTYPE, BEGIN, RES, LODS, FDIM, BITS, MULTI, ZERO, W1, B1, W2, B2, HIDDEN = range(3, 17)
G_TABLE, G_W1, G_B1, G_W2, G_B2, LOSS, SCRATCH, SCRATCH_BYTES, STREAM = range(17, 26)


def _host_args(resolutions=(16, 80, 406, 2048), F=8, bits=12, multi=0, hidden=128, n=8):
    """a call whose sizes are valid and whose pointers point at host memory: nothing may be dereferenced on the way to a refusal
    (begin_idxes and resolutions are host arrays by contract)"""
    import wisp._C as C
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    L = len(resolutions)
    _, begin = ohg.table_layout(resolutions, 2 ** bits)
    bi = (ctypes.c_int64 * (L + 1))(*[int(b) for b in begin])
    rs = (ctypes.c_int32 * max(L, 1))(*resolutions)
    need = int(C.lib.wisp_hash_sdf_train_scratch_bytes(n, L, F, multi, hidden))
    args = [ptr, ptr, n, ptr, 0, bi, rs, L, F, bits, multi, L * F, ptr, ptr, ptr, ptr, hidden] + [ptr] * 7 + [need, ctypes.c_void_p(0)]
    return args, (buf, bi, rs)


def test_argument_checks_are_returned_before_any_launch():
    """every refusal comes back as WISP_ERR_INVALID with a text, with host pointers in every slot: had anything been launched or
    dereferenced on the way, this process would not be here to say so"""
    import wisp._C as C
    f = C._cdll.wisp_hash_sdf_train_step
    null = ctypes.c_void_p(0)
    args, keep = _host_args()
    assert args[SCRATCH_BYTES] > 0
    bad = [{FDIM: 3}, {FDIM: 16}, {HIDDEN: 0}, {HIDDEN: 257}, {LODS: 17}, {LODS: 0}, {N: 0}, {N: -1}, {MULTI: 2}, {BITS: 0}, {BITS: 31},
           {ZERO: -1}, {DTYPE: 1}, {DTYPE: 2}, {DTYPE: 3}] + \
          [{k: null} for k in (COORDS, GTS, CODEBOOK, BEGIN, RES, W1, B1, W2, B2, G_TABLE, G_W1, G_B1, G_W2, G_B2, LOSS, SCRATCH)]
    for patch in bad:
        args, keep = _host_args()
        for k, v in patch.items():
            args[k] = v
        assert f(*args) == -1, patch                                               # WISP_ERR_INVALID
        assert C.lib.wisp_last_error(), patch
    # 33 feature columns do not exist (feature_dim is even): the nearest shapes past 32 are 34 ('cat' of 17 x 2 - also 17 levels)
    # and 40 ('cat' of 5 x 8)
    args, keep = _host_args(resolutions=(4, 8, 16, 32, 64))
    assert f(*args) == -1 and b"32 feature columns" in C.lib.wisp_last_error()
    args, keep = _host_args(resolutions=tuple(range(4, 21)), F=2, multi=1)
    assert f(*args) == -1 and b"num_lods" in C.lib.wisp_last_error()
    # scratch one byte short
    args, keep = _host_args()
    args[SCRATCH_BYTES] -= 1
    assert f(*args) == -1 and b"scratch too small" in C.lib.wisp_last_error()
    # a level with fewer rows than a hashed index reaches
    args, keep = _host_args()
    args[BEGIN][4] -= 1
    assert f(*args) == -1 and b"fewer rows" in C.lib.wisp_last_error()


def test_scratch_bytes_is_monotone_and_rejects_what_the_step_does_not_serve():
    import wisp._C as C
    g = C.lib.wisp_hash_sdf_train_scratch_bytes
    for multi in (0, 1):
        sizes = [int(g(n, 4, 8, multi, 128)) for n in (1, 2, 16, 17, 512, 513, 5000, 1 << 16, 1 << 20)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], (multi, sizes)
    assert int(g(512, 4, 8, 0, 256)) > int(g(512, 4, 8, 0, 128)) > int(g(512, 4, 8, 1, 128))
    # one partial row per workgroup of 16 samples, rows padded to 16 floats, and 2^16 fp64 accumulators for every level's small-level
    # sums: nglod_hash.yaml at 512 coordinates
    assert int(g(512, 4, 8, 0, 128)) == 32 * ((128 * 35 + 2 * 128 + 2 + 15) // 16 * 16) * 4 + 4 * 65536 * 8
    for bad in ((0, 4, 8, 0, 128), (-1, 4, 8, 0, 128), (512, 0, 8, 0, 128), (512, 17, 2, 1, 128), (512, 4, 3, 0, 128), (512, 4, 16, 0, 128),
                (512, 5, 8, 0, 128), (512, 4, 8, 2, 128), (512, 4, 8, 0, 0), (512, 4, 8, 0, 257)):
        assert int(g(*bad)) == -1, bad
    assert int(g(512, 16, 2, 0, 256)) > 0 and int(g(512, 16, 8, 1, 256)) > 0       # the largest admitted shapes


def step_lds_bytes(hidden, cols, num_lods, F, multi):
    """the dynamic LDS of hash_sdf_train_kernel (csrc/sdf_step_dev.h: sdf_step_lds_bytes over hash_sdf_group_floats), restated"""
    in_dim = 3 + cols
    stage = hidden * (in_dim | 1) + 2 * hidden + 16 * (in_dim + (num_lods * F if multi else 0))
    return 4 * (stage + 16 * (2 * hidden + 2 + cols) + hidden * in_dim + 2 * hidden + 2)


@pytest.mark.skipif(not kernel_meta.available(LIB), reason="libwisp_hip.so not built or llvm-readelf missing")
def test_the_two_kernels_have_no_scratch_and_the_largest_shape_fits_the_lds():
    meta = kernel_meta.kernels(LIB)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    for part in ("hash_sdf_train_kernel", "hash_sdf_train_reduce_kernel"):
        hits = {n: v for n, v in kern.items() if part + "(" in n}
        assert len(hits) == 1, (part, list(hits))
        for name, v in hits.items():
            assert v["scratch"] == 0 and v["wg"] == 256 and v["lds"] == 0 and v["vgpr"] + v["agpr"] <= 128, (name, v)
    # dynamic LDS only, raised past the 64 KB default through WISP_ALLOW_LDS; every admitted shape fits one workgroup's 160 KiB
    worst = max(step_lds_bytes(256, L * F if not multi else F, L, F, multi)
                for F in (2, 4, 8) for L in range(1, 17) for multi in (0, 1) if (F if multi else L * F) <= 32)
    assert worst == step_lds_bytes(256, 32, 4, 8, 0) == 112968 and worst <= LDS_LIMIT
    assert step_lds_bytes(128, 32, 4, 8, 0) == 58696                              # nglod_hash.yaml: two workgroups a compute unit


# ------------------------------------------------------------------------------------------------ 2. the float64 reference
@pytest.mark.parametrize("res", R.GENERIC_RES)
@pytest.mark.parametrize("hidden,F,multiscale,lod_idx", [(32, 8, 'cat', 3), (17, 4, 'cat', 2), (32, 4, 'sum', 1), (8, 2, 'cat', 0)])
def test_reference_equals_autograd_and_the_oracle_scatter(res, hidden, F, multiscale, lod_idx):
    """the written-out gradients against torch autograd through the same float64 forward (rounding of float64 sums only), and the
    table gradient against oracle.hashgrid.hashgrid_backward fed with the reference's feature gradient: the two differ by the fp32
    rounding of the oracle's blend factors, 3 * 2^-24 relative per term"""
    fld = R.generic_field(res, hidden, F=F, multiscale=multiscale, lod_idx=lod_idx, seed=7)
    coords = R.generic_points(300, seed=3)
    gts = R.sphere_sdf(coords)
    got, want = S.step_reference(fld, coords, gts), S.autograd_reference(fld, coords, gts)
    for k in ("loss", "pred", "table", "w1", "b1", "w2", "b2"):
        assert got[k].shape == want[k].shape, k
        scale = max(float(want[k].abs().max()), 1e-30)
        assert float((got[k] - want[k]).abs().max()) <= 1e-12 * scale + 1e-18, k
    assert torch.equal(got["pred"].reshape(-1, 1), R.reference(fld, coords))
    L = len(res)
    p = S.decoder_parts(fld, coords, gts)
    full = torch.zeros(300, L * F, dtype=torch.float64)
    for l, col in S.live_levels(fld):
        full[:, l * F:(l + 1) * F] = p["dfeat"][:, col:col + F]
    orc = ohg.hashgrid_backward(coords, full, tuple(fld["table"].shape), fld["begin"], fld["resolutions"], fld["bitwidth"],
                                accum_dtype=torch.float64)
    mass = ohg.hashgrid_backward(coords, full.abs(), tuple(fld["table"].shape), fld["begin"], fld["resolutions"], fld["bitwidth"],
                                 accum_dtype=torch.float64)
    assert bool(((got["table"] - orc).abs() <= 4 * 2.0 ** -24 * mass + 1e-30).all())
    begin = fld["begin"]
    if multiscale == 'cat':                                                        # the levels from lod_idx on stay untouched
        assert bool((got["table"][int(begin[lod_idx]):] == 0).all())
        assert lod_idx == 0 or bool((got["table"][:int(begin[lod_idx])] != 0).any())
    else:
        assert all(bool((got["table"][int(begin[l]):int(begin[l + 1])] != 0).any()) for l in range(L))


# (hidden, F, multiscale, lod_idx, resolutions, bitwidth): hidden 1 / 17 / 128 / 256, F 2 / 4 / 8, 'cat' and 'sum', the last LOD, a
# middle one and 'cat' at LOD 0, tables of 2^6 .. 2^10 rows (2^6: every level hashed), one dense + one hashed level
EXACT = [(1, 8, 'cat', 3, R.EXACT_RES, 8), (17, 4, 'cat', 2, R.EXACT_RES, 10), (128, 2, 'cat', 0, R.EXACT_RES, 10),
         (256, 8, 'sum', 3, R.EXACT_RES, 7), (128, 4, 'sum', 1, (4, 16), 8), (256, 8, 'cat', 3, R.EXACT_RES, 6),
         (17, 2, 'cat', 1, (4, 16), 8),
         # a level of more than 2^16 entries keeps the f32 atomic scatter, beside small levels on the fp64 accumulators in one launch:
         # hashed (2^14 rows x 8) behind three small dense ones; hashed in the middle of a 'cat' whose last level is not gathered;
         # dense (32^3 rows x 8) at 2^16
         (128, 8, 'sum', 3, R.EXACT_RES, 14), (17, 8, 'cat', 2, (4, 32, 16), 14), (256, 8, 'sum', 3, R.EXACT_RES, 16)]


@pytest.mark.parametrize("n", [1, 16, 512])
@pytest.mark.parametrize("hidden,F,multiscale,lod_idx,res,bitwidth", EXACT)
def test_exact_step_cases_are_exact(hidden, F, multiscale, lod_idx, res, bitwidth, n):
    """the generator's own assertions ran when the case was built (bit budget of every stage at or below 24 bits, relu on both
    sides, every live level with a gradient, shared table rows); here: float64 and autograd agree BIT FOR BIT - exact sums have no
    order - and the fp32 forward equals the float64 one"""
    case = S.exact_step_case(hidden, F, multiscale, lod_idx, n, res, bitwidth, seed=2)
    fld, coords, gts, want = case["field"], case["coords"], case["gts"], case["want"]
    assert set(case["spans"]) == {"diff", "loss", "b2", "b1", "w2", "w1", "dfeat", "table"} and max(case["spans"].values()) < 24.0
    auto = S.autograd_reference(fld, coords, gts)
    for k in auto:
        assert torch.equal(auto[k], want[k]), k
        assert torch.equal(want[k].float().double(), want[k]), k                    # every result is an fp32 value
    assert torch.equal(R.reference(fld, coords, torch.float32).double().reshape(-1), want["pred"])
    dense = [ohg.level_is_dense(r, 2 ** bitwidth) for r in res]
    assert dense == {6: [False] * 4, 7: [True, False, False, False], 8: [True] + [False] * (len(res) - 1),
                     10: [True, True, False, False], 14: [r < 32 for r in res], 16: [True] * 4}[bitwidth]
    # which scatter a live level takes (csrc/hash_sdf_train.hip: at most 2^16 entries -> fp64 accumulators): from 2^14 rows on both
    entries = [int(fld["begin"][l + 1] - fld["begin"][l]) * F for l, _ in S.live_levels(fld)]
    assert (bitwidth >= 14) == (any(e > 2 ** 16 for e in entries) and any(e <= 2 ** 16 for e in entries))
    if n > 1:
        assert bool((coords < -1).any()) and bool((gts.double() != want["pred"]).sum() > n // 2)
    if multiscale == 'cat' and lod_idx == 0:
        assert bool((want["table"] == 0).all()) and bool((want["w1"][:, 3:] == 0).all()) and bool((want["w1"][:, :3] != 0).any())
    assert float(want["loss"]) > 0 and bool((want["w2"] != 0).any())


def test_an_inexact_step_is_refused():
    case = S.exact_step_case(17, 4, 'cat', 2, 16, R.EXACT_RES, 10, seed=2)
    fld, coords, gts = case["field"], case["coords"], case["gts"]
    with pytest.raises(AssertionError, match="power of two"):
        S.check_exact_step(fld, coords[:15], gts[:15], case["bits"])
    with pytest.raises(AssertionError, match="quantum"):
        S.check_exact_step(fld, coords, gts + 2.0 ** -10, case["bits"])
    with pytest.raises(AssertionError, match="leave fp32"):
        S.check_exact_step(fld, coords, gts, case["bits"], prefill=2.0 ** 12)
    with pytest.raises(AssertionError):
        S.check_exact_step(fld, R.generic_points(16, seed=1), gts, case["bits"])


# ------------------------------------------------------------------------------------------------ 3. shape rules
def _cpu_nef(F=8, lods=4, multiscale='cat', hidden=32, bitwidth=12):
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralSDF
    torch.manual_seed(3)
    grid = HashGrid.from_geometric(None, feature_dim=F, num_lods=lods, multiscale_type=multiscale, feature_std=0.05,
                                   codebook_bitwidth=bitwidth, min_grid_res=16, max_grid_res=2048)
    nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=hidden, num_layers=1)
    return nef


def test_fused_field_takes_the_hash_branch_only_when_asked_and_only_for_its_shape(monkeypatch):
    """the rules on CPU objects that claim to live on the GPU (nothing is launched): every tensor answers is_cuda with True"""
    from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
    from wisp.trainers import SDFTrainStep
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED", raising=False)
    steps = dict(default=SDFTrainStep(_cpu_nef()), asked=SDFTrainStep(_cpu_nef(), fused_hash=True),
                 summed=SDFTrainStep(_cpu_nef(multiscale='sum'), fused_hash=True),
                 all_lods=SDFTrainStep(_cpu_nef(), fused_hash=True, only_last=False),
                 half=SDFTrainStep(_cpu_nef(), fused_hash=True),
                 wide=SDFTrainStep(_cpu_nef(lods=5), fused_hash=True),
                 tex=SDFTrainStep(NeuralSDFTex(_cpu_nef().grid, embedder_type='identity', hidden_dim=32, num_layers=1), fused_hash=True))
    half = steps["half"].nef.grid.codebook.feats                                    # (FlatParams homes parameters in f32: re-typed after)
    half.data, half.grad = half.data.half(), None
    half.grad = torch.zeros_like(half.data)
    assert steps["asked"]._fused_field() is None                                    # on the host nothing is fused
    steps["asked"]._fused_cache = None
    monkeypatch.setattr(torch.Tensor, "is_cuda", True, raising=False)
    assert not steps["default"].fused_hash and steps["default"]._fused_field() is None
    ok = steps["asked"]._fused_field()
    nef = steps["asked"].nef
    assert ok is not None and ok["hash"] and ok["grid"] is nef.grid and ok["lods"] == 4
    assert ok["host"] == dict(kind='hash', begin_idxes=nef.grid.codebook.begin_idxes.tolist(), resolutions=[16, 80, 406, 2048],
                              feature_dim=8, codebook_bitwidth=12, multiscale='cat', zero_from_col=24)
    assert ok["prm"][0] is nef.grid.codebook.feats and len(ok["prm"]) == 5
    assert steps["asked"]._fused_field() is ok                                      # cached
    s = steps["summed"]._fused_field()
    assert s is not None and s["host"]["multiscale"] == 'sum' and s["host"]["zero_from_col"] == 32
    for name in ("all_lods", "half", "wide", "tex"):
        assert steps[name]._fused_field() is None, name
    assert steps["tex"].textured
    # what can change under a live trainer is looked at on every call
    assert steps["asked"]._fused_still_valid(ok)
    grad = nef.grid.codebook.feats.grad
    nef.grid.codebook.feats.grad = None
    assert not steps["asked"]._fused_still_valid(ok) and steps["asked"]._fused_field() is None
    nef.grid.codebook.feats.grad = grad
    steps["asked"]._fused_cache = None
    assert steps["asked"]._fused_field() is not None
    steps["asked"].only_last = False
    assert steps["asked"]._fused_field() is None
    steps["asked"].only_last = True
    assert steps["asked"]._fused_field() is not None
    monkeypatch.setenv("WISP_SDF_TRAIN_FUSED", "0")
    steps["asked"]._fused_cache = None
    assert steps["asked"]._fused_field() is None


def test_config_sdf_trainer_keeps_the_reference_schema():
    import dataclasses
    from wisp.trainers import ConfigSDFTrainer
    assert "fused_hash" not in {f.name for f in dataclasses.fields(ConfigSDFTrainer)}


# ------------------------------------------------------------------------------------------------ 4. the reference's step
def _cpu_hashgrid(coords, codebook_bitwidth, lod_idx, codebook, zero_from_col=None):
    """wisp.ops.grid.hashgrid on the host: the oracle's autograd function, with the kernel's fused zeroing as a mask"""
    out = ohg.hashgrid(coords, codebook.resolutions, codebook_bitwidth, lod_idx, codebook.feats, codebook.begin_idxes)
    if zero_from_col is not None:
        keep = torch.ones(out.shape[-1], dtype=out.dtype)
        keep[zero_from_col:] = 0
        out = out * keep
    return out


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not mounted")
@pytest.mark.parametrize("only_last", [True, False])
def test_modular_hash_loss_equals_the_reference_method(only_last, monkeypatch):
    """SDFTrainer.step (trainers/sdf_trainer.py:65-124), the method body compiled from the reference file, over a NeuralSDF /
    HashGrid of this package on the host (the grid op replaced by the oracle's) with torch.optim.Adam - next to
    SDFTrainStep.step(coords, gts) (fused optimizer replaced by its CPU restatement): same loss, same parameters after three
    steps.  The finest level's rows never move: 'cat' zeroes the columns from lod_idx * feature_dim on, at the finest LOD too."""
    import wisp._C as C
    import wisp.models.grids.hash_grid as hg
    from test_reference_modules import _TorchWithoutNvtx, _reference_method, _torch_optim_groups
    from wisp.trainers import SDFTrainStep
    monkeypatch.setattr(hg.grid_ops, "hashgrid", _cpu_hashgrid)
    monkeypatch.setattr(C, "optim_step_groups", _torch_optim_groups)
    ref_step = _reference_method("trainers/sdf_trainer.py", "SDFTrainer", "step", dict(torch=_TorchWithoutNvtx()))
    g = torch.Generator().manual_seed(2)
    X, Y = torch.rand(3, 64, 3, generator=g) * 2 - 1, torch.randn(3, 64, 1, generator=g) * 0.1
    fr, fm = _cpu_nef(bitwidth=8), _cpu_nef(bitwidth=8)
    lods = [3] if only_last else [0, 1, 2, 3]
    named = dict(fr.named_parameters())
    opt = torch.optim.Adam([{"params": [p for n, p in named.items() if 'decoder' in n], "lr": 1e-3},
                            {"params": [p for n, p in named.items() if 'decoder' not in n], "lr": 2e-3}], eps=1e-15)
    metrics = types.SimpleNamespace(total_loss=0.0, l2_loss=0.0, rgb_loss=0.0, num_samples=0)
    me = types.SimpleNamespace(pipeline=types.SimpleNamespace(nef=fr, zero_grad=fr.zero_grad), device='cpu', loss_lods=lods,
                               train_dataset=types.SimpleNamespace(sample_tex=False), tracker=types.SimpleNamespace(metrics=metrics),
                               optimizer=opt)
    first = fm.grid.codebook.feats.detach().clone()
    tr = SDFTrainStep(fm, lr=1e-3, eps=1e-15, grid_lr_weight=2.0, optimizer='adam', only_last=only_last)
    assert not tr.textured and tr.loss_lods() == lods and tr._fused_field() is None
    for x, y in zip(X, Y):
        before = metrics.total_loss
        ref_step(me, {"coords": x, "sdf": y})
        loss = tr.step(x, y)
        want = metrics.total_loss - before
        assert abs(float(loss) * x.shape[0] - want) <= 2e-5 * max(1.0, want)
    for (n1, p1), (n2, p2) in zip(fr.named_parameters(), fm.named_parameters()):
        np.testing.assert_allclose(p2.detach().numpy(), p1.detach().numpy(), rtol=1e-5, atol=2e-7, err_msg=n1)
    begin = fm.grid.codebook.begin_idxes.tolist()
    moved = fm.grid.codebook.feats.detach() != first
    assert bool(moved[:begin[3]].any()) and not bool(moved[begin[3]:].any())


# ------------------------------------------------------------------------------------------------ 5. the script
def test_train_nglod_wires_fused_hash(monkeypatch):
    """--grid hash --fused-step builds SDFTrainStep(..., fused_hash=True), an octree grid leaves it off, and fit_fused returns what
    the JSON record's fused_hash_step carries; the docstring no longer says the hash grid has no fused step"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train_nglod
    finally:
        sys.path.pop(0)
    import wisp.trainers as T
    assert "no fused step" not in train_nglod.__doc__ and "fused_hash=True" in train_nglod.__doc__
    seen = []

    class Step:
        def __init__(self, nef, **kw):
            seen.append(kw)
            self.fused_hash = kw["fused_hash"]

        def _fused_field(self):
            raise AssertionError("on the host the field is not asked")

        def step(self, coords, gts):
            return torch.zeros(())

    monkeypatch.setattr(T, "SDFTrainStep", Step)
    cfg = types.SimpleNamespace(optimizer=types.SimpleNamespace(lr=1e-3, eps=1e-15, betas=(0.9, 0.999)), grid_lr_weight=1.0,
                                dataloader=types.SimpleNamespace(batch_size=4), only_last=True, max_epochs=1, resample=False)
    ds = types.SimpleNamespace(data=dict(coords=torch.zeros(8, 3), sdf=torch.zeros(8)))
    for nef, want in ((_cpu_nef(), True), (types.SimpleNamespace(grid=object(), train=lambda: None, eval=lambda: None), False)):
        trainer = types.SimpleNamespace(pipeline=types.SimpleNamespace(nef=nef))
        assert train_nglod.fit_fused(trainer, ds, cfg, "cpu") is False
        assert seen[-1]["fused_hash"] is want and seen[-1]["only_last"] is True
    src = open(os.path.join(ROOT, "scripts", "train_nglod.py")).read()
    assert "fused_hash_step=fused_hash_step" in src
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_nglod.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--fused-step" in r.stdout and "--grid {octree,hash}" in r.stdout
