"""CPU: the host side of the fused triplanar SDF training step (wisp_triplane_sdf_train_step, csrc/triplane_sdf_train.hip;
SDFTrainStep(fused_triplane=True)): the float64 reference of tests/triplane_sdf_step_ref.py against float64 autograd through
oracle/triplanar.py, its exact-case generator and the coverage it claims, declaration / binding / export agreement, argument checks
that return before any launch, the scratch size, the two kernels' resources, the shape rules of SDFTrainStep._fused_field's
triplanar branch, and the script's option wiring."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_meta
import triplane_sdf_eval_ref as R
import triplane_sdf_step_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
STEP, BYTES = "wisp_triplane_sdf_train_step", "wisp_triplane_sdf_train_scratch_bytes"
LDS_LIMIT = 160 * 1024                                   # one workgroup may hold the whole LDS of a compute unit
WIDE = 1 << 16                                           # a plane of at most this many entries is summed in fp64 accumulators


# ------------------------------------------------------------------------------------------------ 1. the float64 reference
@pytest.mark.parametrize("hidden,F,multiscale,sizes", [(32, 4, 'sum', (33,)), (17, 2, 'cat', (9, 17, 33)), (32, 4, 'sum', (5, 9, 17)),
                                                       (8, 1, 'cat', (1, 9)), (1, 4, 'sum', (33,))])
def test_reference_equals_float64_autograd_through_the_oracle_grid(hidden, F, multiscale, sizes):
    """the written-out gradients against torch autograd over oracle.triplanar.interpolate (F.grid_sample, align_corners=True,
    reflection) and a float64 decoder, on random planes and nn.Linear-initialised weights.  The positions lie on the 2^-20 lattice
    (a third outside the cube, some on the faces): over power-of-two spans the fp32 source coordinate the kernel forms is then the
    exact one - asserted - so grid_sample's float64 coordinate is the same number and the two differ by the rounding of float64 sums
    alone."""
    fld = R.generic_field(sizes, hidden, F=F, multiscale=multiscale, seed=7)
    coords = S.lattice_points(300, seed=3)
    c = coords.numpy()
    for size in sizes:
        assert np.array_equal(R.source_index(c, size).astype(np.float64), R.exact_source_index(c.astype(np.float64), size))
    assert bool((coords.abs() > 1).any()) and bool((coords.abs() == 1).any())
    gts = R.sphere_sdf(coords)
    got, want = S.step_reference(fld, coords, gts), S.autograd_reference(fld, coords, gts)
    for k in ("loss", "pred", "w1", "b1", "w2", "b2"):
        assert got[k].shape == want[k].shape, k
        scale = max(float(want[k].abs().max()), 1e-30)
        assert float((got[k] - want[k]).abs().max()) <= 1e-12 * scale + 1e-18, k
    assert len(got["planes"]) == len(want["planes"]) == 3 * len(sizes)
    for i, (a, b) in enumerate(zip(got["planes"], want["planes"])):
        assert a.shape == b.shape == fld["planes"][i].shape, i
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-30) + 1e-18, i
        assert hidden == 1 or bool((a != 0).any()), i
    assert torch.equal(got["pred"].reshape(-1, 1), R.reference(fld, coords))
    assert float(want["loss"]) > 0


# (hidden, F, multiscale, sizes, b): hidden 1 / 17 / 128 / 256; 'sum' over 33 alone and over 5 + 9 + 17 + 33; 'cat' of 2 and 4 levels,
# one of them with K = 48 columns; a plane of size 1 under 'sum' and under 'cat'; and planes of 4 x 129 x 129 = 66564 entries, above
# 2^16: the f32-atomic regime, alone and beside a small plane on the fp64 accumulators (b = 3: a fraction bit at size 129)
EXACT = [(1, 4, 'sum', (33,), 1), (17, 4, 'sum', (5, 9, 17, 33), 1), (128, 4, 'sum', (33,), 1), (256, 4, 'sum', (5, 9, 17, 33), 1),
         (128, 2, 'cat', (9, 33), 1), (17, 2, 'cat', (5, 9, 17, 33), 1), (256, 4, 'cat', (5, 9, 17, 33), 1), (128, 4, 'sum', (1, 9), 1),
         (128, 4, 'cat', (1, 17), 1), (128, 4, 'sum', (129,), 3), (17, 4, 'cat', (9, 129), 3)]
STAGES = {"pred - gt", "diff", "loss", "b2", "b1", "w2", "w1", "dfeat", "planes"}


@pytest.mark.parametrize("n", [1, 16, 512])
@pytest.mark.parametrize("hidden,F,multiscale,sizes,b", EXACT)
def test_exact_step_cases_are_exact(hidden, F, multiscale, sizes, b, n):
    """the generator's own assertions ran when the case was built (bit budget of every stage below 24 bits, relu on both sides,
    reflected samples, lookups on the last texel line, lookups on a texel, shared texels); here: float64 and float64 autograd agree
    BIT FOR BIT - exact sums have no order -, every result is an fp32 value, and the fp32 forward equals the float64 one"""
    case = S.exact_step_case(hidden, F, multiscale, sizes, n, seed=2, b=b)
    fld, coords, gts, want, cov = case["field"], case["coords"], case["gts"], case["want"], case["coverage"]
    assert set(case["spans"]) == STAGES and max(case["spans"].values()) < 24.0
    auto = S.autograd_reference(fld, coords, gts)
    for k in ("loss", "pred", "w1", "b1", "w2", "b2"):
        assert torch.equal(auto[k], want[k]), k
        assert torch.equal(want[k].float().double(), want[k]), k
    for i, (a, w) in enumerate(zip(auto["planes"], want["planes"])):
        assert torch.equal(a, w) and torch.equal(w.float().double(), w), i
    assert torch.equal(R.reference(fld, coords, torch.float32).double().reshape(-1), want["pred"])
    assert R.num_cols(fld) == (3 * F if multiscale == 'sum' else 3 * F * len(sizes)) <= 48
    entries = [F * s * s for s in sizes]
    assert (129 in sizes) == any(e > WIDE for e in entries) and (sizes == (129,) or any(e <= WIDE for e in entries))
    if n >= 16:
        assert cov["reflected"] >= 1 and cov["edge"] >= 1 and cov["on_texel"] >= 1 and cov["shared"] >= 1, cov
        assert cov["planes_with_gradient"] >= (1 if hidden == 1 else len(sizes)), cov
        assert bool((gts.double() != want["pred"]).sum() > n // 2)
    if n == 512:
        assert cov["shared"] >= 100 and cov["reflected"] >= 100 and cov["edge"] >= 100, cov
    assert float(want["loss"]) > 0 and float(want["b2"]) != 0


def test_the_all_miss_case_moves_the_output_bias_alone():
    case = S.exact_step_case(128, 4, 'sum', (33,), 16, seed=2, all_miss=True)
    want = case["want"]
    assert float(want["b2"]) != 0 and float(want["loss"]) > 0
    assert all(bool((want[k] == 0).all()) for k in ("w1", "b1", "w2")) and all(bool((g == 0).all()) for g in want["planes"])


def test_an_inexact_step_is_refused():
    case = S.exact_step_case(17, 4, 'sum', (5, 9, 17, 33), 16, seed=2)
    fld, coords, gts = case["field"], case["coords"], case["gts"]
    with pytest.raises(AssertionError, match="power of two"):
        S.check_exact_step(fld, coords[:15], gts[:15], case["bits"])
    with pytest.raises(AssertionError, match="quantum"):
        S.check_exact_step(fld, coords, gts + 2.0 ** -10, case["bits"])
    with pytest.raises(AssertionError, match="leave fp32"):
        S.check_exact_step(fld, coords, gts, case["bits"], prefill=2.0 ** 14)
    with pytest.raises(AssertionError):
        S.check_exact_step(fld, R.generic_points(16, seed=1), gts, case["bits"])
    with pytest.raises(AssertionError, match="power of two"):                      # a span of 9: the reflection is not exact
        S.check_exact_step(R.exact_field(17, sizes=(10,), seed=1, w2_nonzero=16), coords, gts, case["bits"])


# ------------------------------------------------------------------------------------------------ 2. ABI and argument checks
def test_the_two_entry_points_are_declared_bound_and_exported():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    assert f"int {STEP}(" in header and f"int64_t {BYTES}(" in header
    assert STEP in header[header.index("Entry points that are only ADDED"):header.index("int wisp_abi_version")]
    assert "sdf_trainer.py:65-124" in header[header.index(f"int64_t {BYTES}(") - 2500:header.index(f"int64_t {BYTES}(")]
    assert STEP in C.SIGNATURES and BYTES in C.SIGNATURES and len(C.SIGNATURES[BYTES]) == 6
    # coords, gts, n | the triplanar field of wisp_triplane_sdf_query (10) | plane gradients, four gradients, loss, scratch,
    # scratch_bytes, stream
    assert len(C.SIGNATURES[STEP]) == 3 + 10 + 9
    assert C.SIGNATURES[STEP][3:13] == C.SIGNATURES["wisp_triplane_sdf_query"][2:12]
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
    assert C.lib.wisp_triplane_sdf_train_scratch_bytes.restype is C.c_i64
    assert C.lib.wisp_abi_version() == 4 == C.ABI_VERSION
    assert callable(C.triplane_sdf_train_step)
    mk = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "Makefile")).read()
    assert "triplane_sdf_train.hip" in mk
    for kind in ("octree", "hash"):
        with pytest.raises(ValueError, match="kind"):
            C.triplane_sdf_train_step(None, None, dict(kind=kind), None, None, None, None, None)


# positions in the argument list
COORDS, GTS, N = 0, 1, 2
PLANES, SIZES, LODS, FDIM, MULTI, W1, B1, W2, B2, HIDDEN = range(3, 13)
G_PLANES, G_W1, G_B1, G_W2, G_B2, LOSS, SCRATCH, SCRATCH_BYTES, STREAM = range(13, 22)


def _sizes(sizes):
    return (ctypes.c_int32 * max(len(sizes), 1))(*sizes)


def _scratch_bytes(n, sizes, F, multi, hidden, lods=None):
    import wisp._C as C
    return int(C.lib.wisp_triplane_sdf_train_scratch_bytes(n, ctypes.cast(_sizes(sizes), ctypes.c_void_p), len(sizes) if lods is None else lods,
                                                           F, multi, hidden))


def _host_args(sizes=(33,), F=4, multi=1, hidden=128, n=8):
    """a call whose sizes are valid and whose pointers point at host memory: nothing may be dereferenced on the way to a refusal
    (planes, sizes and grad_planes are host arrays by contract)"""
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    L = len(sizes)
    pl = (ctypes.c_void_p * max(3 * L, 1))(*([ptr.value] * (3 * L)))
    gpl = (ctypes.c_void_p * max(3 * L, 1))(*([ptr.value] * (3 * L)))
    sz = _sizes(sizes)
    need = _scratch_bytes(n, sizes, F, multi, hidden)
    args = [ptr, ptr, n, pl, sz, L, F, multi, ptr, ptr, ptr, ptr, hidden, gpl] + [ptr] * 6 + [need, ctypes.c_void_p(0)]
    return args, (buf, pl, gpl, sz)


def test_argument_checks_are_returned_before_any_launch():
    """every refusal comes back as WISP_ERR_INVALID with a text, with host pointers in every slot: had anything been launched or
    dereferenced on the way, this process would not be here to say so"""
    import wisp._C as C
    f = C._cdll.wisp_triplane_sdf_train_step
    null = ctypes.c_void_p(0)
    args, keep = _host_args()
    assert args[SCRATCH_BYTES] > 0
    bad = [{FDIM: 0}, {FDIM: -1}, {FDIM: 17}, {FDIM: 2 ** 30}, {HIDDEN: 0}, {HIDDEN: 257}, {LODS: 0}, {LODS: 17}, {LODS: -1}, {N: 0},
           {N: -1}, {MULTI: 2}, {MULTI: -1}] + \
          [{k: null} for k in (COORDS, GTS, PLANES, SIZES, W1, B1, W2, B2, G_PLANES, G_W1, G_B1, G_W2, G_B2, LOSS, SCRATCH)]
    for patch in bad:
        args, keep = _host_args()
        for k, v in patch.items():
            args[k] = v
        assert f(*args) == -1, patch                                               # WISP_ERR_INVALID
        assert C.lib.wisp_last_error(), patch
    # 60 feature columns: 'cat' of 5 levels x 3 x 4 (the same planes are fine as a 'sum'; nothing is launched for them either: the
    # scratch is then a byte short)
    args, keep = _host_args(sizes=(3, 5, 9, 17, 33), multi=1)
    args[MULTI] = 0
    assert f(*args) == -1 and b"48 feature columns" in C.lib.wisp_last_error()
    args, keep = _host_args(sizes=(9, 0, 33))
    assert f(*args) == -1 and b"plane size" in C.lib.wisp_last_error()
    args, keep = _host_args(sizes=(9, 17))
    args[PLANES][4] = None
    assert f(*args) == -1 and b"null plane" in C.lib.wisp_last_error()
    args, keep = _host_args(sizes=(9, 17))
    args[G_PLANES][5] = None
    assert f(*args) == -1 and b"null plane gradient" in C.lib.wisp_last_error()
    # scratch one byte short - at the shipped shape, at the largest one, and where a plane takes the f32 atomics
    for shape in (dict(), dict(sizes=(5, 9, 17, 33), F=4, multi=0, hidden=256), dict(sizes=(9, 129), F=4, multi=0, hidden=17),
                  dict(sizes=(3, 5, 9, 17, 33), multi=1)):
        args, keep = _host_args(**shape)
        assert args[SCRATCH_BYTES] > 0, shape
        args[SCRATCH_BYTES] -= 1
        assert f(*args) == -1 and b"scratch too small" in C.lib.wisp_last_error(), shape


def test_scratch_bytes_is_exact_monotone_and_rejects_what_the_step_does_not_serve():
    for sizes, F, multi, hidden in (((33,), 4, 1, 128), ((5, 9, 17, 33), 4, 0, 256), ((9, 129), 4, 0, 17)):
        got = [_scratch_bytes(n, sizes, F, multi, hidden) for n in (1, 2, 16, 17, 512, 513, 5000, 1 << 16, 1 << 20)]
        assert got[0] > 0 and all(b >= a for a, b in zip(got, got[1:])) and got[-1] > got[0], (sizes, got)
    assert _scratch_bytes(512, (33,), 4, 1, 256) > _scratch_bytes(512, (33,), 4, 1, 128)
    # one partial row per workgroup of 16 samples, rows padded to 16 floats, and an fp64 accumulator for every entry of the three
    # planes: nglod_triplanar.yaml at 512 coordinates
    row = (128 * 15 + 2 * 128 + 2 + 15) // 16 * 16
    assert _scratch_bytes(512, (33,), 4, 1, 128) == 32 * row * 4 + 3 * 4 * 33 * 33 * 8
    assert _scratch_bytes(1 << 20, (33,), 4, 1, 128) == 1024 * row * 4 + 3 * 4 * 33 * 33 * 8          # at most 1024 workgroups
    # a plane above 2^16 entries has no accumulators: 4 x 129 x 129 = 66564; 4 x 128 x 128 = 2^16 still has them
    row = (17 * 27 + 2 * 17 + 2 + 15) // 16 * 16
    assert _scratch_bytes(16, (9, 129), 4, 0, 17) == row * 4 + 3 * 4 * 81 * 8
    assert _scratch_bytes(16, (9, 128), 4, 0, 17) == row * 4 + 3 * 4 * (81 + 128 * 128) * 8
    for bad in ((0, (33,), 4, 1, 128), (-1, (33,), 4, 1, 128), (512, (33,), 0, 1, 128), (512, (33,), 17, 1, 128), (512, (33,), 4, 2, 128),
                (512, (33,), 4, 1, 0), (512, (33,), 4, 1, 257), (512, (3, 5, 9, 17, 33), 4, 0, 128), (512, (9, 0), 4, 1, 128),
                (512, (5,) * 17, 1, 1, 128)):
        assert _scratch_bytes(*bad) == -1, bad
    assert _scratch_bytes(512, (33,), 4, 1, 128, lods=0) == -1
    import wisp._C as C
    assert int(C.lib.wisp_triplane_sdf_train_scratch_bytes(512, ctypes.c_void_p(0), 1, 4, 1, 128)) == -1
    assert _scratch_bytes(512, (5, 9, 17, 33), 4, 0, 256) > 0 and _scratch_bytes(512, (5,) * 16, 16, 1, 256) > 0    # the largest shapes


def step_lds_bytes(hidden, cols):
    """the dynamic LDS of triplane_sdf_train_kernel (csrc/sdf_step_dev.h: sdf_step_lds_bytes with 3 + cols floats a group), restated"""
    in_dim = 3 + cols
    stage = hidden * (in_dim | 1) + 2 * hidden + 16 * in_dim
    return 4 * (stage + 16 * (2 * hidden + 2 + cols) + hidden * in_dim + 2 * hidden + 2)


@pytest.mark.skipif(not kernel_meta.available(LIB), reason="libwisp_hip.so not built or llvm-readelf missing")
def test_the_two_kernels_have_no_scratch_and_the_largest_shape_fits_the_lds():
    meta = kernel_meta.kernels(LIB)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    for part in ("triplane_sdf_train_kernel", "triplane_sdf_train_reduce_kernel"):
        hits = {n: v for n, v in kern.items() if part + "(" in n}
        assert len(hits) == 1, (part, list(hits))
        for name, v in hits.items():
            assert v["scratch"] == 0 and v["wg"] == 256 and v["lds"] == 0 and v["vgpr"] + v["agpr"] <= 128, (name, v)
    # dynamic LDS only, raised past the 64 KB default; every admitted shape fits one workgroup's 160 KiB
    worst = max(step_lds_bytes(256, cols) for cols in range(3, 49, 3))
    assert worst == step_lds_bytes(256, 48) == 147784 and worst <= LDS_LIMIT
    assert step_lds_bytes(128, 12) == 35656                                       # nglod_triplanar.yaml


# ------------------------------------------------------------------------------------------------ 3. shape rules
def _cpu_nef(F=4, lods=1, multiscale='sum', hidden=32, base=3, positional=False):
    from wisp.models.grids import TriplanarGrid
    from wisp.models.nefs import NeuralSDF
    torch.manual_seed(3)
    grid = TriplanarGrid(None, feature_dim=F, log_base_resolution=base, num_lods=lods, multiscale_type=multiscale, feature_std=0.01)
    return NeuralSDF(grid, pos_embedder='positional' if positional else 'none', position_input=True, hidden_dim=hidden, num_layers=1)


def test_fused_field_takes_the_triplanar_branch_only_when_asked_and_only_for_its_shape(monkeypatch):
    """the rules on CPU objects that claim to live on the GPU (nothing is launched): every tensor answers is_cuda with True"""
    from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
    from wisp.trainers import SDFTrainStep
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED", raising=False)
    steps = dict(default=SDFTrainStep(_cpu_nef()), asked=SDFTrainStep(_cpu_nef(hidden=128, base=5), fused_triplane=True),
                 hash_only=SDFTrainStep(_cpu_nef(), fused_hash=True),
                 cat=SDFTrainStep(_cpu_nef(lods=2, multiscale='cat', F=2), fused_triplane=True),
                 all_lods=SDFTrainStep(_cpu_nef(), fused_triplane=True, only_last=False),
                 half=SDFTrainStep(_cpu_nef(), fused_triplane=True),
                 wide=SDFTrainStep(_cpu_nef(lods=5, multiscale='cat', base=1), fused_triplane=True),
                 embedded=SDFTrainStep(_cpu_nef(positional=True), fused_triplane=True),
                 tex=SDFTrainStep(NeuralSDFTex(_cpu_nef().grid, embedder_type='identity', hidden_dim=32, num_layers=1), fused_triplane=True))
    half = steps["half"].nef.grid.features[0].fmy                                    # (FlatParams homes parameters in f32: re-typed after)
    half.data, half.grad = half.data.half(), None
    half.grad = torch.zeros_like(half.data)
    assert steps["asked"]._fused_field() is None                                    # on the host nothing is fused
    steps["asked"]._fused_cache = None
    monkeypatch.setattr(torch.Tensor, "is_cuda", True, raising=False)
    assert not steps["default"].fused_triplane and steps["default"]._fused_field() is None
    assert not steps["hash_only"].fused_triplane and steps["hash_only"]._fused_field() is None
    ok = steps["asked"]._fused_field()
    nef = steps["asked"].nef
    vol = nef.grid.features[0]
    assert ok is not None and ok["triplane"] and not ok.get("hash") and ok["grid"] is nef.grid and ok["lods"] == 1 and ok["multiscale"] == 'sum'
    assert len(ok["prm"]) == 3 + 4 and [id(q) for q in ok["prm"][:3]] == [id(vol.fmx), id(vol.fmy), id(vol.fmz)]
    assert all(q.shape == (1, 4, 33, 33) for q in ok["prm"][:3]) and ok["prm"][3] is nef.decoder.layers[0].weight
    assert steps["asked"]._fused_field() is ok                                      # cached
    c = steps["cat"]._fused_field()
    assert c is not None and c["multiscale"] == 'cat' and len(c["prm"]) == 6 + 4
    for name in ("all_lods", "half", "wide", "embedded", "tex"):
        assert steps[name]._fused_field() is None, name
    assert steps["tex"].textured
    # what can change under a live trainer is looked at on every call
    assert steps["asked"]._fused_still_valid(ok)
    grad = vol.fmz.grad
    vol.fmz.grad = None
    assert not steps["asked"]._fused_still_valid(ok) and steps["asked"]._fused_field() is None
    vol.fmz.grad = grad
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
    assert "fused_triplane" not in {f.name for f in dataclasses.fields(ConfigSDFTrainer)}


# ------------------------------------------------------------------------------------------------ 4. the scripts
def test_train_nglod_wires_fused_kernel(monkeypatch):
    """--fused-kernel builds SDFTrainStep(..., fused_triplane=True) and its answer becomes the JSON record's fused_triplane_step;
    --help names the option; a hash grid refuses it; --grid triplanar --fused-step stays refused"""
    import types
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train_nglod
    finally:
        sys.path.pop(0)
    import wisp.trainers as T
    assert "There is no fused training step" not in train_nglod.__doc__ and "fused_triplane=True" in train_nglod.__doc__
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
    trainer = types.SimpleNamespace(pipeline=types.SimpleNamespace(nef=_cpu_nef()))
    assert train_nglod.fit_fused(trainer, ds, cfg, "cpu", fused_triplane=True) is False
    assert seen[-1]["fused_triplane"] is True and seen[-1]["fused_hash"] is False and seen[-1]["only_last"] is True
    assert train_nglod.fit_fused(trainer, ds, cfg, "cpu") is False
    assert seen[-1]["fused_triplane"] is False
    src = open(os.path.join(ROOT, "scripts", "train_nglod.py")).read()
    assert "fused_triplane_step=fused_triplane_step" in src
    script = os.path.join(ROOT, "scripts", "train_nglod.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--fused-kernel" in r.stdout and "--fused-step" in r.stdout
    for grid in ("hash", "octree"):
        r = subprocess.run([sys.executable, script, "mesh.obj", "--grid", grid, "--fused-kernel"], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--grid triplanar" in r.stderr, (grid, r.stderr[-500:])
    r = subprocess.run([sys.executable, script, "mesh.obj", "--grid", "triplanar", "--fused-step", "--fused-kernel"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--grid triplanar has no fused training step" in r.stderr


def test_bench_script_takes_the_triplanar_grid():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_hash_sdf_step.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "--grid {hash,triplanar}" in r.stdout
