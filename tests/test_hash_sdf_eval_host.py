"""CPU: the host side of the fused hash-grid SDF evaluation (csrc/hash_sdf_eval.hip) - the exactness conditions of
tests/hash_sdf_eval_ref.py's generator, its float64 reference against oracle/hashgrid.py and against this package's NeuralSDF /
HashGrid shape and quirk rules, the three entry points' declaration / binding / export and argument checks, the kernels'
resources, the shape rules of PackedSDFTracer._fused_field / wisp.ops.sdf.fused_sdf_field, and the script's --grid option."""
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
from oracle import hashgrid as ohg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
ENTRIES = ("wisp_hash_sdf_query", "wisp_hash_sdf_fd_gradient", "wisp_hash_sdf_trace_step_fused")


# ------------------------------------------------------------------------------------------------ 1. the reference itself
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hidden,F,multiscale,lod_idx", [(1, 8, 'cat', 3), (17, 4, 'cat', 0), (128, 2, 'cat', 2), (256, 8, 'sum', 3),
                                                         (128, 4, 'sum', 1)])
def test_exact_query_cases_are_exact(hidden, F, multiscale, lod_idx, dtype):
    """float64 and float32 evaluation agree bit for bit (the generator's own assertions ran when the case was built)"""
    case = R.exact_case(hidden, F, multiscale, lod_idx, n=400, seed=5, dtype=dtype)
    fld, coords = case["field"], case["coords"]
    a, b = R.reference(fld, coords), R.reference(fld, coords, torch.float32)
    assert torch.equal(a, b.double()) and a.shape == (400, 1)
    dense = [ohg.level_is_dense(r, 2 ** R.EXACT_BITWIDTH) for r in R.EXACT_RES]
    assert dense == [True, True, False, False]                                       # two dense levels, two hashed
    face = coords[::5]
    assert bool(torch.equal(face * 16, torch.round(face * 16)))                     # every 5th point on a cell face
    feat = R.features(fld, coords)
    assert feat.shape == (400, R.num_cols(fld))
    if multiscale == 'cat':
        assert bool((feat[:, lod_idx * F:] == 0).all())
        assert lod_idx == 0 or int((feat[:, :lod_idx * F] != 0).sum()) > 100
    else:
        assert int((feat != 0).sum()) > 100


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hidden,multiscale", [(1, 'cat'), (128, 'sum'), (256, 'cat')])
def test_exact_gradient_cases_are_exact(hidden, multiscale, dtype):
    case = R.exact_gradient_case(hidden, 8, multiscale, 3, n=400, seed=6, dtype=dtype)
    a = R.gradient_reference(case["field"], case["coords"], case["eps"])
    b = R.gradient_reference(case["field"], case["coords"], case["eps"], torch.float32)
    assert torch.equal(a, b.double()) and int((a != 0).sum()) > (200 if hidden > 1 else 20)


def test_an_inexact_case_is_refused():
    fld = R.exact_field(128, seed=1)
    with pytest.raises(AssertionError):
        R.check_exact(fld, R.generic_points(50, seed=1), 12)
    with pytest.raises(AssertionError, match="clamp"):                              # a cell past MAX_CELL: the coarsest level clamps
        R.check_exact(fld, torch.tensor([[0.5, 0.0, 0.0]]), 12)
    half = R.exact_field(128, dtype=torch.bfloat16, seed=1)
    with pytest.raises(AssertionError, match="bfloat16"):                           # the f32 sub-grid under a bf16 table
        R.check_exact(half, R.exact_points(200, b=1, step=1, seed=3), 12)


@pytest.mark.parametrize("res", R.GENERIC_RES)
@pytest.mark.parametrize("multiscale,dtype", [('cat', torch.float32), ('sum', torch.float32), ('cat', torch.float16)])
def test_reference_equals_the_oracle_grid_and_a_torch_decoder(res, multiscale, dtype):
    """features against oracle.hashgrid.grid_interpolate (fp32 blend in corner order, pinned to the reference's kernels): the two
    differ by the fp32 rounding of the blend - g = 1 - f, two products, eight fma steps: under 16 * 2^-24 of the largest table
    entry per level ('sum': times the levels) - and, behind a half table dtype, by one unit of that dtype where the rounding
    falls the other way.  The decoder against torch.nn.Linear modules in float64 on the same features."""
    fld = R.generic_field(res, 128, F=8 if multiscale == 'cat' else 4, multiscale=multiscale, lod_idx=2, seed=4, dtype=dtype)
    coords = R.generic_points(600, seed=8)
    assert bool((coords.abs() > 1).any()) and bool((coords.abs() == 1).any())
    got = R.features(fld, coords)
    F = fld["table"].shape[1]
    want = ohg.grid_interpolate(coords, fld["lod_idx"], multiscale, F, fld["resolutions"], fld["bitwidth"], fld["table"],
                                fld["begin"]).double()
    top = float(fld["table"].float().abs().max())
    levels = len(res) if multiscale == 'sum' else 1
    bound = levels * (16 * 2.0 ** -24 * top if dtype == torch.float32 else 2.0 ** -10 * top)
    err = float((got - want).abs().max())
    assert got.shape == want.shape and err <= bound, (err, bound)
    if dtype != torch.float32:                                                      # ... and almost everywhere none at all
        assert float(((got - want).abs() > 16 * 2.0 ** -24 * top).double().mean()) < 0.01
    lin1 = torch.nn.Linear(3 + R.num_cols(fld), 128).double()
    lin2 = torch.nn.Linear(128, 1).double()
    with torch.no_grad():
        lin1.weight.copy_(fld["w1"]); lin1.bias.copy_(fld["b1"]); lin2.weight.copy_(fld["w2"].reshape(1, -1)); lin2.bias.copy_(fld["b2"])
        out = lin2(torch.relu(lin1(torch.cat([coords.double(), got], 1))))
    assert float((R.reference(fld, coords) - out).abs().max()) <= 1e-13


def _cpu_nef(F=8, lods=4, multiscale='cat', hidden=32, bitwidth=12, coord_dim=3, positional=False, pos=True, layers=1,
             resolutions=None):
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralSDF
    torch.manual_seed(3)
    if resolutions is not None:
        grid = HashGrid.from_resolutions(None, feature_dim=F, resolutions=resolutions, multiscale_type=multiscale, feature_std=0.05,
                                         codebook_bitwidth=bitwidth, coord_dim=coord_dim)
    else:
        grid = HashGrid.from_geometric(None, feature_dim=F, num_lods=lods, multiscale_type=multiscale, feature_std=0.05,
                                       codebook_bitwidth=bitwidth, min_grid_res=16, max_grid_res=2048, coord_dim=coord_dim)
    return NeuralSDF(grid, pos_embedder='positional' if positional else 'none', position_input=pos, hidden_dim=hidden,
                     num_layers=layers)


def ref_field_of(nef, lod_idx):
    """the reference's view (CPU tensors) of a NeuralSDF(HashGrid)'s parameters at lod_idx"""
    g, dec = nef.grid, nef.decoder
    return dict(table=g.codebook.feats.detach().cpu(), begin=g.codebook.begin_idxes.cpu(), resolutions=[int(r) for r in g.resolutions],
                bitwidth=int(g.codebook_bitwidth), multiscale=g.multiscale_type, lod_idx=int(lod_idx),
                w1=dec.layers[0].weight.detach().float().cpu(), b1=dec.layers[0].bias.detach().float().cpu(),
                w2=dec.lout.weight.detach().float().cpu().reshape(-1), b2=dec.lout.bias.detach().float().cpu())


def test_package_field_shapes_and_the_cat_quirk():
    """this package's NeuralSDF over a HashGrid, built on the host (its interpolation needs a device): the table layout, the
    decoder's input width and the resolutions are what the reference model is fed with, and the reference follows the 'cat' rule
    of HashGrid.interpolate - at lod_idx 0 the position alone decides, at the last level the last level's rows do not matter"""
    nef = _cpu_nef()
    g = nef.grid
    assert g.resolutions == [16, 80, 406, 2048] and g.num_lods == 4 and g.codebook_size == 4096
    _, begin = ohg.table_layout(g.resolutions, 4096)
    assert g.codebook.begin_idxes.tolist() == begin.tolist() and g.codebook.feats.shape == (int(begin[-1]), 8)
    assert nef.decoder.layers[0].in_features == 3 + 32 and nef.decoder.lout.out_features == 1
    assert _cpu_nef(multiscale='sum').decoder.layers[0].in_features == 3 + 8
    coords = R.generic_points(200, seed=2)
    f0 = ref_field_of(nef, 0)
    assert R.zero_from_col(f0) == 0 and bool((R.features(f0, coords) == 0).all())
    moved = dict(f0, table=f0["table"] + 1.0)
    assert torch.equal(R.reference(f0, coords), R.reference(moved, coords))
    last = ref_field_of(nef, 3)
    assert R.zero_from_col(last) == 24
    table = last["table"].clone()
    table[int(begin[3]):] += 1.0                                                    # the last level's rows
    assert torch.equal(R.reference(last, coords), R.reference(dict(last, table=table), coords))
    table = last["table"].clone()
    table[int(begin[2]):int(begin[3])] += 1.0
    assert not torch.equal(R.reference(last, coords), R.reference(dict(last, table=table), coords))
    s = ref_field_of(_cpu_nef(multiscale='sum'), 1)                                 # 'sum' takes every level whatever lod_idx
    assert R.zero_from_col(s) == 32 and torch.equal(R.reference(s, coords), R.reference(dict(s, lod_idx=3), coords))


# ------------------------------------------------------------------------------------------------ 2. ABI and argument checks
def test_the_three_entry_points_are_declared_bound_and_exported():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    for name in ENTRIES:
        assert f"int {name}(" in header and name in C.SIGNATURES
    assert "hash_grid.py:205-233" in header and "gradients.py:29-45" in header and "packed_sdf_tracer.py:118-146" in header
    field = 14                                                                      # codebook .. hidden
    assert len(C.SIGNATURES["wisp_hash_sdf_query"]) == 2 + field + 4
    assert len(C.SIGNATURES["wisp_hash_sdf_fd_gradient"]) == 2 + field + 3
    assert len(C.SIGNATURES["wisp_hash_sdf_trace_step_fused"]) == 18 + field + 3
    # argument by argument against the declaration: pointer / int64 / int / float
    kinds = {C.c_vp: "p", C.c_i64: "l", C.c_i32: "i", C.c_f32: "f"}
    for name in ENTRIES:
        decl = header[header.index(f"int {name}("):]
        decl = decl[decl.index("(") + 1:decl.index(");")]
        got = []
        for arg in decl.split(","):
            arg = arg.split("/*")[0].strip()
            got.append("p" if "*" in arg or arg.startswith("wisp_stream_t") else "l" if arg.startswith("int64_t") else
                       "f" if arg.startswith("float") else "i")
        assert got == [kinds[a] for a in C.SIGNATURES[name]], name
    lib = ctypes.CDLL(C.LIB_PATH)
    assert all(hasattr(lib, name) for name in ENTRIES)
    assert C.lib.wisp_abi_version() == 4 == C.ABI_VERSION
    assert callable(C.hash_sdf_trace_step_fused) and callable(C.sdf_trace_step_field)
    mk = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "Makefile")).read()
    assert "hash_sdf_eval.hip" in mk and "hash_sdf_eval_dev.h" in mk
    with pytest.raises(ValueError, match="kind"):
        C.sdf_query(None, dict(kind="triplanar"))


# positions in the <hash field> part of the argument lists
CODEBOOK, DTYPE, BEGIN, RES, LODS, FDIM, BITS, MULTI, ZERO, W1, B1, W2, B2, HIDDEN = range(14)


def _host_args(entry, resolutions=(16, 80, 406, 2048), F=8, bits=12, multi=0):
    """a call whose sizes are valid and whose pointers point at host memory: nothing may be dereferenced on the way to a refusal
    (begin_idxes and resolutions are host arrays by contract)"""
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    n = len(resolutions)
    _, begin = ohg.table_layout(resolutions, 2 ** bits)
    bi = (ctypes.c_int64 * (n + 1))(*[int(b) for b in begin])
    rs = (ctypes.c_int32 * max(n, 1))(*resolutions)
    field = [ptr, 0, bi, rs, n, F, bits, multi, n * F, ptr, ptr, ptr, ptr, 128]
    if entry == "query":
        args, at = [ptr, 8] + field + [ptr, ptr, ptr, ctypes.c_void_p(0)], 2
    elif entry == "gradient":
        args, at = [ptr, 8] + field + [ctypes.c_float(0.005), ptr, ctypes.c_void_p(0)], 2
    else:
        args = [8, 0] + [ptr] * 4 + [ctypes.c_float(6.0), ctypes.c_float(3e-4), ctypes.c_float(1.5e-3)] + [ptr] * 9
        args, at = args + field + [ctypes.c_float(0.8), ctypes.c_void_p(0), ctypes.c_void_p(0)], 18
    return args, at, (buf, bi, rs)


@pytest.mark.parametrize("entry", ["query", "gradient", "trace"])
def test_argument_checks_are_returned_before_any_launch(entry):
    import wisp._C as C
    f = getattr(C._cdll, dict(query=ENTRIES[0], gradient=ENTRIES[1], trace=ENTRIES[2])[entry])
    null = ctypes.c_void_p(0)
    bad = [{FDIM: 3}, {FDIM: 16}, {FDIM: 0}, {HIDDEN: 0}, {HIDDEN: 257}, {DTYPE: 3}, {DTYPE: -1}, {LODS: 0}, {LODS: 17}, {MULTI: 2},
           {BITS: 0}, {BITS: 31}, {ZERO: -1}, {CODEBOOK: null}, {BEGIN: null}, {RES: null}, {W1: null}, {B1: null}, {W2: null}, {B2: null}]
    for patch in bad:
        args, at, keep = _host_args(entry)
        for k, v in patch.items():
            args[at + k] = v
        assert f(*args) == -1, patch                                               # WISP_ERR_INVALID
        assert C.lib.wisp_last_error()
    # 40 feature columns: 'cat' of 5 levels x 8 - and the same table is fine as a 'sum' (8 columns)
    args, at, keep = _host_args(entry, resolutions=(4, 8, 16, 32, 64))
    assert f(*args) == -1 and b"32 feature columns" in C.lib.wisp_last_error()
    # a resolution below 1; a level with fewer rows than a hashed index reaches
    args, at, keep = _host_args(entry, resolutions=(16, 0, 406, 2048))
    assert f(*args) == -1
    args, at, keep = _host_args(entry)
    args[at + BEGIN][4] -= 1
    assert f(*args) == -1 and b"fewer rows" in C.lib.wisp_last_error()
    head = dict(query=[{1: -1}, {0: null}, {2 + 14: null, 2 + 16: null}, {2 + 15: null}],       # n, coords, nothing to write, counts without gts
                gradient=[{1: -1}, {0: null}, {2 + 14: ctypes.c_float(0.0)}, {2 + 14: ctypes.c_float(-1.0)}, {2 + 15: null}],  # eps, grad
                trace=[{0: -1}] + [{i: null} for i in (2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 15, 16, 17)])[entry]
    for patch in head:
        args, at, keep = _host_args(entry)
        for k, v in patch.items():
            args[k] = v
        assert f(*args) == -1, patch
    # an empty batch is fine with nothing but the field described ... but the shape checks still come first
    args, at, keep = _host_args(entry)
    if entry == "trace":
        args[0] = 0
        for i in (2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 15, 16, 17):
            args[i] = null
    else:
        args[0], args[1] = null, 0
        args[2 + 14 if entry == "query" else 2 + 15] = null
    assert f(*args) == 0
    args[at + FDIM] = 3
    assert f(*args) == -1


@pytest.mark.skipif(not kernel_meta.available(LIB), reason="libwisp_hip.so not built or llvm-readelf missing")
def test_the_kernels_have_no_scratch_and_fit_four_waves_a_simd():
    """workgroup 256, no scratch, no static LDS, at most 128 VGPRs: four waves share a SIMD's 512 registers"""
    meta = kernel_meta.kernels(LIB)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    for part in ("hash_sdf_point_query_kernel<", "hash_sdf_point_gradient_kernel<", "hash_sdf_march_kernel<"):
        hits = {n: v for n, v in kern.items() if part in n}
        assert len(hits) == 3, (part, list(hits))                                   # f32 / f16 / bf16 tables
        for name, v in hits.items():
            assert v["scratch"] == 0 and v["wg"] == 256 and v["vgpr"] + v["agpr"] <= 128 and v["lds"] == 0, (name, v)


# ------------------------------------------------------------------------------------------------ 3. shape rules
class _CudaLike(torch.Tensor):
    is_cuda = True


def _on_gpu(nef):
    """the shape rules ask for tables on the GPU: a stand-in that says so (nothing is launched here)"""
    cb = nef.grid.codebook
    table = cb.feats.detach().as_subclass(_CudaLike)
    del cb._parameters["feats"]
    cb.feats = table
    return nef


def test_fused_field_accepts_the_nglod_hash_shape_and_nothing_else(monkeypatch):
    from wisp.ops.sdf import fused_sdf_field
    from wisp.tracers import PackedSDFTracer
    nef = _on_gpu(_cpu_nef(hidden=128, bitwidth=19))                                # nglod_hash.yaml
    ok = fused_sdf_field(nef, None)
    assert ok is not None and ok["kind"] == "hash" and ok["multiscale"] == "cat" and ok["zero_from_col"] == 24
    assert ok["resolutions"] == [16, 80, 406, 2048] and ok["feature_dim"] == 8 and ok["codebook_bitwidth"] == 19
    assert ok["begin_idxes"] == nef.grid.codebook.begin_idxes.tolist() and ok["codebook"].shape == nef.grid.codebook.feats.shape
    assert ok["w1"].shape == (128, 35) and ok["b1"].shape == (128,) and ok["w2"].shape == (128,) and ok["b2"].shape == (1,)
    assert torch.equal(ok["w1"], nef.decoder.layers[0].weight) and torch.equal(ok["w2"], nef.decoder.lout.weight.reshape(-1))
    assert [fused_sdf_field(nef, l)["zero_from_col"] for l in range(4)] == [0, 8, 16, 24]       # lod_idx 0 is served
    assert PackedSDFTracer._fused_field(nef, 2)["zero_from_col"] == 16
    s = fused_sdf_field(_on_gpu(_cpu_nef(multiscale='sum')), 1)
    assert s["multiscale"] == "sum" and s["zero_from_col"] == 32 and s["w1"].shape == (32, 11)
    assert fused_sdf_field(_on_gpu(_cpu_nef(F=2, lods=16)), 15)["w1"].shape == (32, 35)
    assert fused_sdf_field(_on_gpu(_cpu_nef(hidden=256)), 3) is not None
    for name, bad, lod in (("feature_dim 16", _cpu_nef(F=16, lods=2), 1), ("40 columns", _cpu_nef(F=8, lods=5), 4),
                           ("17 levels", _cpu_nef(F=2, lods=17, multiscale='sum'), 16),
                           ("2-D", _cpu_nef(coord_dim=2), 3), ("fourier", _cpu_nef(positional=True), 3),
                           ("no position", _cpu_nef(pos=False), 3), ("two layers", _cpu_nef(layers=2), 3),
                           ("hidden 300", _cpu_nef(hidden=300), 3), ("lod_idx out of range", _cpu_nef(), 4)):
        assert fused_sdf_field(_on_gpu(bad), lod) is None, name
    assert fused_sdf_field(_cpu_nef(), 3) is None                                   # tables on the host
    from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
    tex = NeuralSDFTex(_cpu_nef().grid, embedder_type='identity', hidden_dim=32, num_layers=1)
    assert fused_sdf_field(_on_gpu(tex), 3) is None                                 # textured over a hash grid: out of scope
    monkeypatch.setenv("WISP_SDF_FUSED", "0")
    assert fused_sdf_field(nef, 3) is None


def test_an_octree_field_yields_the_dict_it_always_did():
    import test_sdf_eval_host as octree_host
    from wisp.ops.sdf import fused_sdf_field
    nef = octree_host._cpu_field()
    got = fused_sdf_field(nef, 2)
    g, dec = nef.grid, nef.decoder
    want = dict(feats=[g.features[i].detach().contiguous() for i in range(3)], levels=[int(l) for l in g.active_lods[:3]],
                half_round=bool(g.half_features), w1=dec.layers[0].weight.detach().float().contiguous(),
                b1=dec.layers[0].bias.detach().float().contiguous(), w2=dec.lout.weight.detach().float().reshape(-1).contiguous(),
                b2=dec.lout.bias.detach().float().contiguous(), octree=g.blas.octree, exsum=g.blas.prefix, points=g.blas.points,
                trinkets=g.trinkets.int().contiguous())
    assert list(got) == list(want) and "kind" not in got
    for k, v in want.items():
        if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            assert all(torch.equal(a, b) for a, b in zip(got[k], v)), k
        elif isinstance(v, torch.Tensor):
            assert torch.equal(got[k], v) and got[k].dtype == v.dtype, k
        else:
            assert got[k] == v, k
    assert fused_sdf_field(nef, 0) is None                                          # the octree path keeps its lod_idx >= 1 rule


def test_train_nglod_help_lists_the_grid_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_nglod.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--grid {octree,hash}" in r.stdout and "--codebook-bitwidth" in r.stdout
