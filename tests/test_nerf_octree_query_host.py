"""CPU: the host side of the fused field query of the octree family (csrc/nerf_octree_query.hip) - the entry point's declaration /
binding / export and argument validation, the kernel's resources, the decoder definition it shares with nerf_query.hip, the path
selection (nerf_octree_query_supported, the tracer's routing), the decoded-table cache of CodebookOctreeGrid, the float64
reference of the GPU tests next to the oracle, and the render script's command line."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import nerf_octree_query_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kaolin-wisp_amd", "csrc")
ENTRY = "wisp_nerf_octree_query"
OK, INVALID, UNSUPPORTED = 0, -1, -3
SWITCH = "WISP_NERF_OCTREE_QUERY_FUSED"


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_entry_point_is_declared_bound_and_exported():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    kinds = {C.c_vp: "p", C.c_i64: "l", C.c_i32: "i", C.c_f32: "f"}
    assert f"int {ENTRY}(" in header and ENTRY in C.SIGNATURES
    decl = header[header.index(f"int {ENTRY}("):]
    decl = decl[decl.index("(") + 1:decl.index(");")]
    got = []
    for arg in decl.split(","):
        arg = arg.split("/*")[0].strip()
        got.append("p" if "*" in arg or arg.startswith("wisp_stream_t") else "l" if arg.startswith("int64_t") else
                   "f" if arg.startswith("float") else "i")
    assert got == [kinds[a] for a in C.SIGNATURES[ENTRY]] and len(got) == 24
    comment = header[header.index("The inference query of an octree-backed radiance field"):header.index(f"int {ENTRY}(")]
    assert "nerf.py:219-264" in comment and "octree_grid.py:165-219" in comment
    assert hasattr(ctypes.CDLL(C.LIB_PATH), ENTRY)
    assert C.lib.wisp_abi_version() == C.ABI_VERSION == 4                            # an added entry point does not bump it
    assert ENTRY in header[header.index("Entry points that are only ADDED"):header.index("int wisp_abi_version(void);")]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "nerf_octree_query.hip" in mk and "octree_nerf_eval_dev.h" in mk
    assert callable(C.nerf_octree_query)


# ------------------------------------------------------------------------------------------------ 2. argument validation
def _args(**over):
    """a valid argument list for the nerf_octree.yaml shape (F = 5, four levels 5..8 of a level-8 octree, 'sum'), with dummy non-null
    pointers (validation fails before any is read)"""
    buf = ctypes.create_string_buffer(256)
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)                                         # 16-byte aligned, as the trinkets must be
    a = dict(coords=p, dirs=p, ridx=None, num_rays=0, n=512, octree=p, exsum=p, points=p, trinkets=p, max_level=8,
             feats=(ctypes.c_void_p * 4)(p.value, p.value, p.value, p.value), dtype_feats=0,
             levels=(ctypes.c_int32 * 4)(5, 6, 7, 8), num_lods=4, feature_dim=5, half_round=1, sum=1, params=p, dtype_params=0,
             in_dim=5, hidden=64, rgb=p, density=p)
    a.update(over)
    a["_keep_alive"] = buf
    return a


def _call(a):
    import wisp._C as C
    lib = ctypes.CDLL(C.LIB_PATH)
    fn = getattr(lib, ENTRY)
    fn.argtypes = C.SIGNATURES[ENTRY]
    fn.restype = ctypes.c_int

    def ptr(x):
        return None if x is None else x if isinstance(x, ctypes.c_void_p) else ctypes.cast(x, ctypes.c_void_p)
    rc = fn(a["coords"], a["dirs"], a["ridx"], a["num_rays"], a["n"], a["octree"], a["exsum"], a["points"], a["trinkets"],
            a["max_level"], ptr(a["feats"]), a["dtype_feats"], ptr(a["levels"]), a["num_lods"], a["feature_dim"], a["half_round"],
            a["sum"], a["params"], a["dtype_params"], a["in_dim"], a["hidden"], a["rgb"], a["density"], None)
    return rc, C.last_error()


def test_the_shipped_shapes_pass_validation_with_nothing_to_do():
    for over in (dict(), dict(sum=0, in_dim=20), dict(feature_dim=16, in_dim=16), dict(feature_dim=8, sum=0, in_dim=32),
                 dict(feature_dim=1, in_dim=1), dict(dtype_feats=1), dict(dtype_feats=2), dict(num_lods=1), dict(half_round=0)):
        assert _call(_args(n=0, **over))[0] == OK, over


@pytest.mark.parametrize("over", [dict(feature_dim=0, in_dim=0), dict(feature_dim=17, in_dim=17), dict(num_lods=0), dict(num_lods=17),
                                  dict(hidden=128), dict(hidden=32), dict(in_dim=6), dict(in_dim=20), dict(sum=0, in_dim=5),
                                  dict(sum=0, feature_dim=9, in_dim=36), dict(sum=0, feature_dim=16, in_dim=64),
                                  dict(dtype_feats=3), dict(dtype_feats=-1), dict(dtype_params=1), dict(dtype_params=2)])
def test_unsupported_shapes_are_refused_before_any_launch(over):
    rc, msg = _call(_args(**over))
    assert rc == UNSUPPORTED and "nerf_octree_query" in msg and "hidden 64" in msg
    rc, _ = _call(_args(n=0, **over))
    assert rc == UNSUPPORTED                                                         # whatever the sample count


@pytest.mark.parametrize("name", ["coords", "dirs", "octree", "exsum", "points", "trinkets", "feats", "levels", "params"])
def test_null_pointers_are_invalid(name):
    rc, msg = _call(_args(**{name: None}))
    assert rc == INVALID and "null pointer" in msg
    rc, _ = _call(_args(n=0, **{name: None}))
    assert rc == OK                                                                  # nothing to do, nothing read


def test_output_and_ray_index_pointers():
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _call(_args(rgb=None, density=None))[0] == INVALID                        # nothing to write
    rc, msg = _call(_args(ridx=p, dirs=None, num_rays=4))
    assert rc == INVALID and ("ray_dirs" in msg or "null pointer" in msg)            # ridx given without ray_dirs
    rc, msg = _call(_args(ridx=p, dirs=None, num_rays=4, rgb=None))
    assert rc == INVALID and "ray_dirs" in msg                                       # ... also when only the density is asked for
    assert _call(_args(ridx=p, num_rays=0))[0] == INVALID                            # rays to index, none given
    assert _call(_args(ridx=p, num_rays=0, n=0))[0] == OK


def test_other_invalid_arguments_and_the_empty_call():
    a = _args()
    odd = ctypes.c_void_p(a["trinkets"].value + 4)
    null_table = (ctypes.c_void_p * 4)(a["coords"].value, a["coords"].value, None, a["coords"].value)
    for over in (dict(n=-1), dict(max_level=16), dict(max_level=-1), dict(max_level=7),          # the last level lies below it
                 dict(levels=(ctypes.c_int32 * 4)(5, 7, 6, 8)), dict(levels=(ctypes.c_int32 * 4)(5, 6, 6, 8)),
                 dict(levels=(ctypes.c_int32 * 4)(-1, 6, 7, 8)), dict(feats=null_table), dict(trinkets=odd)):
        rc, _ = _call(_args(**over))
        assert rc == INVALID, over
    assert _call(_args(n=0))[0] == OK
    assert _call(_args(n=0, rgb=None, density=None))[0] == OK


def test_the_python_wrapper_refuses_cpu_tensors():
    import wisp._C as C
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        C.nerf_octree_query(torch.zeros(8, 3), torch.zeros(8, 3), None, torch.zeros(1, dtype=torch.uint8),
                            torch.zeros(2, dtype=torch.int32), torch.zeros(1, 3, dtype=torch.int16),
                            torch.zeros(1, 8, dtype=torch.int32), 0, [torch.zeros(8, 5)], [0], True, True, torch.zeros(10), 5, 64)


# ------------------------------------------------------------------------------------------------ 3. the kernel
def test_kernel_resources():
    """all six forms (three table dtypes, with and without the colour half): workgroup 256 (4 waves, one per SIMD), no scratch, no
    static LDS, and a dynamic LDS size - restated here from the file's own constants - within the CU's 160 KB"""
    import kernel_meta
    import wisp._C as C
    meta = kernel_meta.kernels(C.LIB_PATH)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    hits = {n: v for n, v in kern.items() if "nerf_octree_query_kernel<" in n}
    assert len(hits) == 6, list(hits)
    src = open(os.path.join(CSRC, "nerf_octree_query.hip")).read()
    dev = open(os.path.join(CSRC, "octree_nerf_eval_dev.h")).read()
    waves = int(re.search(r"constexpr int NOQ_WAVES = (\d+);", src).group(1))
    assert waves == 4
    for name, v in hits.items():
        assert v["scratch"] == 0 and v["wg"] == waves * 64 and v["vgpr"] <= 512 and v["lds"] == 0, (name, v)
    IN, H, LDI, LDH = 32, 64, 33, 65
    weights = H * LDI + 32 * LDH + H * LDH + H * LDH + 32 * LDH
    biases = 3 * H + 64
    per_wave = 64 * LDI + 2 * 32 * LDH                                               # x0 and the two aliased activation tiles
    assert (weights + biases + waves * per_wave) * 4 <= 160 * 1024
    assert "static_assert(NOQ_LDS_BYTES <= 160 * 1024" in src
    for word in ("printf", "assert(", "atomic"):
        assert word not in src.replace("static_assert(", "") and word not in dev, word


def test_both_query_kernels_expand_one_decoder_definition():
    """nerf_octree_query.hip carries no layer of its own: it expands the stage macros of nerf_mlp_f32_dev.h in the order
    nerf_query.hip expands them, over the same staging functions; its lookup takes the weights from sdf_eval_coeffs"""
    query, octree = (open(os.path.join(CSRC, f)).read() for f in ("nerf_query.hip", "nerf_octree_query.hip"))
    dev = open(os.path.join(CSRC, "octree_nerf_eval_dev.h")).read()
    stage = re.compile(r"\b(WISP_F32_[A-Z0-9_]+|f32_stage_[a-z_]+)\(")

    def sequence(text):
        body = text[text.index("__global__"):]
        return stage.findall(body[:body.index("\n}\n")])
    assert sequence(query) == sequence(octree) and len(sequence(octree)) == 8
    for macro in ("WISP_F32_VIEW_ENCODE", "WISP_F32_LAYER1", "WISP_F32_LAYER2", "WISP_F32_LAYER_HIDDEN", "WISP_F32_LAYER5"):
        assert macro + "(" in octree, macro
    for text in (octree, dev):
        assert "#define WISP_F32" not in text and "mfma" not in text and "sinf(" not in text and "expf(" not in text
    assert '#include "nerf_mlp_f32_dev.h"' in octree and '#include "octree_nerf_eval_dev.h"' in octree
    assert '#include "sdf_eval_dev.h"' in dev and "sdf_eval_coeffs(" in dev and "#pragma clang fp contract(off)" in dev
    assert "1.0f - " not in dev                                                      # no third copy of the weights
    # one spelling of the blend and of the fp16 rounding of a level's result in the query and in the modular lookups it must equal
    interp = open(os.path.join(CSRC, "spc_interp.hip")).read()
    lookups = interp[interp.index("spc_trilinear_fwd_kernel("):interp.index('extern "C" int wisp_spc_trilinear_multi_fwd')]
    assert lookups.count("__builtin_fmaf(fv, w[j], acc") == 3 and lookups.count("wisp_round_through_f16(acc") == 3
    assert "fv * w[j]" not in lookups and "__float2half_rn(acc" not in lookups
    assert "__builtin_fmaf(fv, w[j], acc[c])" in dev and "wisp_round_through_f16(acc[c])" in dev


# ------------------------------------------------------------------------------------------------ 4. path selection
def _cpu_nef(kind="octree", multiscale='sum', hidden=64, bias=False, interpolation='linear', bitwidth=4, feature_dim=5, level=3):
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import CodebookOctreeGrid, OctreeGrid
    from wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(0)
    shape = dict(feature_dim=feature_dim, num_lods=4, interpolation_type=interpolation, multiscale_type=multiscale, feature_std=0.1)
    blas = OctreeAS.make_dense(level)
    grid = CodebookOctreeGrid(blas, codebook_bitwidth=bitwidth, **shape) if kind == "codebook" else OctreeGrid(blas, **shape)
    nef = NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=hidden, num_layers=1, bias=bias,
                              prune_density_decay=None, prune_min_density=None)
    return nef.eval()


@pytest.fixture
def as_if_on_the_gpu(monkeypatch):
    """every tensor reports is_cuda: the one property of the selection that a CPU box cannot satisfy"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setenv(SWITCH, "1")                             # the switch's default is off
    monkeypatch.delenv("WISP_NERF_QUERY_FUSED", raising=False)


@pytest.mark.parametrize("kind", ["octree", "codebook"])
def test_the_unmodified_fields_are_selected(kind, as_if_on_the_gpu):
    """the nerf_octree.yaml / nerf_codebook.yaml shapes: F = 5, 4 LODs, 'sum', bias-free decoders"""
    from wisp.ops.nerf_mlp import nerf_octree_query_supported, nerf_query_supported
    nef = _cpu_nef(kind)
    assert nerf_octree_query_supported(nef) and not nerf_query_supported(nef)
    for lod_idx in range(4):
        assert nerf_octree_query_supported(nef, lod_idx) and not nerf_query_supported(nef, lod_idx)
    assert nerf_octree_query_supported(_cpu_nef(kind, bias=True))
    cat = _cpu_nef(kind, multiscale='cat')
    assert nerf_octree_query_supported(cat) and nerf_octree_query_supported(cat, 3) and not nerf_query_supported(cat)
    assert nerf_octree_query_supported(_cpu_nef(kind, multiscale='cat', feature_dim=8))          # 32 columns
    assert not nerf_octree_query_supported(_cpu_nef(kind, multiscale='cat', feature_dim=9))      # 36


@pytest.mark.parametrize("kind", ["octree", "codebook"])
@pytest.mark.parametrize("case", ["switch", "switch_unset", "cat_below_last", "closest", "hidden128", "autocast", "half_decoder", "cpu", "bad_lod",
                                  "bf16_compute", "unfused_decoder", "codebook_training", "baked", "half_dictionary",
                                  "large_dictionary"])
def test_every_disqualifying_case_is_refused(kind, case, as_if_on_the_gpu, monkeypatch):
    from wisp.ops.nerf_mlp import nerf_octree_query_supported
    codebook_only = case in ("codebook_training", "baked", "half_dictionary", "large_dictionary")
    if codebook_only and kind != "codebook":
        kind = "codebook"                                                           # (the same check twice costs nothing)
    nef = _cpu_nef(kind, multiscale='cat' if case == "cat_below_last" else 'sum', hidden=128 if case == "hidden128" else 64,
                   interpolation='closest' if case == "closest" else 'linear', bitwidth=9 if case == "large_dictionary" else 4)
    lod_idx = None
    if case != "large_dictionary":
        assert nerf_octree_query_supported(nef, 3 if case == "cat_below_last" else None) == (case not in ("closest", "hidden128"))
    if case == "switch":
        monkeypatch.setenv(SWITCH, "0")
    elif case == "switch_unset":
        monkeypatch.delenv(SWITCH)
    elif case == "cat_below_last":
        lod_idx = 2
    elif case == "bf16_compute":
        nef.decoder_compute = 'bf16'
    elif case == "unfused_decoder":
        nef.fused_decoder = False
    elif case == "cpu":
        monkeypatch.undo()                            # tensors say where they are again
        monkeypatch.setenv(SWITCH, "1")
    elif case == "autocast":
        monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    elif case == "half_decoder":
        nef.decoder_color.lout.weight.data = nef.decoder_color.lout.weight.data.half()      # the LAST of the ten tensors
    elif case == "bad_lod":
        lod_idx = 4
    elif case == "codebook_training":
        nef.train()
    elif case == "baked":
        nef.grid.bake()
        assert nef.grid.features[0].ndim == 1
    elif case == "half_dictionary":
        nef.grid.dictionary[2].data = nef.grid.dictionary[2].data.half()
    assert not nerf_octree_query_supported(nef, lod_idx)


def test_fused_nerf_octree_query_refuses_gradients_and_cpu_fields():
    from wisp.ops.nerf_mlp import fused_nerf_octree_query
    for kind in ("octree", "codebook"):
        nef = _cpu_nef(kind)
        coords, dirs = torch.zeros(4, 3), torch.zeros(4, 3)
        with pytest.raises(NotImplementedError, match="no backward"):
            fused_nerf_octree_query(nef, coords, ray_d=dirs)                         # the parameters require a gradient
        with pytest.raises(NotImplementedError, match="no backward"):
            fused_nerf_octree_query(nef.requires_grad_(False), coords.clone().requires_grad_(True), ray_d=dirs)
        nef.requires_grad_(False)
        with pytest.raises(RuntimeError, match="must be a GPU tensor"):
            fused_nerf_octree_query(nef, coords, ray_d=dirs)                         # a field on the CPU: no fallback
        with torch.no_grad(), pytest.raises(RuntimeError, match="must be a GPU tensor"):
            fused_nerf_octree_query(nef.requires_grad_(True), coords, ray_d=dirs)
        with torch.no_grad():
            with pytest.raises(ValueError):
                fused_nerf_octree_query(nef, coords, ray_d=dirs, ray_dirs=dirs, ridx=torch.zeros(4, dtype=torch.int64))
            with pytest.raises(ValueError):
                fused_nerf_octree_query(nef, coords, ray_dirs=dirs)


def _traced_with(tracer, nef, monkeypatch, grad=False, extra=()):
    """runs tracer.trace over stubs of everything behind the query; returns which query the call took"""
    import wisp.ops.nerf_mlp as ops
    import wisp.ops.render as render_ops
    import wisp.tracers._fused_trace as fused_trace
    from wisp.core import Rays
    taken = []
    monkeypatch.setattr(fused_trace, "supports", lambda *a, **k: False)              # (the one-node training trace: not the subject)

    def stub(name):
        def fused(nef_, coords, ray_d=None, ray_dirs=None, ridx=None, lod_idx=None, want_rgb=True, pad_rows=0):
            taken.append(name)
            assert ray_d is None and ray_dirs.shape == (3, 3) and ridx.shape == (5,) and lod_idx == nef.grid.num_lods - 1
            return torch.zeros(5, 3), torch.zeros(5, 1)
        return fused
    monkeypatch.setattr(ops, "fused_nerf_query", stub("hash"))
    monkeypatch.setattr(ops, "fused_nerf_octree_query", stub("octree"))
    monkeypatch.setattr(render_ops, "composite", lambda *a, **k: (torch.zeros(3, 3), torch.zeros(3, 1), None, torch.zeros(3, dtype=torch.bool)))
    rm = types.SimpleNamespace(ridx=torch.tensor([0, 0, 2, 2, 2]), samples=torch.zeros(5, 3), deltas=torch.ones(5, 1),
                               depth_samples=torch.ones(5, 1), boundary=None, ray_offsets=torch.tensor([0, 2, 2, 5]), pack_info=None)
    monkeypatch.setattr(nef.grid, "raymarch", lambda *a, **k: rm)

    def modular(*a, **k):
        taken.append("modular")
        return torch.zeros(5, 3), torch.zeros(5, 1)
    monkeypatch.setattr(type(nef), "forward", lambda self, *a, **k: modular(*a, **k))
    rays = Rays(torch.zeros(3, 3), torch.ones(3, 3), dist_min=0.0, dist_max=1.0)
    with torch.set_grad_enabled(grad):
        if extra:
            with pytest.raises(Exception):
                tracer.trace(nef, rays, {"rgb"}, set(extra))                         # (the stub field has no such channel)
        else:
            tracer.trace(nef, rays, {"rgb"}, set())
    return taken


@pytest.mark.parametrize("kind", ["octree", "codebook"])
def test_tracer_takes_the_octree_route_for_these_fields_only(kind, as_if_on_the_gpu, monkeypatch):
    from wisp.tracers import PackedRFTracer
    nef = _cpu_nef(kind).requires_grad_(False)
    tracer = PackedRFTracer(raymarch_type='voxel', num_steps=4)
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]                     # attribute absent: today's path
    tracer.fused_query = False
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]
    tracer.fused_query = True
    assert _traced_with(tracer, nef, monkeypatch) == ["octree"]
    assert _traced_with(tracer, nef, monkeypatch, grad=True)[:1] != ["octree"]       # gradients enabled
    assert "octree" not in _traced_with(tracer, nef, monkeypatch, extra=("normal",))  # an extra channel
    monkeypatch.setenv("WISP_NERF_QUERY_FUSED", "0")                                  # the hash query's switch is not this one's
    assert _traced_with(tracer, nef, monkeypatch) == ["octree"]
    monkeypatch.setenv(SWITCH, "0")
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]
    monkeypatch.delenv(SWITCH)                                                       # unset: off
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]
    if kind == "codebook":
        monkeypatch.setenv(SWITCH, "1")
        nef.train()
        assert _traced_with(tracer, nef, monkeypatch) == ["modular"]


def test_tracer_keeps_the_hash_route_for_hash_grids(as_if_on_the_gpu, monkeypatch):
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralRadianceField
    from wisp.tracers import PackedRFTracer
    torch.manual_seed(0)
    grid = HashGrid.from_geometric(OctreeAS.make_dense(2), feature_dim=2, num_lods=6, multiscale_type='cat', feature_std=0.1,
                                   codebook_bitwidth=12, min_grid_res=4, max_grid_res=64)
    nef = NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=64, num_layers=1, bias=True)
    nef = nef.requires_grad_(False)
    tracer = PackedRFTracer(raymarch_type='ray', num_steps=4)
    tracer.fused_query = True
    assert _traced_with(tracer, nef, monkeypatch) == ["hash"]
    monkeypatch.setenv("WISP_NERF_QUERY_FUSED", "0")
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]                     # and the octree predicate refuses a HashGrid


# ------------------------------------------------------------------------------------------------ 5. the decoded-table cache
def test_decoded_tables_are_rebuilt_after_a_parameter_update_and_not_otherwise(monkeypatch):
    import wisp._C as C
    from wisp.ops.grid import note_raw_parameter_write
    calls = []

    def decode(logits, dictionary, training):
        calls.append((logits.data_ptr(), bool(training)))
        return torch.from_numpy(ref.decoded_rows(logits.numpy(), dictionary.numpy())).clone()
    monkeypatch.setattr(C, "codebook_decode_rows", decode)
    nef = _cpu_nef("codebook")
    grid = nef.grid
    first = grid.decoded_tables()
    assert len(first) == 4 and len(calls) == 4 and not any(t for _, t in calls)      # one decode per level, eval-mode rows
    assert all(t.shape == (f.shape[0], 5) and t.dtype == torch.float32 and not t.requires_grad for t, f in zip(first, grid.features))
    assert all(a is b for a, b in zip(first, grid.decoded_tables())) and len(calls) == 4          # unchanged: not rebuilt
    nef.train(); nef.eval()                                                           # noqa: E702 - a mode change alone is no update
    assert all(a is b for a, b in zip(first, grid.decoded_tables())) and len(calls) == 4
    # neither a parameter nor a buffer, and absent from state_dict
    names = [n for n, _ in nef.named_parameters()] + [n for n, _ in nef.named_buffers()] + list(nef.state_dict())
    assert not any("decoded" in n for n in names) and "_decoded_cache" in grid.__dict__
    state = {k: v.clone() for k, v in nef.state_dict().items()}
    # an optimizer step (in place: `_version` moves)
    opt = torch.optim.SGD([grid.features[1], grid.dictionary[2]], lr=1.0)
    grid.features[1].grad = torch.randn_like(grid.features[1])
    grid.dictionary[2].grad = torch.ones_like(grid.dictionary[2])
    opt.step()
    second = grid.decoded_tables()
    assert len(calls) == 8 and not any(a is b for a, b in zip(first, second))
    assert torch.equal(second[2], first[2] - 1.0) and not torch.equal(second[1], first[1])
    assert all(a is b for a, b in zip(second, grid.decoded_tables())) and len(calls) == 8
    # load_state_dict (copies in place)
    nef.load_state_dict(state)
    third = grid.decoded_tables()
    assert len(calls) == 12 and all(torch.equal(a, b) for a, b in zip(first, third))
    # a new tensor behind a parameter (`data_ptr` moves)
    grid.dictionary[0].data = grid.dictionary[0].data + 1.0
    assert torch.equal(grid.decoded_tables()[0], first[0] + 1.0) and len(calls) == 16
    # a write that leaves the version counters alone, announced as the trainers' raw-pointer optimizer kernels are
    f = grid.features[3]
    version = f._version
    f.data.copy_(torch.flip(f.data, dims=[1]))
    assert f._version == version
    assert len(calls) == 16 and grid.decoded_tables() is not None and len(calls) == 16
    note_raw_parameter_write()
    assert not torch.equal(grid.decoded_tables()[3], first[3]) and len(calls) == 20


def test_the_flat_optimizer_announces_its_writes():
    """FlatParams.mark_shadow_current is what every raw-pointer optimizer path of the trainers calls after it rewrote parameters"""
    from wisp.ops.grid import raw_write_epoch
    from wisp.trainers.multiview_trainer import FlatParams
    nef = _cpu_nef("codebook")
    flat = FlatParams(nef)
    before = raw_write_epoch()
    flat.mark_shadow_current()
    assert raw_write_epoch() == before + 1


# ------------------------------------------------------------------------------------------------ 6. the float64 reference
def _oracle_blas(grid):
    t = ref.tree_of(grid)
    return types.SimpleNamespace(octree=t["octree"], exsum=t["exsum"], points=t["points"]), t


@pytest.mark.parametrize("multiscale", ['sum', 'cat'])
@pytest.mark.parametrize("kind", ["octree", "codebook"])
def test_reference_agrees_with_the_oracle(kind, multiscale):
    """features against oracle/octree_grid.py (float32 torch) and the whole field against the oracle's decoder classes, without
    autograd.  Bounds: the oracle evaluates the same expression in float32 - per level 8 products and 7 additions on weights that
    are products of three factors (16 roundings of 2^-24 relative to the largest table entry), plus the cell position
    2^level * fl(0.5 c + 0.5) - point, whose float32 rounding of 2^-24 is scaled by 2^level and enters through each of the three
    axes with a slope of at most twice the largest entry; the level sum adds the levels' bounds.  With half_features the two sides
    may round a blend to different fp16 neighbours: one fp16 spacing of the largest value per level on top.  The decoder is held to
    the project's fp32 parity bound (1e-4 on colours, 1e-4 of the largest density)."""
    from oracle import nerf as onerf, octree_grid as ogrid
    nef = _cpu_nef(kind, multiscale=multiscale, bias=True).requires_grad_(False)
    grid = nef.grid
    with torch.no_grad():
        for f in grid.features:
            f.mul_(5.0)
        for p in nef.decoder_density.parameters():
            p.mul_(2.0)
    blas, tree = _oracle_blas(grid)
    g = torch.Generator().manual_seed(1)
    coords = torch.rand(300, 3, generator=g) * 2.0 - 1.0
    coords[:4] = torch.tensor([[1.0, -1.0, 0.25], [1.5, 0.0, 0.0], [0.0, 0.0, 0.0], [-1.0, -1.0, -1.0]])
    dirs = torch.nn.functional.normalize(torch.randn(300, 3, generator=g), dim=1)
    levels = [int(l) for l in grid.active_lods]
    lods = [3] if multiscale == 'cat' else [0, 1, 3]
    eps = 2.0 ** -24
    for half in ([False] if kind == "codebook" else [False, True]):
        grid.half_features = half
        for lod_idx in lods:
            num = lod_idx + 1
            feats = [f.detach() for f in grid.features]
            if kind == "codebook":
                want = ogrid.codebook_grid_interpolate(blas, tree["trinkets"], feats, [d.detach() for d in grid.dictionary], coords,
                                                       lod_idx, levels, multiscale, 5, False)
                tables = [ref.decoded_rows(f.numpy(), d.detach().numpy()) for f, d in zip(feats, grid.dictionary)][:num]
            else:
                want = ogrid.octree_grid_interpolate(blas, tree["trinkets"], feats, coords, lod_idx, grid.base_lod, levels, multiscale,
                                                     5, half_round=half)
                tables = [f.numpy() for f in feats[:num]]
            got = ref.features64(tree, tables, levels[:num], coords.numpy(), half_round=half, sum_lods=multiscale == 'sum')
            assert got.shape == tuple(want.shape)
            top = max(float(np.abs(t).max()) for t in tables)
            per_level = top * (16 * eps + 3 * 2 * 2.0 ** levels[num - 1] * eps) + (top * 2.0 ** -10 if half else 0.0)
            bound = per_level * (num if multiscale == 'sum' else 1)
            err = float(np.abs(got - want.double().numpy()).max())
            assert err <= bound, (kind, multiscale, half, lod_idx, err, bound)
            assert float(np.abs(got).max()) > 100 * bound and (got[1] == 0.0).all()  # (the point outside the cube)
    grid.half_features = kind != "codebook"
    # the whole field: the oracle's decoders on the oracle's float32 features
    dd = onerf.OracleDecoder(nef.effective_feature_dim(), 16, 64, 1, True)
    dc = onerf.OracleDecoder(15 + 27, 3, 64, 2, True)
    dd.load_state_dict(nef.decoder_density.state_dict())
    dc.load_state_dict(nef.decoder_color.state_dict())
    with torch.no_grad():
        y = dd(want.float())
        rgb32 = torch.sigmoid(dc(torch.cat([y, onerf.positional_embed(dirs, 4)], -1)[..., 1:]))
        den32 = torch.relu(y[..., 0:1])
    rgb64, den64 = ref.field64(nef, coords, dirs, lods[-1])
    assert float(np.abs(rgb64 - rgb32.double().numpy()).max()) <= 1e-4
    assert float(np.abs(den64 - den32.double().numpy()).max()) <= 1e-4 * max(float(den32.max()), 1.0)
    assert float(den32.max()) > 0.0 and float(rgb32.std()) > 0.0
    none, den_only = ref.field64(nef, coords, None, lods[-1])
    assert none is None and np.array_equal(den_only, den64)


def test_reference_first_index_rule():
    logits = np.array([[0.0, 3.0, 3.0, 1.0], [2.0, 2.0, 2.0, 2.0], [-1.0, -5.0, -1.0, -7.0]], dtype=np.float32)
    dictionary = np.arange(8, dtype=np.float32).reshape(4, 2)
    assert np.array_equal(ref.decoded_rows(logits, dictionary), dictionary[[1, 0, 0]])
    assert torch.equal(torch.from_numpy(dictionary)[torch.max(torch.from_numpy(logits), dim=-1)[1]],
                       torch.from_numpy(ref.decoded_rows(logits, dictionary)))


# ------------------------------------------------------------------------------------------------ 7. the script
def test_render_script_help_names_the_grid_option():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_nerf.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for word in ("--grid", "hash", "octree", "codebook", "--octree-level", "--cloud-rays", "--no-fused"):
        assert word in out.stdout, word
    bench = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_nerf_eval.py"), "--help"], capture_output=True,
                           text=True, timeout=120)
    assert bench.returncode == 0 and "--grid" in bench.stdout, bench.stderr
