"""CPU: the host side of the fused field query of a triplanar radiance field (csrc/nerf_triplane_query.hip over the kernel of
csrc/nerf_field_query_dev.h) - the entry point's declaration / binding / export and argument validation, the kernel's resources, the
path selection (nerf_triplane_query_supported, the tracer's routing), the float64 reference of the GPU tests next to the oracle,
the exactness of every exact case the GPU file uses, and the scripts' command lines."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import nerf_triplane_query_ref as ref
import triplane_sdf_eval_ref as tri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kaolin-wisp_amd", "csrc")
ENTRY = "wisp_nerf_triplane_query"
OK, INVALID, UNSUPPORTED = 0, -1, -3
SWITCH = "WISP_NERF_TRIPLANE_QUERY_FUSED"

EXACT_CASES, COUNTS, exact_case_inputs = ref.EXACT_CASES, ref.COUNTS, ref.exact_case_inputs


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
    assert got == [kinds[a] for a in C.SIGNATURES[ENTRY]] and len(got) == 18
    comment = header[header.index("The inference query of a triplanar radiance field"):header.index(f"int {ENTRY}(")]
    assert "nerf.py:219-264" in comment and "triplanar_grid.py:97-146" in comment
    assert hasattr(ctypes.CDLL(C.LIB_PATH), ENTRY)
    assert C.lib.wisp_abi_version() == C.ABI_VERSION == 4                            # an added entry point does not bump it
    assert ENTRY in header[header.index("Entry points that are only ADDED"):header.index("int wisp_abi_version(void);")]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "nerf_triplane_query.hip" in mk and "nerf_field_query_dev.h" in mk and "triplane_sdf_eval_dev.h" in mk
    assert callable(C.nerf_triplane_query)


# ------------------------------------------------------------------------------------------------ 2. argument validation
def _args(**over):
    """a valid argument list for the nerf_triplanar.yaml shape (F = 4, planes of 33 .. 257 texels a side, 'sum'), with dummy non-null
    pointers (validation fails before any is read)"""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    a = dict(coords=p, dirs=p, ridx=None, num_rays=0, n=512, planes=(ctypes.c_void_p * 48)(*([p.value] * 48)),
             sizes=(ctypes.c_int32 * 16)(33, 65, 129, 257, *([9] * 12)), num_lods=4, feature_dim=4, sum=1, params=p, dtype_params=0,
             in_dim=12, hidden=64, rgb=p, density=p, feats_out=None)
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
    rc = fn(a["coords"], a["dirs"], a["ridx"], a["num_rays"], a["n"], ptr(a["planes"]), ptr(a["sizes"]), a["num_lods"],
            a["feature_dim"], a["sum"], a["params"], a["dtype_params"], a["in_dim"], a["hidden"], a["rgb"], a["density"],
            a["feats_out"], None)
    return rc, C.last_error()


def test_the_shipped_shapes_pass_validation_with_nothing_to_do():
    for over in (dict(), dict(sum=0, num_lods=2, in_dim=24), dict(feature_dim=10, in_dim=30), dict(feature_dim=1, in_dim=3),
                 dict(num_lods=1), dict(num_lods=16), dict(sum=0, num_lods=2, feature_dim=5, in_dim=30),
                 dict(sum=0, num_lods=10, feature_dim=1, in_dim=30), dict(sizes=(ctypes.c_int32 * 16)(*([1] * 16)))):
        assert _call(_args(n=0, **over))[0] == OK, over


@pytest.mark.parametrize("over", [dict(num_lods=0), dict(num_lods=17), dict(num_lods=-1), dict(feature_dim=0, in_dim=0),
                                  dict(feature_dim=-1, in_dim=-3), dict(in_dim=11), dict(in_dim=48), dict(sum=0, in_dim=12),
                                  dict(feature_dim=11, in_dim=33), dict(sum=0, num_lods=3, in_dim=36),
                                  dict(sum=0, num_lods=16, in_dim=192), dict(hidden=128), dict(hidden=32), dict(dtype_params=1),
                                  dict(dtype_params=2), dict(dtype_params=-1),
                                  dict(sizes=(ctypes.c_int32 * 16)(33, 0, 129, 257, *([9] * 12))),
                                  dict(sizes=(ctypes.c_int32 * 16)(33, 65, 129, -5, *([9] * 12)))])
def test_unsupported_shapes_are_refused_before_any_launch(over):
    rc, msg = _call(_args(**over))
    assert rc == UNSUPPORTED and "nerf_triplane_query" in msg and "hidden 64" in msg
    rc, _ = _call(_args(n=0, **over))
    assert rc == UNSUPPORTED                                                         # whatever the sample count


@pytest.mark.parametrize("name", ["coords", "dirs", "planes", "sizes", "params"])
def test_null_pointers_are_invalid(name):
    rc, msg = _call(_args(**{name: None}))
    assert rc == INVALID and "null pointer" in msg
    rc, _ = _call(_args(n=0, **{name: None}))
    assert rc == OK                                                                  # nothing to do, nothing read


def test_output_ray_index_and_plane_pointers():
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _call(_args(rgb=None, density=None))[0] == INVALID                        # nothing to write
    assert _call(_args(rgb=None, density=None, feats_out=p))[0] == INVALID           # (the feature rows alone are no result)
    rc, msg = _call(_args(ridx=p, dirs=None, num_rays=4))
    assert rc == INVALID and ("ray_dirs" in msg or "null pointer" in msg)            # ridx given without ray_dirs
    rc, msg = _call(_args(ridx=p, dirs=None, num_rays=4, rgb=None))
    assert rc == INVALID and "ray_dirs" in msg                                       # ... also when only the density is asked for
    assert _call(_args(ridx=p, num_rays=0))[0] == INVALID                            # rays to index, none given
    assert _call(_args(ridx=p, num_rays=0, n=0))[0] == OK
    assert _call(_args(n=-1))[0] == INVALID
    for hole in (0, 5, 11):                                                          # a null plane among the 12 in use
        planes = (ctypes.c_void_p * 48)(*([p.value] * 48))
        planes[hole] = None
        rc, msg = _call(_args(planes=planes))
        assert rc == INVALID and "null plane" in msg
    planes = (ctypes.c_void_p * 48)(*([p.value] * 48))
    planes[12] = None                                                                # behind the levels in use: not looked at
    assert _call(_args(planes=planes, n=0))[0] == OK
    assert _call(_args(n=0))[0] == OK
    assert _call(_args(n=0, rgb=None, density=None))[0] == OK


def test_the_python_wrapper_refuses_cpu_tensors():
    import wisp._C as C
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        C.nerf_triplane_query(torch.zeros(8, 3), torch.zeros(8, 3), None, [torch.zeros(1, 4, 5, 5)] * 3, [5], 4, True,
                              torch.zeros(10), 12, 64)


# ------------------------------------------------------------------------------------------------ 3. the kernel
def test_kernel_resources():
    """both forms (with and without the colour half): workgroup 256 (4 waves, one per SIMD), no scratch, no static LDS, and a
    dynamic LDS size - restated here from the header's own constants - no larger than the sibling's (nerf_octree_query.hip)"""
    import kernel_meta
    import wisp._C as C
    meta = kernel_meta.kernels(C.LIB_PATH)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    hits = {n: v for n, v in kern.items() if "nerf_field_query_kernel<" in n and "TriNerfEnc" in n}
    assert len(hits) == 2, list(hits)
    hdr = open(os.path.join(CSRC, "nerf_field_query_dev.h")).read()
    src = open(os.path.join(CSRC, "nerf_triplane_query.hip")).read()
    waves = int(re.search(r"constexpr int NFQ_WAVES = (\d+);", hdr).group(1))
    assert waves == 4
    for name, v in hits.items():
        assert v["scratch"] == 0 and v["wg"] == waves * 64 and v["vgpr"] <= 512 and v["lds"] == 0, (name, v)
    IN, H, LDI, LDH = 32, 64, 33, 65
    weights = H * LDI + 32 * LDH + H * LDH + H * LDH + 32 * LDH
    biases = 3 * H + 64
    per_wave = 64 * LDI + 2 * 32 * LDH                                               # x0 and the two aliased activation tiles
    sibling = (weights + biases + 4 * per_wave) * 4                                  # NOQ_LDS_BYTES of nerf_octree_query.hip
    assert (weights + biases + waves * per_wave) * 4 <= sibling <= 160 * 1024
    assert "static_assert(NFQ_LDS_BYTES <= 160 * 1024" in hdr
    layout = lambda text, tag: re.sub(r"\s+", " ", text[text.index(f"constexpr int {tag}_B1"):text.index(f"constexpr size_t {tag}_LDS_BYTES")])
    octree = open(os.path.join(CSRC, "nerf_octree_query.hip")).read()
    assert layout(hdr, "NFQ") == layout(octree, "NOQ").replace("NOQ", "NFQ")         # the same layout, constant for constant
    for word in ("printf", "assert(", "atomic"):
        assert word not in src.replace("static_assert(", "") and word not in hdr.replace("static_assert(", ""), word


def test_the_kernel_expands_the_shared_decoder_and_the_shared_encoder():
    """the header carries no layer of its own: it expands the stage macros of nerf_mlp_f32_dev.h in the order nerf_octree_query.hip
    expands them, over the same staging functions; the encoder calls tri_sdf_blend of triplane_sdf_eval_dev.h and spells no weight"""
    hdr, octree, src = (open(os.path.join(CSRC, f)).read() for f in ("nerf_field_query_dev.h", "nerf_octree_query.hip",
                                                                      "nerf_triplane_query.hip"))
    stage = re.compile(r"\b(WISP_F32_[A-Z0-9_]+|f32_stage_[a-z_]+)\(")

    def sequence(text):
        body = text[text.index("__global__"):]
        return stage.findall(body[:body.index("\n}\n")])
    assert sequence(hdr) == sequence(octree) and len(sequence(hdr)) == 8
    for text in (hdr, src):
        assert "#define WISP_F32" not in text and "mfma" not in text and "sinf(" not in text and "expf(" not in text
    assert '#include "nerf_mlp_f32_dev.h"' in hdr
    assert '#include "triplane_sdf_eval_dev.h"' in src and '#include "nerf_field_query_dev.h"' in src
    assert "tri_sdf_blend(" in src and "#pragma clang fp contract(off)" in src
    assert "1.0f - " not in src and "fmaf" not in src and "wisp_reflect_source_index(" not in src.split("struct TriNerfEnc {")[1].split("};")[0]
    assert "nerf_field_query_launch<TriNerfEnc>" in src and "WISP_ALLOW_LDS(" in hdr


# ------------------------------------------------------------------------------------------------ 4. path selection
def _cpu_nef(multiscale='sum', hidden=64, bias=True, interpolation='linear', feature_dim=4, lods=4, base=2, pos_embedder='none'):
    from wisp.accelstructs import AxisAlignedBBoxAS
    from wisp.models.grids import TriplanarGrid
    from wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(0)
    grid = TriplanarGrid(AxisAlignedBBoxAS(), feature_dim=feature_dim, log_base_resolution=base, num_lods=lods,
                         interpolation_type=interpolation, multiscale_type=multiscale, feature_std=0.1)
    nef = NeuralRadianceField(grid, pos_embedder=pos_embedder, view_embedder='positional', view_multires=4, hidden_dim=hidden,
                              num_layers=1, bias=bias, prune_density_decay=None, prune_min_density=None)
    return nef.eval()


@pytest.fixture
def as_if_on_the_gpu(monkeypatch):
    """every tensor reports is_cuda: the one property of the selection that a CPU box cannot satisfy"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setenv(SWITCH, "1")                             # the tests set the switch themselves, whatever its default
    monkeypatch.delenv("WISP_NERF_QUERY_FUSED", raising=False)
    monkeypatch.setenv("WISP_NERF_OCTREE_QUERY_FUSED", "1")


def test_the_unmodified_fields_are_selected(as_if_on_the_gpu):
    """the nerf_triplanar.yaml shape (F = 4, 4 LODs, 'sum') and the widest ones"""
    from wisp.ops.nerf_mlp import nerf_octree_query_supported, nerf_query_supported, nerf_triplane_query_supported
    nef = _cpu_nef(base=5)
    assert nerf_triplane_query_supported(nef) and not nerf_query_supported(nef) and not nerf_octree_query_supported(nef)
    for lod_idx in range(4):
        assert nerf_triplane_query_supported(nef, lod_idx)
    assert nerf_triplane_query_supported(_cpu_nef(bias=False))
    cat = _cpu_nef(multiscale='cat', lods=2)
    assert nerf_triplane_query_supported(cat) and nerf_triplane_query_supported(cat, 1)
    assert nerf_triplane_query_supported(_cpu_nef(multiscale='cat', feature_dim=5, lods=2))      # 30 columns
    assert nerf_triplane_query_supported(_cpu_nef(feature_dim=10, lods=2))                       # 30 columns
    assert not nerf_triplane_query_supported(_cpu_nef(feature_dim=11, lods=2))                   # 33
    assert not nerf_triplane_query_supported(_cpu_nef(multiscale='cat', feature_dim=4, lods=3))  # 36


@pytest.mark.parametrize("case", ["switch", "cat_below_last", "closest", "hidden128", "autocast", "half_decoder", "cpu", "bad_lod",
                                  "negative_lod", "bf16_compute", "unfused_decoder", "half_planes", "strided_plane", "cpu_plane",
                                  "pos_embedder", "octree_grid"])
def test_every_disqualifying_case_is_refused(case, as_if_on_the_gpu, monkeypatch):
    from wisp.ops.nerf_mlp import nerf_triplane_query_supported
    multiscale = 'cat' if case == "cat_below_last" else 'sum'
    nef = _cpu_nef(multiscale=multiscale, lods=2 if multiscale == 'cat' else 4, hidden=128 if case == "hidden128" else 64,
                   interpolation='closest' if case == "closest" else 'linear',
                   pos_embedder='positional' if case == "pos_embedder" else 'none')
    lod_idx = None
    assert nerf_triplane_query_supported(nef) == (case not in ("closest", "hidden128", "pos_embedder"))
    if case == "switch":
        monkeypatch.setenv(SWITCH, "0")
    elif case == "cat_below_last":
        lod_idx = 0
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
    elif case == "negative_lod":
        lod_idx = -1
    elif case == "half_planes":
        nef.grid.features[3].fmz.data = nef.grid.features[3].fmz.data.half()                # the LAST of the twelve planes
        assert nerf_triplane_query_supported(nef, 2)                                        # (not among the levels 0..2)
    elif case == "strided_plane":
        v = nef.grid.features[1].fmy
        v.data = torch.randn(1, 4, 9, 18)[..., ::2]
        assert tuple(v.shape) == (1, 4, 9, 9) and not v.is_contiguous()
    elif case == "cpu_plane":
        monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: self is not nef.grid.features[0].fmx), raising=False)
    elif case == "octree_grid":
        from wisp.accelstructs import OctreeAS
        from wisp.models.grids import OctreeGrid
        nef.grid = OctreeGrid(OctreeAS.make_dense(2), feature_dim=12, num_lods=2, multiscale_type='sum', feature_std=0.1)
    assert not nerf_triplane_query_supported(nef, lod_idx)


def test_the_switch_default_is_what_the_documents_say(monkeypatch):
    """the default is decided by the measurement of profiles/bench_nerf_triplanar_eval.json: on only if in every row the slowest
    fused repetition beat the fastest modular one"""
    import json
    import wisp.ops.nerf_mlp as ops
    rec = json.loads(open(os.path.join(ROOT, "profiles", "bench_nerf_triplanar_eval.json")).read().splitlines()[-1])
    rows = list(rec["query"].values()) + list(rec["view"].values())
    assert len(rows) == 4
    won = all(r["fused_max_below_modular_min"] and r["fused_ms_max"] < r["modular_ms_min"] for r in rows)
    assert ops._TRIPLANE_QUERY_DEFAULT == ("1" if won else "0")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.delenv(SWITCH, raising=False)
    assert ops.nerf_triplane_query_supported(_cpu_nef()) == won
    doc = ops.nerf_triplane_query_supported.__doc__
    assert ("default is on" in doc) == won and ("default is off" in doc) == (not won)


def test_fused_nerf_triplane_query_refuses_gradients_and_cpu_fields():
    from wisp.ops.nerf_mlp import fused_nerf_triplane_query
    nef = _cpu_nef()
    coords, dirs = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="no backward"):
        fused_nerf_triplane_query(nef, coords, ray_d=dirs)                           # the parameters require a gradient
    with pytest.raises(NotImplementedError, match="no backward"):
        fused_nerf_triplane_query(nef.requires_grad_(False), coords.clone().requires_grad_(True), ray_d=dirs)
    nef.requires_grad_(False)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        fused_nerf_triplane_query(nef, coords, ray_d=dirs)                           # a field on the CPU: no fallback
    with torch.no_grad(), pytest.raises(RuntimeError, match="must be a GPU tensor"):
        fused_nerf_triplane_query(nef.requires_grad_(True), coords, ray_d=dirs)
    with torch.no_grad():
        with pytest.raises(ValueError):
            fused_nerf_triplane_query(nef, coords, ray_d=dirs, ray_dirs=dirs, ridx=torch.zeros(4, dtype=torch.int64))
        with pytest.raises(ValueError):
            fused_nerf_triplane_query(nef, coords, ray_dirs=dirs)
        with pytest.raises(ValueError):
            fused_nerf_triplane_query(nef, coords)                                   # the colour needs a direction


def _traced_with(tracer, nef, monkeypatch, grad=False, extra=()):
    """runs tracer.trace over stubs of everything behind the query; returns which query the call took"""
    import wisp.ops.nerf_mlp as ops
    import wisp.ops.render as render_ops
    import wisp.tracers._fused_trace as fused_trace
    from wisp.core import Rays
    taken = []
    monkeypatch.setattr(fused_trace, "supports", lambda *a, **k: False)              # (the one-node training trace: not the subject)

    def stub(name):
        def fused(nef_, coords, ray_d=None, ray_dirs=None, ridx=None, lod_idx=None, want_rgb=True, pad_rows=0, want_feats=False):
            taken.append(name)
            assert ray_d is None and ray_dirs.shape == (3, 3) and ridx.shape == (5,) and lod_idx == nef.grid.num_lods - 1
            return torch.zeros(5, 3), torch.zeros(5, 1)
        return fused
    monkeypatch.setattr(ops, "fused_nerf_query", stub("hash"))
    monkeypatch.setattr(ops, "fused_nerf_octree_query", stub("octree"))
    monkeypatch.setattr(ops, "fused_nerf_triplane_query", stub("triplanar"))
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


def test_tracer_takes_the_triplanar_route_for_this_field_only(as_if_on_the_gpu, monkeypatch):
    from wisp.tracers import PackedRFTracer
    nef = _cpu_nef().requires_grad_(False)
    tracer = PackedRFTracer(raymarch_type='voxel', num_steps=4)
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]                     # attribute absent: today's path
    tracer.fused_query = False
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]
    tracer.fused_query = True
    assert _traced_with(tracer, nef, monkeypatch) == ["triplanar"]
    assert _traced_with(tracer, nef, monkeypatch, grad=True)[:1] != ["triplanar"]    # gradients enabled
    assert "triplanar" not in _traced_with(tracer, nef, monkeypatch, extra=("normal",))   # an extra channel
    monkeypatch.setenv("WISP_NERF_QUERY_FUSED", "0")                                  # the other queries' switches are not this one's
    monkeypatch.setenv("WISP_NERF_OCTREE_QUERY_FUSED", "0")
    assert _traced_with(tracer, nef, monkeypatch) == ["triplanar"]
    monkeypatch.setenv(SWITCH, "0")
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]


def test_tracer_asks_hash_first_then_octree_then_triplanar(as_if_on_the_gpu, monkeypatch):
    """the order of the three predicates, and that the first to accept decides: a hash grid and an octree grid keep their routes
    with all three switches on"""
    import wisp.ops.nerf_mlp as ops
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import HashGrid, OctreeGrid
    from wisp.models.nefs import NeuralRadianceField
    from wisp.tracers import PackedRFTracer
    torch.manual_seed(0)
    shape = dict(view_embedder='positional', view_multires=4, hidden_dim=64, num_layers=1, bias=True)
    hash_nef = NeuralRadianceField(HashGrid.from_geometric(OctreeAS.make_dense(2), feature_dim=2, num_lods=6, multiscale_type='cat',
                                                           feature_std=0.1, codebook_bitwidth=12, min_grid_res=4, max_grid_res=64),
                                   **shape).requires_grad_(False)
    octree_nef = NeuralRadianceField(OctreeGrid(OctreeAS.make_dense(3), feature_dim=5, num_lods=4, multiscale_type='sum',
                                                feature_std=0.1), prune_density_decay=None, prune_min_density=None,
                                     **shape).requires_grad_(False).eval()
    tracer = PackedRFTracer(raymarch_type='ray', num_steps=4)
    tracer.fused_query = True
    assert _traced_with(tracer, hash_nef, monkeypatch) == ["hash"]
    assert _traced_with(tracer, octree_nef, monkeypatch) == ["octree"]
    assert _traced_with(tracer, _cpu_nef().requires_grad_(False), monkeypatch) == ["triplanar"]
    asked = []
    for name in ("nerf_query_supported", "nerf_octree_query_supported", "nerf_triplane_query_supported"):
        monkeypatch.setattr(ops, name, lambda nef, lod_idx=None, name=name: asked.append(name) or False)
    with torch.no_grad():
        assert tracer._fused_query(_cpu_nef(), 3, set()) is None
    assert asked == ["nerf_query_supported", "nerf_octree_query_supported", "nerf_triplane_query_supported"]
    del asked[:]
    monkeypatch.setattr(ops, "nerf_octree_query_supported", lambda nef, lod_idx=None: asked.append("octree") or True)
    with torch.no_grad():
        assert tracer._fused_query(_cpu_nef(), 3, set()) is ops.fused_nerf_octree_query
    assert asked == ["nerf_query_supported", "octree"]                               # the triplanar predicate is not reached


# ------------------------------------------------------------------------------------------------ 5. the float64 reference
@pytest.mark.parametrize("multiscale", ['sum', 'cat'])
def test_reference_features_agree_with_the_oracle(multiscale):
    """features against oracle/triplanar.py (torch's fp32 CPU grid_sample) inside the bound tests/test_triplane_sdf_eval_host.py
    states: the planes have power-of-two spans, where grid_sample's source coordinate and the restated one are the same fp32 value,
    so the two differ by the fp32 rounding of the blend alone - under 8 * 2^-24 of the largest plane entry per level; 'sum' adds L
    levels with L - 1 more roundings of a sum of at most L entries: L (8 + L) * 2^-24"""
    from oracle import triplanar as otri
    nef = _cpu_nef(multiscale=multiscale, lods=2 if multiscale == 'cat' else 4, base=3).requires_grad_(False)
    with torch.no_grad():
        for p in nef.grid.parameters():
            p.mul_(5.0)
    coords = ref.generic_points(900, seed=8)
    assert bool((coords.abs() > 1).any()) and bool((coords.abs() == 1).any()) and float(coords.abs().max()) > 1.25
    vols = [(v.fmx.detach(), v.fmy.detach(), v.fmz.detach()) for v in nef.grid.features]
    for lod_idx in ([1] if multiscale == 'cat' else [0, 1, 3]):
        got = ref.features64(nef, coords, lod_idx)
        want = otri.interpolate(vols, coords, lod_idx, multiscale).double().numpy()
        L = lod_idx + 1
        top = max(float(p.abs().max()) for v in vols[:L] for p in v)
        bound = (8 if multiscale == 'cat' else L * (8 + L)) * 2.0 ** -24 * top
        err = float(np.abs(got - want).max())
        assert got.shape == want.shape == (900, 12 * (L if multiscale == 'cat' else 1)) and err <= bound, (multiscale, lod_idx, err, bound)
        assert float(np.abs(got).max()) > 1e4 * bound
        # and the package's own lookup arguments: TriplanarGrid hands the reference the planes in the order x, y, z per level
        fld = ref.planes_of(nef.grid, lod_idx)
        assert len(fld["planes"]) == 3 * L and all(torch.equal(a, b.reshape(a.shape)) for a, b in
                                                    zip(fld["planes"], [p for v in vols[:L] for p in v]))


@pytest.mark.parametrize("bias", [True, False])
def test_reference_field_agrees_with_the_oracle_decoder(bias):
    """the whole field: the oracle's decoder classes on the oracle's float32 features, held to the project's fp32 parity bound (1e-4
    on colours, 1e-4 of the largest density)"""
    from oracle import nerf as onerf, triplanar as otri
    nef = _cpu_nef(bias=bias, base=3).requires_grad_(False)
    with torch.no_grad():
        for p in nef.grid.parameters():
            p.mul_(5.0)
        for p in nef.decoder_density.parameters():
            p.mul_(2.0)
        nef.decoder_density.lout.weight[0].abs_()
    g = torch.Generator().manual_seed(1)
    coords = ref.generic_points(300, seed=3)
    dirs = torch.nn.functional.normalize(torch.randn(300, 3, generator=g), dim=1)
    vols = [(v.fmx.detach(), v.fmy.detach(), v.fmz.detach()) for v in nef.grid.features]
    want = otri.interpolate(vols, coords, 3, 'sum')
    dd = onerf.OracleDecoder(nef.effective_feature_dim(), 16, 64, 1, bias)
    dc = onerf.OracleDecoder(15 + 27, 3, 64, 2, bias)
    dd.load_state_dict(nef.decoder_density.state_dict())
    dc.load_state_dict(nef.decoder_color.state_dict())
    with torch.no_grad():
        y = dd(want.float())
        rgb32 = torch.sigmoid(dc(torch.cat([y, onerf.positional_embed(dirs, 4)], -1)[..., 1:]))
        den32 = torch.relu(y[..., 0:1])
    rgb64, den64 = ref.field64(nef, coords, dirs, 3)
    assert float(np.abs(rgb64 - rgb32.double().numpy()).max()) <= 1e-4
    assert float(np.abs(den64 - den32.double().numpy()).max()) <= 1e-4 * max(float(den32.max()), 1.0)
    assert float(den32.max()) > 0.0 and float(rgb32.std()) > 0.0
    none, den_only = ref.field64(nef, coords, None, 3)
    assert none is None and np.array_equal(den_only, den64)


@pytest.mark.parametrize("name", list(EXACT_CASES))
def test_every_exact_case_of_the_gpu_file_is_exact(name):
    """check_exact_features on the planes and positions the GPU file uses, at every sample count and every lod_idx it queries; and
    the consequence it is there for: a float32 evaluation of the reference equals the float64 one bit for bit"""
    F, multiscale, base, lods = EXACT_CASES[name]
    for n in COUNTS:
        planes, sizes, coords, bits = exact_case_inputs(name, n)
        assert len(planes) == 3 * lods and all(R in tri.EXACT_SIZES for R in sizes)
        for lod_idx in (range(lods) if multiscale == 'sum' else [lods - 1]):
            fld = dict(planes=planes[:3 * (lod_idx + 1)], multiscale=multiscale)
            ref.check_exact_features(fld, coords, bits)
            a, b = tri.features(fld, coords), tri.features(fld, coords, torch.float32)
            assert torch.equal(a, b.double()) and a.shape == (n, 3 * F * (1 if multiscale == 'sum' else lods))
    planes, sizes, coords, bits = exact_case_inputs(name, 700)
    c = coords.numpy()
    assert (np.abs(c) == 1.0).any() and (np.abs(c) > 1.0).any() and float(np.abs(c).max()) <= 1.5      # faces and reflected points
    ix = tri.source_index(c, sizes[0])
    assert (ix == np.floor(ix)).all(axis=1).sum() >= 700 // 5                                            # on texel lines
    assert int((tri.features(dict(planes=planes, multiscale=multiscale), coords) != 0).sum()) > 700


def test_check_exact_features_blames_inexact_inputs():
    planes, sizes, coords, bits = exact_case_inputs("f4_sum4", 65)
    fld = dict(planes=planes, multiscale='sum')
    ref.check_exact_features(fld, coords, bits)
    with pytest.raises(AssertionError, match="source coordinate|blend factor"):
        ref.check_exact_features(fld, coords + 1e-3, bits)
    with pytest.raises(AssertionError, match="-1 / 0 / 1"):
        ref.check_exact_features(dict(planes=[p * 0.3 for p in planes], multiscale='sum'), coords, bits)
    with pytest.raises(AssertionError, match="power of two"):
        ref.check_exact_features(dict(planes=[p[:, :4, :4] for p in planes[:3]], multiscale='sum'), coords, bits)


# ------------------------------------------------------------------------------------------------ 6. the scripts
def test_both_scripts_name_the_triplanar_grid():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_nerf.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for word in ("--grid", "triplanar", "nerf_triplanar.yaml", "--no-fused", "fused_query_route"):
        assert word in out.stdout, word
    bench = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_nerf_eval.py"), "--help"], capture_output=True,
                           text=True, timeout=120)
    assert bench.returncode == 0 and "triplanar" in bench.stdout, bench.stderr
