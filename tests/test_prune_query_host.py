"""CPU: the host side of the fused prune query (csrc/prune_query.hip) - the entry points' argument validation and error codes,
their declaration / binding / export, the kernels' resources, and the path selection of NeuralRadianceField.prune with the
native call stubbed."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("wisp_nerf_prune_query", "wisp_nerf_prune_query_debug")
OK, INVALID, UNSUPPORTED = 0, -1, -3


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_entry_points_are_declared_bound_and_exported():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    kinds = {C.c_vp: "p", C.c_i64: "l", C.c_i32: "i", C.c_f32: "f"}
    for name in ENTRIES:
        assert f"int {name}(" in header and name in C.SIGNATURES
        decl = header[header.index(f"int {name}("):]
        decl = decl[decl.index("(") + 1:decl.index(");")]
        got = []
        for arg in decl.split(","):
            arg = arg.split("/*")[0].strip()
            got.append("p" if "*" in arg or arg.startswith("wisp_stream_t") else "l" if arg.startswith("int64_t") else
                       "f" if arg.startswith("float") else "i")
        assert got == [kinds[a] for a in C.SIGNATURES[name]], name
    assert C.SIGNATURES[ENTRIES[1]][:-3] == C.SIGNATURES[ENTRIES[0]][:-1]           # the debug form adds (feats, density)
    lib = ctypes.CDLL(C.LIB_PATH)
    assert all(hasattr(lib, name) for name in ENTRIES)
    assert C.lib.wisp_abi_version() == C.ABI_VERSION == 4                            # added entry points do not bump it
    mk = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "Makefile")).read()
    assert "prune_query.hip" in mk and "nerf_mlp_f32_dev.h" in mk
    assert callable(C.nerf_prune_query)


# ------------------------------------------------------------------------------------------------ 2. argument validation
def _args(**over):
    """a valid argument list for the nerf_hash.yaml shape, with dummy non-null pointers (validation fails before any is read)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(points=p, unit=p, cells=512, level=3, table=p, dtype_table=0, feature_dim=2, coord_dim=3, first_idx=p,
             resolutions=(ctypes.c_int32 * 16)(*[16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512]), num_lods=16,
             bitwidth=19, zero_from_col=30, params=p, dtype_params=0, in_dim=32, hidden=64, occ_in=p, decay=0.95, min_density=1.0,
             occ_out=p, keep=p)
    a.update(over)
    a["_keep_alive"] = buf
    return a


def _call(a, debug=False, feats=None, density=None):
    import wisp._C as C
    lib = ctypes.CDLL(C.LIB_PATH)
    fn = getattr(lib, ENTRIES[1 if debug else 0])
    fn.argtypes = C.SIGNATURES[ENTRIES[1 if debug else 0]]
    fn.restype = ctypes.c_int
    res = a["resolutions"]
    head = [a["points"], a["unit"], a["cells"], a["level"], a["table"], a["dtype_table"], a["feature_dim"], a["coord_dim"],
            a["first_idx"], None if res is None else ctypes.cast(res, ctypes.c_void_p), a["num_lods"], a["bitwidth"],
            a["zero_from_col"], a["params"], a["dtype_params"], a["in_dim"], a["hidden"], a["occ_in"], a["decay"], a["min_density"],
            a["occ_out"], a["keep"]]
    if debug:
        head += [feats, density]
    return fn(*head, None), C.last_error()


@pytest.mark.parametrize("over", [dict(feature_dim=4), dict(coord_dim=2), dict(num_lods=17, in_dim=34), dict(num_lods=0, in_dim=0),
                                  dict(hidden=128), dict(hidden=32), dict(in_dim=30), dict(num_lods=8, in_dim=32),
                                  dict(dtype_table=1), dict(dtype_table=2), dict(dtype_params=2)])
def test_unsupported_shapes_are_refused_before_any_launch(over):
    rc, msg = _call(_args(**over))
    assert rc == UNSUPPORTED and "nerf_prune_query" in msg and "hidden 64" in msg
    rc, _ = _call(_args(cells=0, **over))
    assert rc == UNSUPPORTED                                                         # whatever the cell count


@pytest.mark.parametrize("name", ["points", "unit", "table", "first_idx", "resolutions", "params", "occ_in", "occ_out", "keep"])
def test_null_pointers_are_invalid(name):
    rc, msg = _call(_args(**{name: None}))
    assert rc == INVALID and "null pointer" in msg
    rc, _ = _call(_args(cells=0, **{name: None}))
    assert rc == OK                                                                  # nothing to do, nothing read


def test_other_invalid_arguments_and_the_empty_call():
    for over in (dict(cells=-1), dict(level=-1), dict(level=15), dict(bitwidth=0), dict(bitwidth=31), dict(zero_from_col=31),
                 dict(zero_from_col=34), dict(zero_from_col=-2)):
        rc, _ = _call(_args(**over))
        assert rc == INVALID, over
    bad = (ctypes.c_int32 * 16)(*([16] * 15 + [0]))
    assert _call(_args(resolutions=bad))[0] == INVALID
    assert _call(_args(cells=0))[0] == OK
    buf = ctypes.create_string_buffer(8)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _call(_args(), debug=True, feats=None, density=p)[0] == INVALID           # the debug form needs both extra outputs
    assert _call(_args(), debug=True, feats=p, density=None)[0] == INVALID
    assert _call(_args(cells=0), debug=True, feats=p, density=p)[0] == OK
    assert _call(_args(hidden=128), debug=True, feats=p, density=p)[0] == UNSUPPORTED


def test_the_python_wrapper_refuses_cpu_tensors_and_bad_shapes():
    import wisp._C as C
    pts = torch.zeros(8, 3, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        C.nerf_prune_query(pts, torch.zeros(8, 3), 1, torch.zeros(72, 2), torch.tensor([0, 8, 72]), [2, 4], 12, 2, torch.zeros(10),
                           4, 64, torch.zeros(8), 0.95, 0.5)


# ------------------------------------------------------------------------------------------------ 3. path selection
def _cpu_nef(level=2, multiscale='cat', hidden=64, num_lods=6):
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(0)
    grid = HashGrid.from_geometric(OctreeAS.make_dense(level), feature_dim=2, num_lods=num_lods, multiscale_type=multiscale,
                                   feature_std=0.1, codebook_bitwidth=12, min_grid_res=4, max_grid_res=64)
    return NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=hidden, num_layers=1, bias=True,
                               prune_density_decay=0.95, prune_min_density=0.5)


@pytest.fixture
def as_if_on_the_gpu(monkeypatch):
    """every tensor reports is_cuda: the one property of the selection that a CPU box cannot satisfy"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.delenv("WISP_PRUNE_FUSED", raising=False)


@pytest.fixture
def stubs(monkeypatch):
    """the native query and the octree build replaced by recorders"""
    import wisp.ops.nerf_mlp as ops
    from wisp.accelstructs import OctreeAS
    seen = {"query": [], "mask": []}

    def query(nef, unit, debug=False, pad_rows=0):
        seen["query"].append(unit.clone())
        cells = unit.shape[0]
        return torch.arange(cells, dtype=torch.float32), torch.arange(cells) % 2 == 0

    def from_leaf_mask(keep, level):
        seen["mask"].append((keep.clone(), level))
        return None                                   # "empty mask": prune leaves the structure alone
    monkeypatch.setattr(ops, "fused_prune_query", query)
    monkeypatch.setattr(OctreeAS, "from_leaf_mask", staticmethod(from_leaf_mask))
    return seen


def test_prune_takes_the_fused_query_and_keeps_every_draw(as_if_on_the_gpu, stubs):
    nef = _cpu_nef()
    assert nef.prune_fused()
    blas = nef.grid.blas
    torch.manual_seed(5)
    nef.prune()
    after = torch.rand(3)
    torch.manual_seed(5)
    unit = torch.rand(64, 3)
    torch.rand(2, 64)                                 # the view-direction draw of the modular path: made, not used
    assert torch.equal(after, torch.rand(3))
    assert len(stubs["query"]) == 1 and torch.equal(stubs["query"][0], unit)
    assert torch.equal(nef.grid.occupancy, torch.arange(64, dtype=torch.float32))
    (keep, level), = stubs["mask"]
    assert level == 2 and torch.equal(keep, torch.arange(64) % 2 == 0) and nef.grid.blas is blas
    # injected draws: passed through, nothing drawn
    torch.manual_seed(6)
    mine = torch.rand(64, 3)
    state = torch.get_rng_state()
    nef.prune(unit_samples=mine, view_dirs=torch.randn(64, 3, generator=torch.Generator().manual_seed(1)))
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(stubs["query"][1], mine)


@pytest.mark.parametrize("case", ["switch", "sum", "hidden128", "half_table", "not_dense", "bf16_compute", "unfused_decoder", "autocast",
                                  "no_threshold", "too_deep", "four_features", "cpu"])
def test_everything_else_takes_the_modular_path(case, as_if_on_the_gpu, stubs, monkeypatch):
    nef = _cpu_nef(multiscale='sum' if case == "sum" else 'cat', hidden=128 if case == "hidden128" else 64)
    if case == "switch":
        monkeypatch.setenv("WISP_PRUNE_FUSED", "0")
    elif case == "half_table":
        nef.grid.codebook.feats.data = nef.grid.codebook.feats.data.half()
    elif case == "not_dense":
        nef.grid.dense_points = nef.grid.dense_points[:63]
    elif case == "bf16_compute":
        nef.decoder_compute = 'bf16'
    elif case == "unfused_decoder":
        nef.fused_decoder = False
    elif case == "no_threshold":
        nef.prune_min_density = None
    elif case == "too_deep":
        nef.grid.blas.max_level = 10
        nef.grid.dense_points = torch.zeros(1, 3, dtype=torch.int16).expand(8 ** 10, 3)
    elif case == "four_features":
        nef.grid.feature_dim = 4
    elif case == "cpu":
        monkeypatch.undo()                            # tensors say where they are again
        monkeypatch.delenv("WISP_PRUNE_FUSED", raising=False)
    elif case == "autocast":                           # (the lookup reads a bf16 table then, the decoder computes in bf16)
        monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    assert not nef.prune_fused()
    assert stubs["query"] == []


def test_the_unmodified_field_is_selected(as_if_on_the_gpu):
    assert _cpu_nef().prune_fused() and _cpu_nef(num_lods=16).prune_fused() and _cpu_nef(level=1, num_lods=1).prune_fused()


# ------------------------------------------------------------------------------------------------ 4. the kernels
def test_kernel_resources():
    """both forms: workgroup 512 (8 waves, two per SIMD: at most 256 VGPRs each), no scratch, no static LDS; and the exact-fp32
    decoder, which now takes its first two layers from the same header, still has no scratch either"""
    import kernel_meta
    import wisp._C as C
    meta = kernel_meta.kernels(C.LIB_PATH)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    hits = {n: v for n, v in kern.items() if "prune_query_kernel<" in n}
    assert len(hits) == 2, list(hits)
    for name, v in hits.items():
        assert v["scratch"] == 0 and v["wg"] == 512 and v["vgpr"] + v["agpr"] <= 256 and v["lds"] == 0, (name, v)
    dec = {n: v for n, v in kern.items() if "nerf_mlp_kernel<float" in n}
    assert len(dec) == 12 and all(v["scratch"] == 0 for v in dec.values()), dec      # 3 I/O types x 1 or 2 waves x forward / backward
