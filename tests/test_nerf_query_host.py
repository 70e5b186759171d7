"""CPU: the host side of the fused field query (csrc/nerf_query.hip) and of the evaluation surface built on it - the entry point's
declaration / binding / export and argument validation, the kernel's resources, the path selection (nerf_query_supported, the
tracer's `fused_query` attribute), MultiviewTrainer.evaluate_metrics next to the reference's method body, and the render script's
command line."""
import ast
import ctypes
import logging
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "wisp_nerf_query"
OK, INVALID, UNSUPPORTED = 0, -1, -3
REF = "/root/reference/wisp"


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
    assert got == [kinds[a] for a in C.SIGNATURES[ENTRY]]
    assert "nerf.py:219-264" in header[header.index("The inference query of a radiance field"):header.index(f"int {ENTRY}(")]
    assert hasattr(ctypes.CDLL(C.LIB_PATH), ENTRY)
    assert C.lib.wisp_abi_version() == C.ABI_VERSION == 4                            # an added entry point does not bump it
    mk = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "Makefile")).read()
    assert "nerf_query.hip" in mk
    assert callable(C.nerf_query)


# ------------------------------------------------------------------------------------------------ 2. argument validation
def _args(**over):
    """a valid argument list for the nerf_hash.yaml shape, with dummy non-null pointers (validation fails before any is read)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(coords=p, dirs=p, ridx=None, num_rays=0, n=512, table=p, dtype_table=0, feature_dim=2, coord_dim=3, first_idx=p,
             resolutions=(ctypes.c_int32 * 16)(*[16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512]), num_lods=16,
             bitwidth=19, zero_from_col=30, params=p, dtype_params=0, in_dim=32, hidden=64, rgb=p, density=p)
    a.update(over)
    a["_keep_alive"] = buf
    return a


def _call(a):
    import wisp._C as C
    lib = ctypes.CDLL(C.LIB_PATH)
    fn = getattr(lib, ENTRY)
    fn.argtypes = C.SIGNATURES[ENTRY]
    fn.restype = ctypes.c_int
    res = a["resolutions"]
    rc = fn(a["coords"], a["dirs"], a["ridx"], a["num_rays"], a["n"], a["table"], a["dtype_table"], a["feature_dim"], a["coord_dim"],
            a["first_idx"], None if res is None else ctypes.cast(res, ctypes.c_void_p), a["num_lods"], a["bitwidth"],
            a["zero_from_col"], a["params"], a["dtype_params"], a["in_dim"], a["hidden"], a["rgb"], a["density"], None)
    return rc, C.last_error()


@pytest.mark.parametrize("over", [dict(feature_dim=4), dict(coord_dim=2), dict(num_lods=17, in_dim=34), dict(num_lods=0, in_dim=0),
                                  dict(hidden=128), dict(hidden=32), dict(in_dim=30), dict(num_lods=8, in_dim=32),
                                  dict(dtype_table=1), dict(dtype_table=2), dict(dtype_params=2)])
def test_unsupported_shapes_are_refused_before_any_launch(over):
    rc, msg = _call(_args(**over))
    assert rc == UNSUPPORTED and "nerf_query" in msg and "hidden 64" in msg
    rc, _ = _call(_args(n=0, **over))
    assert rc == UNSUPPORTED                                                         # whatever the sample count


@pytest.mark.parametrize("name", ["coords", "dirs", "table", "first_idx", "resolutions", "params"])
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
    for over in (dict(n=-1), dict(bitwidth=0), dict(bitwidth=31), dict(zero_from_col=31), dict(zero_from_col=34),
                 dict(zero_from_col=-2)):
        rc, _ = _call(_args(**over))
        assert rc == INVALID, over
    bad = (ctypes.c_int32 * 16)(*([16] * 15 + [0]))
    assert _call(_args(resolutions=bad))[0] == INVALID
    assert _call(_args(n=0))[0] == OK
    assert _call(_args(n=0, rgb=None, density=None))[0] == OK


def test_the_python_wrapper_refuses_cpu_tensors():
    import wisp._C as C
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        C.nerf_query(torch.zeros(8, 3), torch.zeros(8, 3), None, torch.zeros(72, 2), torch.tensor([0, 8, 72]), [2, 4], 12, 2,
                     torch.zeros(10), 4, 64)


# ------------------------------------------------------------------------------------------------ 3. the kernel
def test_kernel_resources():
    """both forms: workgroup 256 (4 waves, one per SIMD), no scratch, no static LDS, and a dynamic LDS size - restated here from the
    file's own constants - within the CU's 160 KB; the exact-fp32 decoder, whose colour half now comes from the same header,
    still has no scratch and stays inside the 512 registers of a single-wave SIMD (the metadata's VGPR count includes the AGPRs)"""
    import kernel_meta
    import wisp._C as C
    meta = kernel_meta.kernels(C.LIB_PATH)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    hits = {n: v for n, v in kern.items() if "nerf_query_kernel<" in n}
    assert len(hits) == 2, list(hits)
    src = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "nerf_query.hip")).read()
    waves = int(re.search(r"constexpr int NQ_WAVES = (\d+);", src).group(1))
    for name, v in hits.items():
        assert v["scratch"] == 0 and v["wg"] == waves * 64 and v["vgpr"] <= 512 and v["lds"] == 0, (name, v)
    IN, H, LDI, LDH = 32, 64, 33, 65
    weights = H * LDI + 32 * LDH + H * LDH + H * LDH + 32 * LDH
    biases = 3 * H + 64
    per_wave = 64 * LDI + 2 * 32 * LDH                                               # x0 and the two aliased activation tiles
    assert (weights + biases + waves * per_wave) * 4 <= 160 * 1024
    assert "static_assert(NQ_LDS_BYTES <= 160 * 1024" in src
    for word in ("printf", "assert(", "atomic"):
        assert word not in src.replace("static_assert(", ""), word
    dec = {n: v for n, v in kern.items() if "nerf_mlp_kernel<float" in n}
    assert len(dec) == 12 and all(v["scratch"] == 0 and v["vgpr"] <= 512 for v in dec.values()), dec


def test_decoder_and_query_expand_one_definition():
    """nerf_mlp.hip no longer carries its own view encoding or layers 3 - 5: both files expand the header's macros"""
    csrc = os.path.join(ROOT, "kaolin-wisp_amd", "csrc")
    mlp, query = open(os.path.join(csrc, "nerf_mlp.hip")).read(), open(os.path.join(csrc, "nerf_query.hip")).read()
    for macro in ("WISP_F32_VIEW_ENCODE", "WISP_F32_LAYER1", "WISP_F32_LAYER2", "WISP_F32_LAYER_HIDDEN", "WISP_F32_LAYER5"):
        assert macro + "(" in mlp and macro + "(" in query, macro
    assert "sinf(" not in mlp and "sinf(" not in query and "expf(" not in query


# ------------------------------------------------------------------------------------------------ 4. path selection
def _cpu_nef(level=2, multiscale='cat', hidden=64, num_lods=6, bias=True):
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralRadianceField
    torch.manual_seed(0)
    grid = HashGrid.from_geometric(OctreeAS.make_dense(level), feature_dim=2, num_lods=num_lods, multiscale_type=multiscale,
                                   feature_std=0.1, codebook_bitwidth=12, min_grid_res=4, max_grid_res=64)
    return NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=hidden, num_layers=1, bias=bias)


@pytest.fixture
def as_if_on_the_gpu(monkeypatch):
    """every tensor reports is_cuda: the one property of the selection that a CPU box cannot satisfy"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.delenv("WISP_NERF_QUERY_FUSED", raising=False)


def test_the_unmodified_field_is_selected(as_if_on_the_gpu):
    from wisp.ops.nerf_mlp import nerf_query_supported
    assert nerf_query_supported(_cpu_nef()) and nerf_query_supported(_cpu_nef(num_lods=16)) and nerf_query_supported(_cpu_nef(num_lods=1))
    assert nerf_query_supported(_cpu_nef(bias=False)) and nerf_query_supported(_cpu_nef(), lod_idx=3)
    nef = _cpu_nef()
    nef.grid.dense_points = nef.grid.dense_points[:63]           # the prune's conditions on the octree do not apply here
    assert nerf_query_supported(nef)


@pytest.mark.parametrize("case", ["switch", "sum", "hidden128", "half_table", "bf16_compute", "unfused_decoder", "autocast",
                                  "four_features", "cpu", "half_decoder", "bad_lod", "octree_grid"])
def test_every_disqualifying_shape_is_refused(case, as_if_on_the_gpu, monkeypatch):
    from wisp.ops.nerf_mlp import nerf_query_supported
    nef = _cpu_nef(multiscale='sum' if case == "sum" else 'cat', hidden=128 if case == "hidden128" else 64)
    lod_idx = None
    if case == "switch":
        monkeypatch.setenv("WISP_NERF_QUERY_FUSED", "0")
    elif case == "half_table":
        nef.grid.codebook.feats.data = nef.grid.codebook.feats.data.half()
    elif case == "bf16_compute":
        nef.decoder_compute = 'bf16'
    elif case == "unfused_decoder":
        nef.fused_decoder = False
    elif case == "four_features":
        nef.grid.feature_dim = 4
    elif case == "cpu":
        monkeypatch.undo()                            # tensors say where they are again
        monkeypatch.delenv("WISP_NERF_QUERY_FUSED", raising=False)
    elif case == "autocast":
        monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    elif case == "half_decoder":
        nef.decoder_color.lout.weight.data = nef.decoder_color.lout.weight.data.half()      # the LAST of the ten tensors
    elif case == "bad_lod":
        lod_idx = 6
    elif case == "octree_grid":
        from wisp.accelstructs import OctreeAS
        from wisp.models.grids import OctreeGrid
        nef.grid = OctreeGrid(OctreeAS.make_dense(2), feature_dim=5, num_lods=2, multiscale_type='sum', feature_std=0.1)
    assert not nerf_query_supported(nef, lod_idx)


def test_fused_nerf_query_refuses_gradients_and_cpu_fields():
    from wisp.ops.nerf_mlp import fused_nerf_query
    nef = _cpu_nef()
    coords, dirs = torch.zeros(4, 3), torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="no backward"):
        fused_nerf_query(nef, coords, ray_d=dirs)                                    # the parameters require a gradient
    with pytest.raises(NotImplementedError, match="no backward"):
        fused_nerf_query(nef.requires_grad_(False), coords.clone().requires_grad_(True), ray_d=dirs)
    nef.requires_grad_(False)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        fused_nerf_query(nef, coords, ray_d=dirs)                                    # a field on the CPU: no fallback
    with torch.no_grad(), pytest.raises(RuntimeError, match="must be a GPU tensor"):
        fused_nerf_query(nef.requires_grad_(True), coords, ray_d=dirs)
    with torch.no_grad():
        with pytest.raises(ValueError):
            fused_nerf_query(nef, coords, ray_d=dirs, ray_dirs=dirs, ridx=torch.zeros(4, dtype=torch.int64))
        with pytest.raises(ValueError):
            fused_nerf_query(nef, coords, ray_dirs=dirs)


def _traced_with(tracer, nef, monkeypatch, grad=False, extra=()):
    """runs tracer.trace over stubs of everything behind the query; returns which query the call took"""
    import wisp.ops.nerf_mlp as ops
    import wisp.ops.render as render_ops
    import wisp.tracers._fused_trace as fused_trace
    from wisp.core import Rays
    taken = []
    monkeypatch.setattr(fused_trace, "supports", lambda *a, **k: False)              # (the one-node training trace: not the subject)

    def fused(nef_, coords, ray_d=None, ray_dirs=None, ridx=None, lod_idx=None, want_rgb=True, pad_rows=0):
        taken.append("fused")
        assert ray_d is None and ray_dirs.shape == (3, 3) and ridx.shape == (5,)
        return torch.zeros(5, 3), torch.zeros(5, 1)
    monkeypatch.setattr(ops, "fused_nerf_query", fused)
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


def test_tracer_reads_the_plain_attribute(as_if_on_the_gpu, monkeypatch):
    import inspect
    from wisp.tracers import PackedRFTracer
    assert "fused_query" not in inspect.signature(PackedRFTracer.__init__).parameters
    nef = _cpu_nef().requires_grad_(False)
    tracer = PackedRFTracer(raymarch_type='ray', num_steps=4)
    assert not hasattr(tracer, "fused_query")
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]                     # absent: today's path
    tracer.fused_query = False
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]
    tracer.fused_query = True
    assert _traced_with(tracer, nef, monkeypatch) == ["fused"]
    assert _traced_with(tracer, nef, monkeypatch, grad=True)[:1] != ["fused"]        # gradients enabled
    assert "fused" not in _traced_with(tracer, nef, monkeypatch, extra=("normal",))  # an extra channel
    monkeypatch.setenv("WISP_NERF_QUERY_FUSED", "0")
    assert _traced_with(tracer, nef, monkeypatch) == ["modular"]


# ------------------------------------------------------------------------------------------------ 5. evaluation surface
class _Tracer:
    """stands for the pipeline's tracer: records what `fused_query` was while it rendered"""


def _stub_trainer(tmp_path, valid_metrics=('psnr',), save=True, views=3, h=5, w=4, fail_at=None):
    from wisp.core import Rays, RenderBuffer
    g = torch.Generator().manual_seed(3)
    tracer = _Tracer()
    seen = []
    buffers = [RenderBuffer(rgb=torch.rand(h * w, 3, generator=g), depth=torch.rand(h * w, 1, generator=g) * 4,
                            alpha=torch.rand(h * w, 1, generator=g), hit=torch.rand(h * w, 1, generator=g) > 0.5) for _ in range(views)]

    class Visualizer:
        calls = 0

        def render(self, pipeline, rays, lod_idx=None):
            seen.append((getattr(pipeline.tracer, "fused_query", "absent"), lod_idx, tuple(rays.origins.shape)))
            if fail_at is not None and self.calls == fail_at:
                raise RuntimeError("render failed")
            self.calls += 1
            return buffers[self.calls - 1]
    rays = Rays(torch.rand(views, h * w, 3, generator=g), torch.rand(views, h * w, 3, generator=g), dist_min=0.5, dist_max=6.0)
    ds = types.SimpleNamespace(img_shape=torch.Size([h, w]), data=dict(rays=rays, rgb=torch.rand(views, h * w, 3, generator=g)))
    me = types.SimpleNamespace(
        tracker=types.SimpleNamespace(log_dir=str(tmp_path), visualizer=Visualizer()),
        cfg=types.SimpleNamespace(valid_metrics=tuple(valid_metrics), save_valid_imgs=save),
        validation_dataset=ds, pipeline=types.SimpleNamespace(tracer=tracer), epoch=7, max_epochs=50, return_dict={}, device='cpu')
    return me, ds, buffers, seen


def _reference_evaluate_metrics(glb):
    path = os.path.join(REF, "trainers/multiview_trainer.py")
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MultiviewTrainer")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "evaluate_metrics")
    fn.decorator_list = []
    ns = dict(glb)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["evaluate_metrics"]


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not mounted (GPU box)")
def test_evaluate_metrics_against_the_reference_method_body(tmp_path, monkeypatch, caplog):
    """the reference's evaluate_metrics (trainers/multiview_trainer.py:191-255), compiled from the file where it lies, and this
    package's, over the same stub trainer whose visualizer returns fixed buffers: metric values, the max rule over three calls, the
    log lines, the PNG names and pixel bytes"""
    import image_ref
    from wisp.core import Rays, RenderBuffer
    from wisp.ops.image import read_png
    from wisp.trainers import MultiviewTrainer
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)            # the reference moves everything `.cuda()`
    written = {}

    def ref_write_png(path, data):
        written[os.path.basename(path)] = data.clone()

    def no_exr(*a, **k):
        raise ImportError("pyexr")
    ref_fn = _reference_evaluate_metrics(dict(os=os, torch=torch, tqdm=lambda x: x, Rays=Rays, RenderBuffer=RenderBuffer,
                                              psnr=image_ref.reference_psnr(), write_png=ref_write_png, write_exr=no_exr,
                                              log=logging.getLogger("ref")))
    ref_dir, our_dir = tmp_path / "ref", tmp_path / "ours"
    ref_me, ds, buffers, _ = _stub_trainer(ref_dir)
    our_me, _, _, seen = _stub_trainer(our_dir)
    os.makedirs(ref_dir / "val")
    ref_me.return_dict, our_me.return_dict = {"psnr": 11.25}, {"psnr": 11.25}        # an earlier, better validation
    lines = {}
    for who, me, fn in (("ref", ref_me, ref_fn), ("ours", our_me, MultiviewTrainer.evaluate_metrics)):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            first = fn(me, ds, 2, name="lod2")
            me.tracker.visualizer.calls = 0
            me.return_dict.pop("psnr")
            second = fn(me, ds, 2, name="lod2")
            me.tracker.visualizer.calls = 0
            me.return_dict["psnr"] = float(second["psnr"]) - 1.0                      # a worse one: replaced
            third = fn(me, ds, 2, name=None)
        lines[who] = [r.getMessage() for r in caplog.records]
        me.results = (first, second, third)
    for a, b in zip(ref_me.results, our_me.results):
        assert list(a) == list(b) == ["psnr"] and float(a["psnr"]) == float(b["psnr"])
    assert float(ref_me.return_dict["psnr"]) == float(our_me.return_dict["psnr"]) == float(our_me.results[2]["psnr"])
    assert lines["ref"] == lines["ours"] and len(lines["ours"]) == 4
    assert lines["ours"][0] == "Skipping EXR logging since pyexr is not found."      # once
    assert re.fullmatch(r"EPOCH 7/50 \| lod2 psnr: \d+\.\d\d", lines["ours"][1]), lines["ours"]
    assert lines["ours"][3].startswith("EPOCH 7/50 | None psnr: ")
    assert sorted(os.listdir(our_dir / "val")) == sorted(written) == ["0-lod2.png", "0.png", "1-lod2.png", "1.png", "2-lod2.png", "2.png"]
    for k, rb in enumerate(buffers):
        want = rb.reshape(5, 4, -1).image().byte().rgb
        assert torch.equal(written[f"{k}-lod2.png"], want)
        for name in (f"{k}-lod2.png", f"{k}.png"):
            assert np.array_equal(read_png(str(our_dir / "val" / name)), want.numpy()), name
    # every render of ours ran with the tracer's fused_query on, per view at full resolution, and the attribute is gone again
    assert seen == [(True, 2, (20, 3))] * 9 and not hasattr(our_me.pipeline.tracer, "fused_query")


def test_evaluate_metrics_without_images_and_its_refusals(tmp_path):
    from wisp.ops.image import psnr
    from wisp.trainers import MultiviewTrainer
    me, ds, buffers, seen = _stub_trainer(tmp_path, save=False)
    out = MultiviewTrainer.evaluate_metrics(me, ds, None, name="x")
    want = sum(psnr(rb.rgb.reshape(5, 4, 3), ds.data["rgb"][k].reshape(5, 4, 3)) for k, rb in enumerate(buffers)) / 3
    assert float(out["psnr"]) == float(want) and me.return_dict == {"psnr": out["psnr"]}
    assert not os.path.exists(tmp_path / "val")
    for metric in ("ssim", "lpips"):
        me, ds, _, seen = _stub_trainer(tmp_path, valid_metrics=("psnr", metric))
        with pytest.raises(NotImplementedError, match=metric):
            MultiviewTrainer.evaluate_metrics(me, ds, None)
        assert seen == []


@pytest.mark.parametrize("before", ["absent", False, True])
def test_fused_query_attribute_is_restored(tmp_path, before):
    from wisp.trainers import MultiviewTrainer
    for fail_at in (None, 1):
        me, ds, _, seen = _stub_trainer(tmp_path, save=False, fail_at=fail_at)
        if before != "absent":
            me.pipeline.tracer.fused_query = before
        if fail_at is None:
            MultiviewTrainer.evaluate_metrics(me, ds, None)
        else:
            with pytest.raises(RuntimeError, match="render failed"):
                MultiviewTrainer.evaluate_metrics(me, ds, None)
        assert [s[0] for s in seen] == [True] * len(seen) and len(seen) == (3 if fail_at is None else 2)
        assert getattr(me.pipeline.tracer, "fused_query", "absent") == before


@pytest.mark.parametrize("before", ["absent", False, True])
def test_render_sets_and_restores_the_attribute(before):
    from wisp.core import Rays, RenderBuffer
    from wisp.trainers.validation import render
    seen = []

    class Tracer:
        def __call__(self, nef, rays=None, lod_idx=None, **kw):
            seen.append(getattr(self, "fused_query", "absent"))
            if rays.origins.shape[0] == 1:
                raise RuntimeError("trace failed")
            return RenderBuffer(rgb=torch.zeros(rays.origins.shape[0], 3))
    tracer = Tracer()
    if before != "absent":
        tracer.fused_query = before
    pipe = types.SimpleNamespace(tracer=tracer, nef=None)
    rays = Rays(torch.zeros(5, 3), torch.ones(5, 3), dist_min=0.0, dist_max=1.0)
    with pytest.raises(RuntimeError, match="trace failed"):                          # (the last chunk has one ray)
        render(pipe, rays, render_batch=2)
    assert seen == [before] * 3                                                       # None: the tracer is left alone
    seen.clear()
    for flag in (True, False):
        with pytest.raises(RuntimeError, match="trace failed"):
            render(pipe, rays, render_batch=2, fused_query=flag)
        assert seen == [flag] * 3 and getattr(tracer, "fused_query", "absent") == before
        seen.clear()
        render(pipe, rays, render_batch=-1, fused_query=flag)
        assert seen == [flag] and getattr(tracer, "fused_query", "absent") == before
        seen.clear()


def test_validate_goes_through_evaluate_metrics_only_with_save_valid_imgs(monkeypatch):
    import wisp.trainers.validation as validation
    from wisp.trainers import MultiviewTrainer
    calls = []
    monkeypatch.setattr(validation, "evaluate_psnr", lambda *a, **k: (calls.append("psnr") or 20.0, "line"))
    grid = types.SimpleNamespace(num_lods=6)
    pipe = types.SimpleNamespace(nef=types.SimpleNamespace(grid=grid), eval=lambda: None, train=lambda: None)

    class Rays_:
        origins = torch.zeros(2, 4, 3)

        def __getitem__(self, i):
            return i
    ds = types.SimpleNamespace(data=dict(rays=Rays_(), rgb=torch.zeros(2, 4, 3)))

    def evaluate_metrics(dataset, lod_idx, name=None):
        calls.append(("evaluate_metrics", lod_idx, name))
        me.return_dict["psnr"] = 21.0
        return {"psnr": 21.0}
    me = types.SimpleNamespace(validation_dataset=ds, pipeline=pipe, epoch=1, max_epochs=2, return_dict={},
                               cfg=types.SimpleNamespace(save_valid_imgs=False), evaluate_metrics=evaluate_metrics)
    assert MultiviewTrainer.validate(me) == {"psnr": 20.0} and calls == ["psnr"]
    me.cfg.save_valid_imgs = True
    assert MultiviewTrainer.validate(me) == {"psnr": 21.0} and calls[1:] == [("evaluate_metrics", 5, "lod5")]
    me.validation_dataset = None
    assert MultiviewTrainer.validate(me) is None


# ------------------------------------------------------------------------------------------------ 6. the script
def test_render_script_help():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_nerf.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--checkpoint", "--write-synlego", "--steps", "--views", "--res", "--render-batch", "--out", "--no-fused"):
        assert flag in out.stdout, flag
