"""CPU: the host side of the fused all-LOD octree SDF step (wisp_sdf_lods_train_step, csrc/spc_grad.hip;
SDFTrainStep(only_last=False, fused_lods=True); scripts/train_nglod.py --all-lods): the float64 restatement of
tests/sdf_lods_step_ref.py against its autograd twin, the reference's weights of the textured loss, declaration / binding / export
agreement, argument checks that fail before any launch, the kernels' resources read from the code object, the rules of
SDFTrainStep._fused_field, the script's option, and what the shapes of the GPU file reach."""
import ctypes
import os
import subprocess
import sys
import types

import pytest
import torch

import kernel_meta
import sdf_lods_step_ref as R
import sdf_step_exact_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
REF = "/root/reference/wisp"
GRADS = ("w1", "b1", "w2", "b2")


# ------------------------------------------------------------------------------------------------ 1. the float64 step
def _same(a, b):
    for k in ("loss",) + GRADS:
        assert torch.equal(a[k].double().reshape(-1), b[k].double().reshape(-1)), k
    for l, (x, y) in enumerate(zip(a["tables"], b["tables"])):
        assert torch.equal(x.double(), y.double()), l


@pytest.mark.parametrize("tex,pos", [(0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("levels,n", [((5,), 16), ((3, 4, 5), 64), ((0, 1, 2, 3, 4, 5), 16)])
def test_float64_step_equals_its_autograd_twins_on_exact_cases(tex, pos, levels, n):
    """the written-out step = the weighted sum over k of X.step_reference on the cut cases = float64 autograd through the oracle with
    the reference's loop = fp32 autograd, BIT FOR BIT (nothing rounds on an exact case, in any order)"""
    case = R.exact_lods_case("small", levels, n, 24, tex=bool(tex), pos_input=pos)
    want = case["want"]
    assert want["loss"].shape == (1 + (2 if tex else 1) * len(levels),)
    _same(R.reference_by_cuts(case), want)
    _same(R.autograd_reference(case), want)
    _same(R.autograd_reference(case, torch.float32), want)
    w_sdf, w_rgb = R.default_weights(case)
    _same(R.autograd_reference(case, w_sdf=w_sdf, w_rgb=w_rgb), want)         # the reference's loop IS the weights 1 and L - k
    L = len(levels)
    assert torch.equal(sum(d["w1"] for d in want["per_lod"]), want["w1"])
    for k, d in enumerate(want["per_lod"]):                                   # LOD k's gradient lands on levels 0..k only
        assert all(not bool(t.any()) for t in d["tables"][k + 1:])
    if L > 1:
        assert bool(want["per_lod"][0]["tables"][0].any()) and not torch.equal(want["per_lod"][0]["tables"][0], want["tables"][0])


def test_float64_step_equals_float64_autograd_on_generic_inputs():
    case = dict(R.exact_lods_case("small", (3, 4, 5), 64, 24, tex=True, pos_input=1))
    g = torch.Generator().manual_seed(5)
    case["tables"] = [torch.randn(t.shape, generator=g) * 0.3 for t in case["tables"]]
    case["w1"], case["b1"] = torch.randn(case["w1"].shape, generator=g) * 0.4, torch.randn(case["b1"].shape, generator=g) * 0.1
    case["w2"], case["b2"] = torch.randn(case["w2"].shape, generator=g) * 0.3, torch.randn(case["b2"].shape, generator=g) * 0.1
    case["gts"], case["rgb_gts"] = torch.randn(64, generator=g) * 0.1, torch.rand(64, 3, generator=g)
    w_sdf, w_rgb = [1.0, 0.5, 3.0], [2.0, 1.0, 0.25]
    want, got = R.lods_reference(case, w_sdf, w_rgb), R.autograd_reference(case, w_sdf=w_sdf, w_rgb=w_rgb)
    # the restatement takes the sigmoid in fp32 and rounds g to fp32 once (2^-24 relative each): 1e-6 of a tensor's largest entry
    for k in ("loss",) + GRADS:
        assert torch.allclose(want[k].reshape(-1), got[k].double().reshape(-1), rtol=1e-5, atol=1e-6 * float(want[k].abs().max())), k
    for a, b in zip(want["tables"], got["tables"]):
        assert bool(a.any()) and torch.allclose(a, b.double(), rtol=1e-5, atol=1e-6 * float(a.abs().max()))


def test_a_refusal_blames_the_inputs():
    case = dict(R.exact_lods_case("small", (3, 4, 5), 64, 24))
    case["gts"] = case["gts"] + 1e-3
    with pytest.raises(AssertionError, match="inputs are not exact|no fp32 value"):
        R.check_exact_lods(case)
    with pytest.raises(AssertionError, match="power of two"):
        R.check_exact_lods(dict(case, n=48))


# ------------------------------------------------------------------------------------------------ 2. the reference's weights
class _Field(torch.nn.Module):
    """CPU stand-in for a textured field (tests/test_sdf_tex_step_host.py's): a table per LOD + one Linear with four outputs"""
    def __init__(self):
        super().__init__()
        torch.manual_seed(8)
        self.grid = torch.nn.Module()
        self.grid.num_lods = 3
        self.grid.feats = torch.nn.Parameter(torch.randn(3, 32, 4) * 0.1)
        self.decoder = torch.nn.Linear(4 + 3, 4)
        self._forward_functions = {self.rgbsdf: {"rgb", "sdf"}}

    def rgbsdf(self, coords, lod_idx):
        cell = ((coords[:, 0] * 0.5 + 0.5) * 31).long().clamp(0, 31)
        return self.decoder(torch.cat([self.grid.feats[: lod_idx + 1, cell].sum(0), coords], -1))

    def forward(self, coords=None, lod_idx=None, channels=None):
        y = self.rgbsdf(coords, lod_idx)
        out = dict(rgb=torch.sigmoid(y[..., :3]), sdf=y[..., 3:4])
        return [out[c] for c in channels] if isinstance(channels, (list, tuple)) else out[channels]


def _weighted_loss(f, x, y, c, w_sdf, w_rgb):
    total = 0.0
    for k in range(3):
        rgb, sdf = f(coords=x, lod_idx=k, channels=["rgb", "sdf"])
        total = total + w_sdf[k] * ((sdf - y) ** 2).sum() + w_rgb[k] * ((rgb - c[..., :3]) ** 2).sum()
    return total / x.shape[0]


def test_modular_textured_loss_has_the_weights_one_and_L_minus_k():
    """SDFTrainStep(only_last=False)'s modular textured loss on the CPU stand-in is sum_k S_k + sum_k (L - k) R_k over B: the weights
    the fused step is handed"""
    from wisp.trainers import SDFTrainStep
    g = torch.Generator().manual_seed(2)
    x, y, c = torch.rand(64, 3, generator=g) * 2 - 1, torch.randn(64, 1, generator=g) * 0.1, torch.rand(64, 4, generator=g)
    f = _Field()
    tr = SDFTrainStep(f, only_last=False)
    assert tr.textured and tr.loss_lods() == [0, 1, 2]
    loss = tr._forward_backward(x, y, c)
    got = {n: p.grad.clone() for n, p in f.named_parameters()}
    f.zero_grad()
    want = _weighted_loss(f, x, y, c, [1.0, 1.0, 1.0], [3.0, 2.0, 1.0])
    want.backward()
    assert abs(float(loss) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    for n, p in f.named_parameters():
        assert torch.allclose(got[n], p.grad, rtol=1e-5, atol=1e-8), n
    f.zero_grad()
    other = _weighted_loss(f, x, y, c, [1.0, 1.0, 1.0], [1.0, 1.0, 1.0])      # (and they are not all 1)
    assert abs(float(other) - float(want)) > 1e-3


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not mounted")
def test_the_weights_are_the_reference_methods():
    """SDFTrainer.step (trainers/sdf_trainer.py:65-124) with sample_tex over every LOD, the method body compiled from the reference
    file: the loss it accumulates is the weighted loss with w_sdf = 1, w_rgb = L - k"""
    from test_reference_modules import _TorchWithoutNvtx, _reference_method
    ref_step = _reference_method("trainers/sdf_trainer.py", "SDFTrainer", "step", dict(torch=_TorchWithoutNvtx()))
    g = torch.Generator().manual_seed(3)
    x, y, c = torch.rand(64, 3, generator=g) * 2 - 1, torch.randn(64, 1, generator=g) * 0.1, torch.rand(64, 4, generator=g)
    fr, fw = _Field(), _Field()
    opt = torch.optim.SGD(fr.parameters(), lr=0.0)
    metrics = types.SimpleNamespace(total_loss=0.0, l2_loss=0.0, rgb_loss=0.0, num_samples=0)
    nef_r = lambda coords=None, lod_idx=None, channels=None: [tuple(fr(coords=coords, lod_idx=lod_idx, channels=channels))]  # noqa: E731
    me = types.SimpleNamespace(pipeline=types.SimpleNamespace(nef=nef_r, zero_grad=fr.zero_grad), device='cpu', loss_lods=[0, 1, 2],
                               train_dataset=types.SimpleNamespace(sample_tex=True), tracker=types.SimpleNamespace(metrics=metrics),
                               optimizer=opt)
    ref_step(me, {"coords": x, "sdf": y, "rgb": c})
    want = _weighted_loss(fw, x, y, c, [1.0, 1.0, 1.0], [3.0, 2.0, 1.0])
    want.backward()
    assert abs(metrics.total_loss - float(want) * 64) <= 2e-5 * max(1.0, float(want) * 64)
    for (n1, p1), (n2, p2) in zip(fr.named_parameters(), fw.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, rtol=1e-5, atol=1e-8), n1


# ------------------------------------------------------------------------------------------------ 3. ABI
def test_sdf_lods_train_step_is_declared_bound_and_exported():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    assert "int wisp_sdf_lods_train_step(" in header and "int64_t wisp_sdf_lods_train_scratch_bytes(" in header
    assert "wisp_sdf_lods_train_step" in header.split("do not bump it")[0]            # named in the "only ADDED" list
    assert "sdf_trainer.py:80-123" in header and "ascending q" in header and "ascending k" in header
    # the textured step's arguments plus n_out, w_sdf and w_rgb
    assert len(C.SIGNATURES["wisp_sdf_lods_train_step"]) == len(C.SIGNATURES["wisp_sdf_tex_train_step"]) + 3 == 34
    assert len(C.SIGNATURES["wisp_sdf_lods_train_scratch_bytes"]) == 6
    assert C._RESTYPES["wisp_sdf_lods_train_scratch_bytes"] is C.c_i64
    decl = header[header.index("int wisp_sdf_lods_train_step("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == 34
    lib = ctypes.CDLL(C.LIB_PATH)
    assert hasattr(lib, "wisp_sdf_lods_train_step") and hasattr(lib, "wisp_sdf_lods_train_scratch_bytes")
    assert C.lib.wisp_abi_version() == 4
    assert callable(C.sdf_lods_train_step)


def _base_args(n_out=4):
    """a call whose sizes are all valid and whose pointers are all null"""
    null = ctypes.c_void_p(0)
    #       coords gts  rgb   n  octree exsum points trinkets feats levels rows  L  C  half n_out pos w_sdf w_rgb w1 b1 w2 b2   H
    return [null, null, null, 8, null, null, null, null, null, null, null, 3, 16, 0, n_out, 1, null, null, null, null, null, null, 128,
            null, null, null, null, null, null, null, 0, null, 0, null]


def _call(args):
    import wisp._C as C
    rc = C._cdll.wisp_sdf_lods_train_step(*args)
    return rc, C.lib.wisp_last_error().decode()


def test_every_argument_check_fails_before_a_launch_with_its_message():
    """every pointer is null or host memory: nothing may be dereferenced on the device or launched on the way to the refusal"""
    buf = ctypes.create_string_buffer(1 << 16)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    ones = (ctypes.c_float * 16)(*([1.0] * 16))
    wp = ctypes.cast(ones, ctypes.c_void_p)

    def full(n_out=4):
        a = [ptr if isinstance(v, ctypes.c_void_p) else v for v in _base_args(n_out)]
        a[16] = wp
        a[17] = wp if n_out == 4 else ctypes.c_void_p(0)
        if n_out == 1:
            a[2] = ctypes.c_void_p(0)
        a[-1] = ctypes.c_void_p(0)                                             # the null stream
        return a
    for patch, msg in (({3: 0}, "bad sizes"), ({11: 0}, "bad sizes"), ({11: 17}, "bad sizes"), ({12: 8}, "16 feature channels"),
                       ({12: 32}, "16 feature channels"), ({22: 0}, "hidden width"), ({22: 257}, "hidden width"), ({14: 2}, "n_out"),
                       ({14: 0}, "n_out"), ({15: 2}, "pos_input"), ({15: -1}, "pos_input"), ({0: ctypes.c_void_p(0)}, "null pointer"),
                       ({16: ctypes.c_void_p(0)}, "null pointer"), ({28: ctypes.c_void_p(0)}, "null pointer"),
                       ({2: ctypes.c_void_p(0)}, "rgb_gts and w_rgb"), ({17: ctypes.c_void_p(0)}, "rgb_gts and w_rgb"),
                       ({}, "scratch too small")):
        args = full()
        for k, v in patch.items():
            args[k] = v
        rc, err = _call(args)
        assert rc == -1 and msg in err, (patch, rc, err)
    one = full(1)
    one[15] = 0
    rc, err = _call(one)
    assert rc == -1 and "pos_input must be 1" in err, err
    one = full(1)
    one[2] = ptr
    rc, err = _call(one)
    assert rc == -1 and "rgb_gts and w_rgb" in err, err
    # null pointers alone
    rc, err = _call(_base_args())
    assert rc == -1 and "null pointer" in err
    # the weights, with a scratch that is large enough: finite and > 0
    import wisp._C as C
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for slot in (16, 17):
            args = full()
            w = (ctypes.c_float * 16)(*([1.0, bad] + [1.0] * 14))
            args[slot] = ctypes.cast(w, ctypes.c_void_p)
            lv = (ctypes.c_int32 * 3)(1, 2, 3)
            rows = (ctypes.c_int64 * 3)(8, 64, 512)
            pp = (ctypes.c_void_p * 3)(ptr.value, ptr.value, ptr.value)
            args[8] = ctypes.cast(pp, ctypes.c_void_p); args[9] = ctypes.cast(lv, ctypes.c_void_p); args[10] = ctypes.cast(rows, ctypes.c_void_p)
            args[23] = ctypes.cast(pp, ctypes.c_void_p)
            args[30] = int(C.lib.wisp_sdf_lods_train_scratch_bytes(8, 3, 16, 128, 4, 1))
            rc, err = _call(args)
            assert rc == -1 and "finite and > 0" in err, (bad, slot, err)


def test_scratch_bytes_is_monotone_and_rejects_bad_arguments():
    import wisp._C as C
    g = C.lib.wisp_sdf_lods_train_scratch_bytes
    for n_out, pos in ((1, 1), (4, 0), (4, 1)):
        for lods in (1, 3, 6, 16):
            sizes = [int(g(n, lods, 16, 128, n_out, pos)) for n in (0, 1, 2, 37, 512, 513, 5000, 100000, 1 << 20)]
            assert sizes[0] >= 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[1] > 0, (n_out, pos, lods, sizes)
    assert int(g(512, 6, 16, 128, 4, 1)) > int(g(512, 6, 16, 128, 4, 0)) and int(g(512, 6, 16, 128, 4, 1)) > int(g(512, 6, 16, 128, 1, 1))
    assert int(g(512, 6, 16, 256, 4, 1)) > int(g(512, 6, 16, 128, 4, 1))
    # d features is [n][L 16] here, [n][16] in the one-LOD step
    assert int(g(100000, 6, 16, 128, 4, 1)) > int(C.lib.wisp_sdf_tex_train_scratch_bytes(100000, 6, 16, 128, 1)) + 100000 * 5 * 16 * 4 - 4096
    for bad in ((-1, 3, 16, 128, 4, 1), (512, 0, 16, 128, 4, 1), (512, 17, 16, 128, 4, 1), (512, 3, 8, 128, 4, 1), (512, 3, 32, 128, 4, 1),
                (512, 3, 16, 0, 4, 1), (512, 3, 16, 257, 4, 1), (512, 3, 16, 128, 4, 2), (512, 3, 16, 128, 4, -1), (512, 3, 16, 128, 2, 1),
                (512, 3, 16, 128, 0, 1), (512, 3, 16, 128, 1, 0)):
        assert int(g(*bad)) == -1, bad


# ------------------------------------------------------------------------------------------------ 4. resources
@pytest.mark.skipif(not kernel_meta.available(LIB), reason="libwisp_hip.so not built or llvm-readelf missing")
def test_the_kernels_have_no_scratch_256_threads_and_dynamic_lds_only():
    meta = kernel_meta.kernels(LIB)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    for part in ("void sdf_lods_train_kernel<1>(", "void sdf_lods_train_kernel<4>(", "sdf_lods_train_reduce_kernel("):
        hits = {n: v for n, v in kern.items() if n.startswith(part)}
        assert len(hits) == 1, (part, list(hits))
        for name, v in hits.items():
            assert v["scratch"] == 0 and v["wg"] == 256, (name, v)
            assert "reduce" in part or v["lds"] == 0, (name, v)


def test_the_largest_shape_fits_the_lds():
    """hidden 256, four outputs, the position in front: the layout restated from st_lods_layout stays under the 160 KB of a CU"""
    H, in_dim, n_out, G = 256, 19, 4, 16
    floats = H * (in_dim | 1) + H + n_out * H + G * in_dim + 2 * G * H + G * n_out + G * 3 + 2 * G * 16 + 32
    entries = H * in_dim + H + n_out * H + n_out + 2 * 16 + 1
    assert (floats + entries) * 4 < 96 * 1024
    src = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "spc_grad.hip")).read()
    assert "WISP_ALLOW_LDS(sdf_lods_train_kernel<NOUT>, lds)" in src


# ------------------------------------------------------------------------------------------------ 5. SDFTrainStep's rules
class _Blas:
    pass


def _bare(only_last, **attrs):
    from wisp.trainers import SDFTrainStep
    s = SDFTrainStep.__new__(SDFTrainStep)
    s.only_last = only_last
    s.fused_hash = s.fused_triplane = False
    s.textured = False
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


def test_fused_field_rules_on_the_host(monkeypatch):
    """without a GPU nothing is fused; what is checked here is which branch is ASKED: with only_last=False the octree branches are
    reached only in a trainer built with fused_lods=True, a hash or triplanar grid never - and a trainer object without the attribute
    (built with __new__, as tests/test_abi_and_host.py does) reads as fused_lods=False"""
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import HashGrid, OctreeGrid, TriplanarGrid
    from wisp.models.nefs import NeuralSDF
    from wisp.models.nefs.neural_sdf_tex import NeuralSDFTex
    from wisp.trainers import SDFTrainStep
    import inspect
    assert inspect.signature(SDFTrainStep.__init__).parameters["fused_lods"].default is False
    blas = OctreeAS.make_dense(2)
    grid = OctreeGrid(blas, feature_dim=16, num_lods=2, multiscale_type='sum', feature_std=0.05)
    plain = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=16, num_layers=1)
    tex = NeuralSDFTex(grid, embedder_type='none', hidden_dim=16)
    asked = []
    monkeypatch.setattr(SDFTrainStep, "_fused_field_tex", lambda self, g, d: asked.append("tex") or None)
    monkeypatch.setattr(SDFTrainStep, "_fused_field_hash", lambda self, g, d: asked.append("hash") or None)
    monkeypatch.setattr(SDFTrainStep, "_fused_field_triplane", lambda self, g, d: asked.append("triplane") or None)
    for only_last, flag, want in ((True, False, ["tex"]), (True, True, ["tex"]), (False, False, []), (False, True, ["tex"])):
        asked.clear()
        s = SDFTrainStep(tex, only_last=only_last, fused_lods=flag)
        assert s.fused_lods is flag and s._fused_field() is None and asked == want, (only_last, flag, asked)
    # toggled under a live trainer: the decision is taken afresh
    s = SDFTrainStep(tex, only_last=True, fused_lods=False)
    asked.clear()
    s._fused_field()
    s.only_last = False
    s._fused_field()
    assert asked == ["tex"]
    s.fused_lods = True
    s._fused_cache = None
    s._fused_field()
    assert asked == ["tex", "tex"]
    # no attribute at all
    b = _bare(False, nef=tex, flat=types.SimpleNamespace(data=torch.zeros(1)))
    asked.clear()
    assert b._fused_field() is None and asked == []
    # hash and triplanar grids with only_last=False stay modular, opt-ins and fused_lods notwithstanding
    hg = types.SimpleNamespace(grid=HashGrid.__new__(HashGrid), decoder=object())
    tg = types.SimpleNamespace(grid=TriplanarGrid.__new__(TriplanarGrid), decoder=object())
    for nef in (hg, tg):
        for only_last in (True, False):
            asked.clear()
            b = _bare(only_last, nef=nef, fused_hash=True, fused_triplane=True, fused_lods=True, flat=types.SimpleNamespace(data=torch.zeros(1)))
            assert b._fused_field() is None
            assert asked == ((["hash"] if nef is hg else ["triplane"]) if only_last else []), (only_last, asked)
    assert SDFTrainStep(plain, only_last=False, fused_lods=True)._fused_field() is None          # on the CPU: modular


def test_fused_still_valid_follows_only_last_and_the_flag():
    """a cache entry goes stale when only_last no longer matches what it was decided for, or when an all-LOD entry meets a trainer
    without the flag; otherwise the parameter comparison behind those rules answers (here: no parameters, none re-homed)"""
    from wisp.trainers import SDFTrainStep
    w = torch.nn.Parameter(torch.zeros(2, 2))
    w.grad = torch.zeros(2, 2)
    lin = types.SimpleNamespace(weight=w, bias=w)
    grid = types.SimpleNamespace(num_lods=0, features=[])
    dec = types.SimpleNamespace(layers=[lin], lout=lin)
    nef = types.SimpleNamespace(grid=grid, decoder=dec)
    entry = dict(grid=grid, dec=dec, lods=0, prm=[w, w, w, w])
    for only_last, flag, marked, ok in ((True, None, False, True), (True, False, False, True), (False, True, True, True),
                                        (False, True, False, False), (True, True, True, False), (False, False, True, False),
                                        (False, None, True, False)):
        s = _bare(only_last, nef=nef)
        if flag is not None:
            s.fused_lods = flag
        c = dict(entry, lods_loss=True) if marked else dict(entry)
        assert SDFTrainStep._fused_still_valid(s, c) is ok, (only_last, flag, marked)


# ------------------------------------------------------------------------------------------------ 6. the script
def test_train_nglod_takes_all_lods(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train_nglod
    finally:
        sys.path.pop(0)
    import wisp.trainers as T
    assert "--all-lods" in train_nglod.__doc__ and "fused_lods=True" in train_nglod.__doc__
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
    from wisp.accelstructs import OctreeAS
    from wisp.models.grids import OctreeGrid
    from wisp.models.nefs import NeuralSDF
    grid = OctreeGrid(OctreeAS.make_dense(2), feature_dim=16, num_lods=2, multiscale_type='sum', feature_std=0.05)
    nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=16, num_layers=1)
    cfg = types.SimpleNamespace(optimizer=types.SimpleNamespace(lr=1e-3, eps=1e-15, betas=(0.9, 0.999)), grid_lr_weight=1.0,
                                dataloader=types.SimpleNamespace(batch_size=4), only_last=False, max_epochs=1, resample=False)
    ds = types.SimpleNamespace(data=dict(coords=torch.zeros(8, 3), sdf=torch.zeros(8)))
    trainer = types.SimpleNamespace(pipeline=types.SimpleNamespace(nef=nef))
    assert train_nglod.fit_fused(trainer, ds, cfg, "cpu", fused_lods=True) is False
    assert seen[-1]["fused_lods"] is True and seen[-1]["only_last"] is False
    assert train_nglod.fit_fused(trainer, ds, cfg, "cpu") is False
    assert seen[-1]["fused_lods"] is False
    # validate_every_lod: every LOD for the call, the trainer's own selection afterwards
    asked = []
    tr = types.SimpleNamespace(pipeline=types.SimpleNamespace(nef=nef), validate=lambda: asked.append(list(tr.loss_lods)) or {"m": [1.0, 2.0]})
    assert train_nglod.validate_every_lod(tr) == {"m": [1.0, 2.0]} and asked == [[0, 1]] and not hasattr(tr, "loss_lods")
    tr.loss_lods = [1]
    train_nglod.validate_every_lod(tr)
    assert tr.loss_lods == [1]
    src = open(os.path.join(ROOT, "scripts", "train_nglod.py")).read()
    assert "fused_lods_step=fused_lods_step" in src and "all_lods=bool(args.all_lods)" in src and "only_last=not args.all_lods" in src
    script = os.path.join(ROOT, "scripts", "train_nglod.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--all-lods" in r.stdout
    for grid_name, opt in (("hash", "--fused-step"), ("triplanar", "--fused-kernel")):
        r = subprocess.run([sys.executable, script, "mesh.obj", "--grid", grid_name, "--all-lods", opt], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--all-lods has no fused step" in r.stderr and grid_name in r.stderr, (grid_name, r.stderr[-500:])


def test_bench_script_is_there():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_sdf_lods_step.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "--num-lods" in r.stdout


# ------------------------------------------------------------------------------------------------ 7. what the GPU shapes reach
def test_coverage_claims_of_the_gpu_file():
    for (tree, levels) in R.LEVEL_LISTS:
        L = len(levels)
        for n in R.NS:
            s = R.launch_shape(L, n)
            assert (s["spb"], s["idle_groups"]) == R.COVERAGE[L], (L, n, s)
            assert s["max_passes"] == 1 and not s["second_pass_all"]
    assert set(len(l) for _, l in R.LEVEL_LISTS) == {1, 2, 3, 6, 8, 9}
    assert R.launch_shape(6, 1)["tail_pass"] and R.launch_shape(3, 16)["tail_pass"] and not R.launch_shape(2, 16)["tail_pass"]
    two = R.launch_shape(len(R.TWO_PASS[1]), R.TWO_PASS[2])
    assert two["spb"] == 1 and two["grid"] == X.GRID_CAP and two["second_pass_all"] and two["max_passes"] == 2
    big = R.launch_shape(len(R.INEXACT_BIG[1]), R.INEXACT_BIG[2])
    assert big["grid"] == X.GRID_CAP and big["second_pass_some"] and big["tail_pass"]
    for n in R.INEXACT_NS:
        assert n & (n - 1) != 0 and R.launch_shape(3, n)["tail_pass"] and R.launch_shape(3, n)["idle_groups"] == 1
    assert R.HIDDENS == (1, 17, 128, 256)


def test_the_two_pass_shape_with_colours_is_refused_for_its_loss():
    """recorded here: the textured 9-level case at n = 2048 is no exact case at any rung (so the GPU file runs the two-pass exact
    case on the plain field and the textured second pass in the bounded test)"""
    tree, levels, n = R.TWO_PASS
    with pytest.raises(AssertionError, match="loss"):
        R.exact_lods_case(tree, levels, n, 24, tex=True, pos_input=0)
