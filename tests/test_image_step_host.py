"""CPU: the host side of the fused image training step (wisp_image_field_train_step, csrc/image_field_train.hip;
ImageTrainStep(fused=True)): declaration / binding / export agreement, argument checks that return before any launch, the two
kernels' resources, the float64 reference of tests/image_step_ref.py against torch autograd through the 2-D oracle lookup, its
exact-case generator ("twin levels"), ImageTrainStep's gates on the host and the script's option wiring."""
import ctypes
import os
import sys
import types

import pytest
import torch

import kernel_meta
import image_step_ref as S
from oracle import hashgrid as ohg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "libwisp_hip.so")
STEP, BYTES = "wisp_image_field_train_step", "wisp_image_field_train_scratch_bytes"
LDS_LIMIT = 160 * 1024                                   # one workgroup may hold the whole LDS of a compute unit


# ------------------------------------------------------------------------------------------------ 1. ABI and argument checks
def test_the_two_entry_points_are_declared_bound_and_exported():
    import wisp._C as C
    header = open(os.path.join(ROOT, "include", "wisp_hip.h")).read()
    assert f"int {STEP}(" in header and f"int64_t {BYTES}(" in header
    comment = header[header.index(f"int64_t {BYTES}(") - 3500:header.index(f"int64_t {BYTES}(")]
    assert "wisp/trainers/image_trainer.py" in comment and "`step`" in comment and "image_nef.py" in comment
    assert STEP in C.SIGNATURES and BYTES in C.SIGNATURES and len(C.SIGNATURES[BYTES]) == 3
    # coords, rgb, n | table: codebook, first_idx, resolutions, num_lods, active_lods, bitwidth | w1, b1, w2, b2, hidden | five
    # gradients | loss, pred | scratch, scratch_bytes, stream
    assert len(C.SIGNATURES[STEP]) == 3 + 6 + 5 + 5 + 2 + 3
    # the table arguments in wisp_image_field_render's order
    assert C.SIGNATURES[STEP][3:9] == C.SIGNATURES["wisp_image_field_render"][5:11]
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
    assert callable(C.image_field_train_step)
    mk = open(os.path.join(ROOT, "kaolin-wisp_amd", "csrc", "Makefile")).read()
    assert "image_field_train.hip" in mk and "image_field_dev.h" in mk
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.image_field_train_step(torch.zeros(4, 2), torch.zeros(4, 3), {}, None, None, None, None, None)


# positions in the argument list
COORDS, RGB, N, CODEBOOK, BEGIN, RES, LODS, ACTIVE, BITS, W1, B1, W2, B2, HIDDEN = range(14)
G_TABLE, G_W1, G_B1, G_W2, G_B2, LOSS, PRED, SCRATCH, SCRATCH_BYTES, STREAM = range(14, 24)


def _host_args(resolutions=(16, 40, 101, 256), bits=12, hidden=64, n=8, active=None):
    """a call whose sizes are valid and whose pointers point at host memory: nothing may be dereferenced on the way to a refusal
    (first_idx and resolutions are host arrays by contract)"""
    import wisp._C as C
    buf = ctypes.create_string_buffer(4096)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    L = len(resolutions)
    begin = S.layout(resolutions, bits)
    bi = (ctypes.c_int64 * (L + 1))(*[int(b) for b in begin])
    rs = (ctypes.c_int32 * max(L, 1))(*resolutions)
    need = int(C.lib.wisp_image_field_train_scratch_bytes(n, L, hidden))
    args = [ptr, ptr, n, ptr, bi, rs, L, L - 1 if active is None else active, bits, ptr, ptr, ptr, ptr, hidden] + [ptr] * 8 + \
           [need, ctypes.c_void_p(0)]
    return args, (buf, bi, rs)


def test_argument_checks_are_returned_before_any_launch():
    """every refusal comes back as WISP_ERR_INVALID with a text, with host pointers in every slot: had anything been launched or
    dereferenced on the way, this process would not be here to say so"""
    import wisp._C as C
    f = C._cdll.wisp_image_field_train_step
    null = ctypes.c_void_p(0)
    args, keep = _host_args()
    assert args[SCRATCH_BYTES] > 0
    bad = [{LODS: 0}, {LODS: 17}, {ACTIVE: -1}, {ACTIVE: 5}, {HIDDEN: 0}, {HIDDEN: 129}, {N: 0}, {N: -1}, {N: (1 << 22) + 1}, {BITS: 0},
           {BITS: 31}] + \
          [{k: null} for k in (COORDS, RGB, CODEBOOK, BEGIN, RES, W1, B1, W2, B2, G_TABLE, G_W1, G_B1, G_W2, G_B2, LOSS, SCRATCH)]
    for patch in bad:
        args, keep = _host_args()
        for k, v in patch.items():
            args[k] = v
        assert f(*args) == -1, patch                                               # WISP_ERR_INVALID
        assert C.lib.wisp_last_error(), patch
    # pred alone may be NULL - that call would launch, so it is not made here; 2^22 samples pass the size check and fail the next
    args, keep = _host_args(n=1 << 22)
    args[SCRATCH_BYTES] -= 1
    assert f(*args) == -1 and b"scratch too small" in C.lib.wisp_last_error()
    # scratch one byte short
    args, keep = _host_args()
    args[SCRATCH_BYTES] -= 1
    assert f(*args) == -1 and b"scratch too small" in C.lib.wisp_last_error()
    # a level with fewer rows than an index reaches: the hashed last level (256^2 >= 2^12 rows), then a dense one (16^2 rows)
    args, keep = _host_args()
    args[BEGIN][4] -= 1
    assert f(*args) == -1 and b"fewer rows" in C.lib.wisp_last_error()
    args, keep = _host_args()
    args[BEGIN][0] += 1
    assert f(*args) == -1 and b"fewer rows" in C.lib.wisp_last_error()


def test_scratch_bytes_is_monotone_and_rejects_what_the_step_does_not_serve():
    import wisp._C as C
    g = C.lib.wisp_image_field_train_scratch_bytes
    sizes = [int(g(n, 16, 64)) for n in (1, 2, 16, 17, 512, 513, 4096, 5000, 1 << 16, 1 << 22)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], sizes
    assert int(g(4096, 16, 128)) > int(g(4096, 16, 64)) > int(g(4096, 4, 64))
    # one fp64 partial row per workgroup of 16 samples (at most 256 workgroups), rows padded to 16 entries, and 2^16 fp64
    # accumulators for every level: image_hash.yaml at 4096 pixels
    assert int(g(4096, 16, 64)) == 256 * ((64 * 46 + 4 * 64 + 4 + 15) // 16 * 16) * 8 + 16 * 65536 * 8
    for bad in ((0, 16, 64), (-1, 16, 64), ((1 << 22) + 1, 16, 64), (512, 0, 64), (512, 17, 64), (512, 16, 0), (512, 16, 129)):
        assert int(g(*bad)) == -1, bad
    assert int(g(1 << 22, 16, 128)) > 0 and int(g(1, 1, 1)) > 0                    # the largest and the smallest admitted shapes


def step_lds_bytes(hidden, num_lods):
    """the dynamic LDS of image_field_train_kernel (csrc/image_field_train.hip: ift_lds_bytes), restated"""
    in_dim = 2 * num_lods + 14
    row = (hidden * in_dim + 4 * hidden + 4 + 15) // 16 * 16
    return 8 * row + 4 * (hidden * (in_dim | 1) + 4 * hidden + 4 + 16 * (in_dim + 2 * hidden + 8 + 32))


def test_the_two_kernels_have_no_scratch_and_the_largest_shape_fits_the_lds():
    assert kernel_meta.available(LIB), "libwisp_hip.so not built or llvm-readelf missing"
    meta = kernel_meta.kernels(LIB)
    names = kernel_meta.demangled(list(meta))
    kern = {names[k]: v for k, v in meta.items()}
    for part in ("image_field_train_kernel", "image_field_train_reduce_kernel"):
        hits = {n: v for n, v in kern.items() if part + "(" in n}
        assert len(hits) == 1, (part, list(hits))
        for name, v in hits.items():
            assert v["scratch"] == 0 and v["wg"] == 256 and v["lds"] == 0 and v["vgpr"] + v["agpr"] <= 128, (name, v)
    # the render kernel, now made of the shared __device__ functions, keeps its resources
    hits = [v for n, v in kern.items() if "image_field_render_kernel(" in n]
    assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["wg"] == 256 and hits[0]["vgpr"] + hits[0]["agpr"] <= 128
    # dynamic LDS only, raised past the 64 KB default through WISP_ALLOW_LDS; every admitted shape fits one workgroup's 160 KiB
    worst = max(step_lds_bytes(H, L) for H in range(1, 129) for L in range(1, 17))
    assert worst == step_lds_bytes(128, 16) == 99344 and worst <= LDS_LIMIT
    assert step_lds_bytes(64, 16) == 52496                                        # image_hash.yaml: two workgroups a compute unit


# ------------------------------------------------------------------------------------------------ 2. the float64 reference
@pytest.mark.parametrize("bitwidth", [6, 12])
@pytest.mark.parametrize("L,hidden,active", [(1, 1, 1), (5, 17, 4), (16, 64, 15), (4, 8, 0)])
def test_reference_equals_autograd_through_the_oracle_lookup(L, hidden, active, bitwidth):
    """the written-out gradients against torch autograd through the same float64 forward (rounding of float64 sums only); the
    forward's features against oracle.hashgrid.hashgrid_forward (fp32 blends: 4 roundings of factors and sums per level) and the
    table gradient against oracle.hashgrid.hashgrid_backward fed with the reference's feature gradient"""
    fld = S.generic_field(L, hidden, active, bitwidth, seed=7)
    coords, rgb = S.generic_points(300, seed=3), S.generic_targets(300, seed=3)
    got, want = S.step_reference(fld, coords, rgb), S.autograd_reference(fld, coords, rgb)
    for k in ("loss", "pred") + S.GRADS:
        assert got[k].shape == want[k].shape, k
        scale = max(float(want[k].abs().max()), 1e-30)
        assert float((got[k] - want[k]).abs().max()) <= 1e-12 * scale + 1e-18, k
    assert bool((coords.abs() > 1).any()) and float(got["loss"]) > 0
    orc = ohg.hashgrid_forward(coords, fld["table"], fld["begin"], fld["resolutions"], fld["bitwidth"]).double()
    mine = S.features(fld, coords)
    if active:
        assert float((mine[:, :2 * active] - orc[:, :2 * active]).abs().max()) <= 8 * 2.0 ** -24 * float(fld["table"].abs().max())
    assert bool((mine[:, 2 * active:] == 0).all())
    p = S.decoder_parts(fld, coords, rgb)
    full = p["dfeat"].clone()
    full[:, 2 * active:] = 0
    shape = tuple(fld["table"].shape)
    orc = ohg.hashgrid_backward(coords, full, shape, fld["begin"], fld["resolutions"], fld["bitwidth"], accum_dtype=torch.float64)
    mass = ohg.hashgrid_backward(coords, full.abs(), shape, fld["begin"], fld["resolutions"], fld["bitwidth"], accum_dtype=torch.float64)
    assert bool(((got["table"] - orc).abs() <= 4 * 2.0 ** -24 * mass + 1e-30).all())
    begin = fld["begin"]
    assert bool((got["table"][int(begin[active]):] == 0).all())                    # the levels from `active` on stay untouched
    assert bool((got["w1"][:, 2 * active:2 * L] == 0).all()) and bool((got["w1"][:, 2 * L:] != 0).any())
    assert active == 0 or bool((got["table"][:int(begin[active])] != 0).any())


@pytest.mark.parametrize("n", S.EXACT_N)
@pytest.mark.parametrize("res,active,bitwidth,hidden", S.EXACT_FIELDS)
def test_exact_cases_are_exact(res, active, bitwidth, hidden, n):
    """the generator's own assertions ran when the case was built (every term on one quantum grid, abs-sums below 2^24 quanta,
    outputs exactly zero); here: float64 and autograd agree BIT FOR BIT - exact sums have no order -, every exact result is an fp32
    value, and the fp32 forward's features equal the float64 ones"""
    case = S.exact_case(res, active, bitwidth, hidden, n, seed=2)
    fld, coords, rgb, want = case["field"], case["coords"], case["rgb"], case["want"]
    L2 = 2 * len(res)
    assert set(case["spans"]) == {"blend", "hidden", "loss", "b2", "w2", "dh", "b1", "w1", "dfeat", "table"}
    assert max(case["spans"].values()) < 2.0 ** 24
    auto = S.autograd_reference(fld, coords, rgb)
    for k in ("loss", "pred", "table", "b1", "w2", "b2"):
        assert torch.equal(auto[k], want[k]), k
        assert torch.equal(want[k].float().double(), want[k]), k
    assert torch.equal(auto["w1"][:, :L2], want["w1"][:, :L2]) and torch.equal(want["w1"][:, :L2].float().double(), want["w1"][:, :L2])
    assert bool((want["pred"] == 0.5).all()) and float(want["loss"]) > 0
    orc = ohg.hashgrid_forward(coords, fld["table"], fld["begin"], fld["resolutions"], fld["bitwidth"]).double()
    assert torch.equal(orc[:, :2 * active], S.features(fld, coords)[:, :2 * active])
    dense = [ohg.level_is_dense(r, 2 ** bitwidth, 2) for r in res]
    assert dense == [r * r < 2 ** bitwidth for r in res]
    if hidden >= 16 and n >= 64 and S.twin_pairs(fld):
        assert bool((want["w2"] != 0).any()) and bool((want["table"] != 0).any())
        assert bool((want["w1"][:, L2:] != 0).any())                               # the embedding columns do get a gradient
    if active == 15:
        assert case["unread"] == [14]


def test_the_reference_case_has_the_intended_structure():
    """resolutions (8, 8, 32, 32, 64), 4 active, bitwidth 8, hidden 64, n = 512: two dense levels, two hashed levels and a dead
    finest one; every output exactly 0; a good part of the hidden units live; many table entries moved"""
    c = S.CHECKED
    case = S.exact_case(c["resolutions"], c["active"], c["bitwidth"], c["hidden"], 512, seed=2)
    fld, want = case["field"], case["want"]
    assert [ohg.level_is_dense(r, 256, 2) for r in c["resolutions"]] == [True, True, False, False, False]
    p = S.decoder_parts(fld, case["coords"], case["rgb"])
    live = float((p["a"] > 0).double().mean())
    assert 0.25 <= live <= 0.75, live
    moved = int((want["table"] != 0).sum())
    assert moved > 500 and bool((want["table"][int(fld["begin"][4]):] == 0).all())
    assert max(case["spans"].values()) < 2.0 ** 22                               # (the pre-fill of 2 alone is 2^21 quanta)


def test_an_inexact_case_is_refused():
    c = S.CHECKED
    case = S.exact_case(c["resolutions"], c["active"], c["bitwidth"], c["hidden"], 64, seed=2)
    fld, coords, rgb = case["field"], case["coords"], case["rgb"]
    with pytest.raises(AssertionError, match="power of two"):
        S.check_exact(fld, coords[:3], rgb[:3])
    bent = coords.clone()
    bent[5, 0] += 2.0 ** -12                                                       # a non-dyadic blend
    with pytest.raises(AssertionError, match="quantum"):
        S.check_exact(fld, bent, rgb)
    with pytest.raises(AssertionError, match="quantum"):
        S.check_exact(fld, coords, rgb + 2.0 ** -10)
    with pytest.raises(AssertionError, match="leave fp32"):
        S.check_exact(fld, coords, rgb, prefill=2.0 ** 22)
    with pytest.raises(AssertionError):
        S.check_exact(fld, S.generic_points(64, seed=1), rgb)


# ------------------------------------------------------------------------------------------------ 3. ImageTrainStep and the script
def _cpu_nef(hidden=16, lods=4, bitwidth=8):
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import ImageNeuralField
    torch.manual_seed(3)
    grid = HashGrid.from_geometric(None, feature_dim=2, num_lods=lods, multiscale_type='cat', feature_std=0.05,
                                   codebook_bitwidth=bitwidth, min_grid_res=16, max_grid_res=64)
    return ImageNeuralField(grid, hidden_dim=hidden)


def _cpu_hashgrid(coords, codebook_bitwidth, lod_idx, codebook, zero_from_col=None):
    """wisp.ops.grid.hashgrid on the host: the oracle's autograd function, with the kernel's fused zeroing as a mask"""
    out = ohg.hashgrid(coords, codebook.resolutions, codebook_bitwidth, lod_idx, codebook.feats, codebook.begin_idxes)
    if zero_from_col is not None:
        keep = torch.ones(out.shape[-1], dtype=out.dtype)
        keep[zero_from_col:] = 0
        out = out * keep
    return out


def test_a_cpu_field_takes_the_modular_path_and_the_default_never_asks(monkeypatch):
    import wisp._C as C
    import wisp.models.grids.hash_grid as hg
    from wisp.trainers import ImageTrainStep

    def never(*a, **k):
        raise AssertionError("the fused image step was taken")
    monkeypatch.setattr(C, "image_field_train_step", never)
    monkeypatch.setattr(hg.grid_ops, "hashgrid", _cpu_hashgrid)
    monkeypatch.delenv("WISP_IMAGE_TRAIN_FUSED", raising=False)
    asked, default = ImageTrainStep(_cpu_nef(), fused=True), ImageTrainStep(_cpu_nef())
    assert asked.fused and not default.fused
    assert asked._fused_field() is None and default._fused_field() is None
    coords, rgb = S.generic_points(32, seed=1), S.generic_targets(32, seed=1)
    la, ld = asked._forward_backward(coords, rgb), default._forward_backward(coords, rgb)
    assert torch.equal(la, ld) and la.ndim == 0 and float(la) > 0
    assert bool((asked.flat.grad != 0).any()) and torch.equal(asked.flat.grad, default.flat.grad)
    # the default never looks at the field's shape at all
    import wisp.models.nefs.image_nef as image_nef
    monkeypatch.setattr(image_nef, "fused_render_shape", never)
    default._fused_cache = None
    assert default._fused_field() is None


def test_fused_field_follows_the_shape_rules_and_what_changes_under_a_live_trainer(monkeypatch):
    """the rules on CPU objects that claim to live on the GPU (nothing is launched): every tensor answers is_cuda with True"""
    from wisp.trainers import ImageTrainStep
    monkeypatch.delenv("WISP_IMAGE_TRAIN_FUSED", raising=False)
    monkeypatch.delenv("WISP_IMAGE_RENDER_FUSED", raising=False)
    steps = dict(asked=ImageTrainStep(_cpu_nef(), fused=True), default=ImageTrainStep(_cpu_nef()),
                 wide=ImageTrainStep(_cpu_nef(hidden=129), fused=True))
    assert steps["asked"]._fused_field() is None                                    # on the host nothing is fused
    steps["asked"]._fused_cache = None
    monkeypatch.setattr(torch.Tensor, "is_cuda", True, raising=False)
    ok = steps["asked"]._fused_field()
    nef = steps["asked"].nef
    assert ok is not None and ok["grid"] is nef.grid and ok["lods"] == 4
    assert ok["host"] == dict(begin_idxes=nef.grid.codebook.begin_idxes.tolist(), resolutions=[16, 25, 40, 63], codebook_bitwidth=8,
                              active_lods=3)
    assert ok["prm"][0] is nef.grid.codebook.feats and len(ok["prm"]) == 5
    assert steps["asked"]._fused_field() is ok                                      # cached
    assert steps["default"]._fused_field() is None and steps["wide"]._fused_field() is None
    assert steps["asked"]._fused_still_valid(ok)
    grad = nef.grid.codebook.feats.grad
    nef.grid.codebook.feats.grad = None
    assert not steps["asked"]._fused_still_valid(ok) and steps["asked"]._fused_field() is None
    nef.grid.codebook.feats.grad = grad
    steps["asked"]._fused_cache = None
    assert steps["asked"]._fused_field() is not None
    monkeypatch.setenv("WISP_IMAGE_TRAIN_FUSED", "0")
    steps["asked"]._fused_cache = None
    assert steps["asked"]._fused_field() is None


def test_train_image_wires_fused_kernel(monkeypatch, tmp_path):
    """--fused-kernel implies --fused-step and builds ImageTrainStep(..., fused=True); --fused-step alone leaves it off; the JSON
    record carries fused_image_step (no device: dataset, trainer and step are stand-ins)"""
    import json
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train_image
    finally:
        sys.path.pop(0)
    import wisp.trainers as T
    assert "--fused-kernel" in train_image.__doc__ and "fused_image_step" in train_image.__doc__
    seen = []

    class Step:
        def __init__(self, nef, **kw):
            seen.append(kw)

        def _fused_field(self):
            return {} if seen[-1]["fused"] else None

        def set_schedule(self, milestones, gamma):
            pass

        def capture(self, n):
            return self

        def step(self, coords, rgb):
            return torch.zeros(())

    class Trainer:
        def __init__(self, cfg, pipeline, ds, tracker=None, device=None):
            self.cfg, self.iterations_per_epoch = cfg, 2

        def validate(self):
            return dict(psnr=20.0)

    class DS:
        h = w = 8

        def __getitem__(self, i):
            return torch.zeros(4, 2), torch.zeros(4, 3)

    monkeypatch.setattr(T, "ImageTrainStep", Step)
    monkeypatch.setattr(T, "ImageTrainer", Trainer)
    monkeypatch.setattr(train_image, "build", lambda *a, **k: (DS(), types.SimpleNamespace(nef=object())))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for flags, fused in ((["--fused-kernel"], True), (["--fused-step"], False), (["--fused-step", "--fused-kernel"], True)):
        out = []
        monkeypatch.setattr("builtins.print", lambda text, out=out: out.append(text))
        train_image.main(["--write-test-image", str(tmp_path / "img.png"), "--size", "8", "8", "--epochs", "1", "--device", "cpu"] + flags)
        rec = json.loads(out[-1])
        assert seen[-1]["fused"] is fused and rec["fused_image_step"] is fused and rec["step"] == "ImageTrainStep"
    src = open(os.path.join(ROOT, "scripts", "train_image.py")).read()
    assert "fused_image_step=fused_image_step" in src
    bench = open(os.path.join(ROOT, "scripts", "bench_image_fit.py")).read()
    assert '"train_step_fused"' in bench and '"train_step_fused_captured"' in bench
