"""Exact-arithmetic tests of the fused NeRF decoder kernels (csrc/nerf_mlp.hip, nerf_mlp_bf16.hip, nerf_mlp_wide.hip).

The inputs of tests/decoder_exact_ref.py make every value a kernel rounds exactly representable, so each kernel must equal
the plain float64 reference BIT FOR BIT, element by element: `torch.equal`, no tolerance.  The one exception is rgb in the
`general` mode (any z), which goes through the sigmoid: |rgb - sigmoid(z)| <= 1e-6.  Derivation: the bf16 kernels compute
1 / (1 + exp(-z)) with v_exp_f32 and v_rcp_f32, one ulp each (2 x 2^-23 relative, on a value <= 1); scaling the argument by
log2(e) loses |z| 2^-24 relative in the exponent's argument, which the sigmoid damps by sigma (1 - sigma) <= 1/4 - their sum
stays below 3e-7 for every z.

A bitwise mismatch on exact inputs is a defect of the kernel (tests/test_decoder_exact_host.py rules out the reference):
the assertion message names the layer, row and column of the first mismatching parameters.
"""
import pytest
import torch

import decoder_exact_ref as R
from gpu_helpers import DEV, margin, _C

pytestmark = pytest.mark.gpu

# name -> (hidden, bf16 compute, per-ray view code)
KERNELS = {"h64_bf16": (64, True, False), "h64_fp32": (64, False, False), "h64_rays": (64, True, True), "h128_bf16": (128, True, False)}
IO = [torch.float32, torch.float16, torch.bfloat16]
COLOUR = ("W3", "b3", "W4", "b4", "W5", "b5")
TAIL = 32                       # rows behind the end of every input buffer, filled with values that must never be used
NUM_RAYS = 97

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """the cases (inputs and references on the GPU) are shared by the tests of this file and freed when it finishes"""
    yield
    _cache.clear()


def _padded(t, fill):
    """a view of the first S rows of a buffer whose TAIL further rows hold `fill`"""
    buf = torch.full((t.shape[0] + TAIL,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def _case(hidden, in_dim, S, pattern, mode, cancel=False, keep=True):
    """inputs on the GPU and the float64 reference computed there (its exactness assertions included), shared by the tests"""
    key = (hidden, in_dim, S, pattern, mode, cancel)
    if key in _cache:
        return _cache[key]
    c = R.make_case(hidden, in_dim, S, pattern, mode, cancel)
    d = dict(hidden=hidden, in_dim=in_dim, S=S, mode=mode, params=c["params"].to(DEV),
             feats=c["feats"].to(DEV), dirs=_padded(c["dirs"].to(DEV), 1.0),
             grad_rgb=_padded(c["grad_rgb"].to(DEV), 8.0), grad_density=_padded(c["grad_density"].to(DEV), 7.0))
    ref = R.reference(d["params"], d["feats"], d["dirs"], d["grad_rgb"], d["grad_density"], hidden)
    d["density"] = ref["density"].float()
    d["sigmoid_z"] = ref["rgb"]
    d["z"] = ref["z"]
    d["grad_feats"] = ref["grad_feats"]
    d["grad_params"] = ref["grad_params"].float()
    assert torch.equal(d["grad_params"].double(), ref["grad_params"])
    # per-ray view code: a random map onto the rays that includes the last one; the rays no sample uses, and the row behind the
    # table, hold a code that is NOT the code of direction 0
    g = torch.Generator().manual_seed(S + 7 * pattern)
    used = torch.randperm(NUM_RAYS, generator=g)[:60]
    ridx = used[torch.randint(0, 60, (S,), generator=g)]
    if S:
        ridx[int(torch.randint(0, S, (1,), generator=g))] = NUM_RAYS - 1
    d["ridx"] = _padded(ridx.to(DEV), 0)
    if keep:
        _cache[key] = d
    return d


def _ray_code(d):
    code = torch.full((NUM_RAYS + 1, 32), 3.0, dtype=torch.bfloat16, device=DEV)
    code[:NUM_RAYS] = _C().nerf_mlp_dir_code(torch.zeros(NUM_RAYS, 3, device=DEV))
    unused = torch.ones(NUM_RAYS, dtype=torch.bool, device=DEV)
    unused[d["ridx"]] = False
    code[:NUM_RAYS][unused] = 3.0
    return code[:NUM_RAYS]


def _args(kernel, d, io):
    hidden, bf16, rays = KERNELS[kernel]
    assert hidden == d["hidden"]
    feats = _padded(d["feats"].to(io), float("nan"))
    kw = dict(ray_code=(d["ridx"], _ray_code(d))) if rays else {}
    return feats, (None if rays else d["dirs"]), bf16, kw


def _forward(kernel, d, io):
    feats, dirs, bf16, kw = _args(kernel, d, io)
    return _C().nerf_mlp_forward(feats, dirs, d["params"], d["in_dim"], d["hidden"], R.NF, bf16, **kw)


def _backward(kernel, d, io, grad_params=None):
    feats, dirs, bf16, kw = _args(kernel, d, io)
    return _C().nerf_mlp_backward(feats, dirs, d["params"], d["grad_rgb"], d["grad_density"], d["in_dim"], d["hidden"], R.NF, bf16,
                                  grad_params=grad_params, **kw)


def _backward_into(kernel, d, io, grad_feats, grad_params):
    """The C entry point itself, writing grad_feats into a buffer of the caller.  wisp._C.nerf_mlp_backward allocates grad_feats
    (torch.empty_like(feats)) and so cannot be handed a buffer with sentinel rows behind its end; hence this test-only twin
    of its call through the binding's own helpers (pointer, dtype code, stream, status check) with a workspace sized by
    wisp_nerf_mlp_bwd_workspace_bytes as the wrapper does."""
    C = _C()
    feats, dirs, bf16, kw = _args(kernel, d, io)
    S, hidden, in_dim = d["S"], d["hidden"], d["in_dim"]
    need = int(C.lib.wisp_nerf_mlp_bwd_workspace_bytes(S, hidden))
    ws = torch.empty((need + 3) // 4 + 64, dtype=torch.float32, device=DEV)
    p = C._p
    if kw:
        ridx, code = kw["ray_code"]
        rc = C.lib.wisp_nerf_mlp_bwd_rays(p(feats), C._DTYPE_CODE[io], p(code), p(ridx), S, in_dim, hidden, R.NF, p(d["params"]),
                                          p(d["grad_rgb"]), p(d["grad_density"]), p(grad_feats), p(grad_params), p(ws),
                                          ws.numel() * 4, C._stream())
    else:
        rc = C.lib.wisp_nerf_mlp_bwd(p(feats), C._DTYPE_CODE[io], p(dirs), S, in_dim, hidden, R.NF, p(d["params"]),
                                     C.BF16 if bf16 else C.F32, p(d["grad_rgb"]), p(d["grad_density"]), p(grad_feats),
                                     p(grad_params), p(ws), ws.numel() * 4, C._stream())
    C._check(rc, "nerf_mlp_bwd")
    torch.cuda.synchronize()


def _same_params(got, want, d, what):
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want).flatten()
    first = [(R.locate(int(i), d["hidden"], d["in_dim"]), float(got[i]), float(want[i])) for i in bad[:6]]
    layers = sorted({R.locate(int(i), d["hidden"], d["in_dim"])[0] for i in bad[:: max(1, bad.numel() // 500)]})
    raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} parameters differ, in {layers}; (where, got, want): {first}")


def _same_rows(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want)
    first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:6]]
    raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ; (index, got, want): {first}")


def _check_forward(kernel, d, io, tag):
    rgb, den = _forward(kernel, d, io)
    assert rgb.dtype == torch.float32 and rgb.shape == (d["S"], 3) and den.shape == (d["S"], 1)
    _same_rows(den, d["density"], f"{tag} density")
    if d["mode"] == "paired":
        _same_rows(rgb, torch.full_like(rgb, 0.5), f"{tag} rgb (z = 0)")
    elif d["S"]:
        margin(f"decoder exact {tag} max |rgb - sigmoid(z)|", float((rgb.double() - d["sigmoid_z"]).abs().max()), 1e-6)
    return rgb, den


def _check_backward(kernel, d, io, tag):
    gf, gp = _backward(kernel, d, io)
    assert gf.dtype == io and gf.shape == (d["S"], d["in_dim"])
    _same_rows(gf, d["grad_feats"].to(io), f"{tag} grad_feats")
    _same_params(gp, d["grad_params"], d, f"{tag} grad_params")
    if d["mode"] == "general":
        P = R.unpack(gp, d["hidden"], d["in_dim"])
        for name in COLOUR:
            assert not bool(P[name].any()), f"{tag}: d{name} must be exactly zero without a colour gradient"
    return gf, gp


@pytest.mark.parametrize("kernel,pattern", [(k, p) for k in KERNELS for p in range(R.num_patterns(KERNELS[k][0]))])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("io", IO, ids=["f32", "f16", "bf16"])
def test_decoder_equals_float64_reference_bit_for_bit(kernel, io, mode, pattern):
    d = _case(KERNELS[kernel][0], 32, R.S_MAIN, pattern, mode)
    tag = f"{kernel} {mode} p{pattern}"
    _check_forward(kernel, d, io, tag)
    gf, gp = _check_backward(kernel, d, io, tag)
    # grad_params= accumulates: old + new, exactly; and a second call returns the same bits
    old = ((torch.arange(gp.numel(), device=DEV) * 7 + pattern) % 11 - 5).float()
    buf = old.clone()
    gf2, out = _backward(kernel, d, io, grad_params=buf)
    assert out.data_ptr() == buf.data_ptr()
    _same_params(buf, old + d["grad_params"], d, f"{tag} grad_params accumulated onto small integers")
    _same_rows(gf2, gf, f"{tag} grad_feats of a second call")


@pytest.mark.parametrize("pattern", [0, 9])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("io", IO, ids=["f32", "f16", "bf16"])
def test_hidden_64_kernels_agree_bit_for_bit(io, mode, pattern):
    """bf16 compute, fp32 compute and the per-ray view code variant on the same inputs"""
    d = _case(64, 32, R.S_MAIN, pattern, mode)
    outs = {}
    for kernel in ("h64_bf16", "h64_fp32", "h64_rays"):
        _, den = _forward(kernel, d, io)
        gf, gp = _backward(kernel, d, io)
        outs[kernel] = (den, gf, gp)
    for kernel in ("h64_fp32", "h64_rays"):
        _same_rows(outs[kernel][0], outs["h64_bf16"][0], f"density {kernel} vs h64_bf16")
        _same_rows(outs[kernel][1], outs["h64_bf16"][1], f"grad_feats {kernel} vs h64_bf16")
        _same_params(outs[kernel][2], outs["h64_bf16"][2], d, f"grad_params {kernel} vs h64_bf16")
    assert float(outs["h64_bf16"][2].abs().max()) > 0 and float(outs["h64_bf16"][1].float().abs().max()) > 0


@pytest.mark.parametrize("S", R.SHAPE_S)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_sample_counts_around_the_tile(kernel, mode, S):
    """a lone sample, both sides of the 32-sample tile, fewer tiles than wave pairs in a workgroup, several ragged rounds per
    chain wave.  The rows behind the end of grad_rgb / grad_density hold non-zero values: a dead lane of the tail tile that
    used them would change dW2 / db2 (its density pre-activation is positive, see the host test)."""
    d = _case(KERNELS[kernel][0], 32, S, R.SHAPE_PATTERN, mode, keep=S < 10000)
    tag = f"{kernel} {mode} S={S}"
    _check_forward(kernel, d, torch.bfloat16, tag)
    _check_backward(kernel, d, torch.bfloat16, tag)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_no_samples(kernel):
    d = _case(KERNELS[kernel][0], 32, 0, 0, "paired")
    rgb, den = _forward(kernel, d, torch.float32)
    assert rgb.shape == (0, 3) and den.shape == (0, 1)
    gf, gp = _backward(kernel, d, torch.float32)
    assert gf.shape == (0, 32) and not bool(gp.any())


@pytest.mark.parametrize("in_dim", R.WIDTHS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("io", IO, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_feature_widths_and_what_lies_behind_the_rows(kernel, io, mode, in_dim):
    """every I/O type at widths 1, 5, 12, 31, 32 (odd widths: 16-bit rows that start off a 4-byte boundary).  grad_feats is
    written into the first S rows of a longer buffer: the rows behind them must keep their sentinel.  (The kernels take
    dense [S, in_dim] rows - there is no row stride, hence no padding column inside a row to guard.)"""
    d = _case(KERNELS[kernel][0], in_dim, R.S_WIDTHS, R.WIDTH_PATTERN, mode)
    tag = f"{kernel} {mode} in_dim={in_dim}"
    _check_forward(kernel, d, io, tag)
    S = d["S"]
    gbuf = torch.full((S + TAIL, in_dim), 77.0, dtype=io, device=DEV)
    gp = torch.zeros_like(d["params"])
    _backward_into(kernel, d, io, gbuf, gp)
    _same_rows(gbuf[:S], d["grad_feats"].to(io), f"{tag} grad_feats")
    assert bool((gbuf[S:] == 77.0).all()), f"{tag}: rows behind the end of grad_feats were written"
    _same_params(gp, d["grad_params"], d, f"{tag} grad_params")


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_b2_enters_before_the_bf16_pack(kernel):
    """geometry features whose value BEFORE the bias (256 + odd) does not fit bf16 while the value after it does"""
    d = _case(KERNELS[kernel][0], 32, R.S_CANCEL, R.SHAPE_PATTERN, "paired", cancel=True)
    _check_forward(kernel, d, torch.bfloat16, f"{kernel} b2_cancel")
    _check_backward(kernel, d, torch.bfloat16, f"{kernel} b2_cancel")


def test_hidden_128_two_scratch_chunks():
    """S = 2^21 + 33: two chunks of the hidden-128 backward scratch, the second accumulating onto the partial rows of the
    first.  Upstream gradients on ~4000 samples that include the first and the last tile of each chunk; the forward is
    compared on all samples; the reference (with its exactness assertions) runs in float64 on the GPU."""
    d = _case(128, 32, R.S_TWO_CHUNKS, R.SHAPE_PATTERN, "paired", keep=False)
    live = (d["grad_density"] != 0).flatten() | (d["grad_rgb"] != 0).any(1)
    assert 3000 < int(live.sum()) < 6000
    for s0 in (0, R.CHUNK - 32, R.CHUNK, R.S_TWO_CHUNKS - 33):
        assert bool(live[s0:s0 + 32].any())
    P = R.unpack(d["grad_params"], 128, 32)
    assert all(float(P[n].abs().max()) > 0 for n in R.NAMES)
    _check_forward("h128_bf16", d, torch.bfloat16, "h128 two chunks")
    _check_backward("h128_bf16", d, torch.bfloat16, "h128 two chunks")
