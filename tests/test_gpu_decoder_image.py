"""The hidden-64 bf16 decoder kernels that copy their operands from a prebuilt image (wisp_nerf_mlp_build_operand_image,
wisp_nerf_mlp_fwd_rays_img / _bwd_rays_img) instead of staging and converting the fp32 parameters in every workgroup.

The image holds the bytes the old prologue leaves in LDS and the tile code is shared, so the image kernels must (1) equal the
float64 reference of tests/decoder_exact_ref.py exactly as tests/test_gpu_decoder_exact.py demands of the old kernels - density,
grad_feats and grad_params bit for bit, rgb within 1e-6 of sigmoid(z) in the `general` mode (derivation there) - and (2) equal
wisp_nerf_mlp_fwd_rays / _bwd_rays bit for bit on any input, exact or random: the arithmetic is identical, no tolerance.
Sample counts: none, one, both sides of the 32-sample tile, 300 (three backward workgroups), 4113 (a ragged last tile after
several rounds per wave).  Widths 32 (wide rows) and 5 (narrow rows).
"""
import pytest
import torch

import decoder_exact_ref as R
from gpu_helpers import DEV, _C

pytestmark = pytest.mark.gpu

IO = [torch.float32, torch.float16, torch.bfloat16]
SIZES = [0, 1, 31, 32, 33, 300, 4113]
PATTERNS = [0, 9]
NUM_RAYS = 97
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _cache.clear()


def _case(in_dim, S, pattern, mode):
    """inputs and the float64 reference on the GPU, computed once and never modified"""
    key = (in_dim, S, pattern, mode)
    if key not in _cache:
        c = R.make_case(64, in_dim, S, pattern, mode)
        d = dict(in_dim=in_dim, S=S, mode=mode, params=c["params"].to(DEV), feats=c["feats"].to(DEV), dirs=c["dirs"].to(DEV),
                 grad_rgb=c["grad_rgb"].to(DEV), grad_density=c["grad_density"].to(DEV))
        ref = R.reference(d["params"], d["feats"], d["dirs"], d["grad_rgb"], d["grad_density"], 64)
        d.update(density=ref["density"].float(), sigmoid_z=ref["rgb"], grad_feats=ref["grad_feats"], grad_params=ref["grad_params"].float())
        g = torch.Generator().manual_seed(S + 7 * pattern)
        d["ridx"] = torch.randint(0, NUM_RAYS, (S,), generator=g).to(DEV)
        d["code"] = _C().nerf_mlp_dir_code(torch.zeros(NUM_RAYS, 3, device=DEV))       # the exact cases look along direction 0
        _cache[key] = d
    return _cache[key]


def _run(d, io, image=None, params=None):
    C = _C()
    params = d["params"] if params is None else params
    ray_code = (d["ridx"], d["code"]) + (() if image is None else (image,))
    feats = d["feats"].to(io)
    rgb, den = C.nerf_mlp_forward(feats, None, params, d["in_dim"], 64, R.NF, True, ray_code=ray_code)
    gf, gp = C.nerf_mlp_backward(feats, None, params, d["grad_rgb"], d["grad_density"], d["in_dim"], 64, R.NF, True, ray_code=ray_code)
    return rgb, den, gf, gp


def _same(got, want, names="rgb density grad_feats grad_params".split()):
    for name, a, b in zip(names, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        if not torch.equal(a, b):
            bad = torch.nonzero(a != b)
            raise AssertionError(f"{name}: {bad.shape[0]} of {a.numel()} elements differ, first at {bad[0].tolist()}: "
                                 f"{float(a[tuple(bad[0])])} vs {float(b[tuple(bad[0])])}")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("io", IO, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("in_dim", [32, 5])
def test_image_kernels_equal_the_float64_reference_and_the_staging_kernels(in_dim, S, io, mode, pattern):
    d = _case(in_dim, S, pattern, mode)
    image = _C().nerf_mlp_operand_image(d["params"], in_dim)
    rgb, den, gf, gp = got = _run(d, io, image)
    assert rgb.dtype == torch.float32 and rgb.shape == (S, 3) and den.shape == (S, 1) and gf.dtype == io and gf.shape == (S, in_dim)
    _same((den, gf, gp), (d["density"], d["grad_feats"].to(io), d["grad_params"]), ["density", "grad_feats", "grad_params"])
    if mode == "paired":
        assert torch.equal(rgb, torch.full_like(rgb, 0.5))
    elif S:
        err = float((rgb.double() - d["sigmoid_z"]).abs().max())
        assert err <= 1e-6, err
    _same(got, _run(d, io))


@pytest.mark.parametrize("io", IO, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("in_dim", [32, 5])
def test_image_kernels_equal_the_staging_kernels_on_random_inputs(in_dim, io):
    C = _C()
    torch.manual_seed(1234 + in_dim)
    S = 4113
    n = int(C.lib.wisp_nerf_mlp_param_count(in_dim, 64, R.NF))
    params = (torch.randn(n) * 0.3).to(DEV)
    dirs = torch.nn.functional.normalize(torch.randn(NUM_RAYS, 3), dim=1).to(DEV)
    d = dict(in_dim=in_dim, S=S, params=params, feats=torch.randn(S, in_dim).to(DEV), grad_rgb=torch.randn(S, 3).to(DEV),
             grad_density=torch.randn(S, 1).to(DEV), ridx=torch.randint(0, NUM_RAYS, (S,)).to(DEV), code=C.nerf_mlp_dir_code(dirs))
    want = _run(d, io)
    assert all(bool(torch.isfinite(t.float()).all()) and float(t.float().abs().max()) > 0 for t in want)
    _same(_run(d, io, C.nerf_mlp_operand_image(params, in_dim)), want)
    # the image follows the parameters it is built from: other parameters, rebuilt image, other (and again identical) results
    params2 = params * 0.5 + 0.01
    got2 = _run(d, io, C.nerf_mlp_operand_image(params2, in_dim), params=params2)
    _same(got2, _run(d, io, params=params2))
    assert not torch.equal(got2[0], want[0]) and not torch.equal(got2[3], want[3])


@pytest.mark.parametrize("in_dim", [32, 5])
def test_builder_stays_inside_the_image(in_dim):
    C = _C()
    n = int(C.lib.wisp_nerf_mlp_operand_image_bytes(64))
    assert n > 0 and n % 16 == 0
    params = _case(in_dim, 33, 0, "general")["params"]
    buf = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    C._check(C.lib.wisp_nerf_mlp_build_operand_image(C._p(params), in_dim, 64, C._p(buf), C._stream()), "build_operand_image")
    torch.cuda.synchronize()
    assert bool((buf[n:] == 0xAB).all())
    assert torch.equal(buf[:n], C.nerf_mlp_operand_image(params, in_dim))
    assert bool((buf[:n] != 0xAB).any())


def test_other_shapes_are_refused():
    C = _C()
    assert int(C.lib.wisp_nerf_mlp_operand_image_bytes(128)) < 0
    params = _case(32, 33, 0, "general")["params"]
    with pytest.raises(RuntimeError):
        C.nerf_mlp_operand_image(params, 32, hidden=128)
    buf = torch.zeros(16, dtype=torch.uint8, device=DEV)
    assert C.lib.wisp_nerf_mlp_build_operand_image(C._p(params), 33, 64, C._p(buf), C._stream()) < 0
    d = _case(32, 33, 0, "general")
    image = C.nerf_mlp_operand_image(params, 32)
    rgb = torch.empty(33, 3, device=DEV); den = torch.empty(33, 1, device=DEV)
    rc = C.lib.wisp_nerf_mlp_fwd_rays_img(C._p(d["feats"]), C.F32, C._p(d["code"]), C._p(d["ridx"]), 33, 32, 128, R.NF, C._p(params),
                                          C._p(image), C._p(rgb), C._p(den), C._stream())
    assert rc == C.lib.wisp_nerf_mlp_fwd_rays(C._p(d["feats"]), C.F32, C._p(d["code"]), C._p(d["ridx"]), 33, 32, 128, R.NF, C._p(params),
                                              C._p(rgb), C._p(den), C._stream()) < 0
