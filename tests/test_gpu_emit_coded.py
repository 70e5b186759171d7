"""wisp_raymarch_ray_emit_coded: the emit launch of the 'ray' march that also writes the decoder's per-ray view code.

Every output it shares with wisp_raymarch_ray_emit must equal that entry point's bit for bit, and the code buffer must equal
wisp_nerf_mlp_dir_code on the same directions bit for bit, for EVERY ray - the ones without samples included (the decoder gathers
by ray index, but a later caller may not).  Nothing behind the end of the code buffer is written.  With an operand-image pointer
the workgroups behind the rays' build the decoder's operand image: byte for byte the stand-alone builder's; without it nothing
but the emit outputs and the code is written.
"""
import numpy as np
import pytest
import torch

from gpu_helpers import DEV, _C, cuda, make_rays, sparse_tree

pytestmark = pytest.mark.gpu

LEVEL, N = 3, 200
SENTINEL = 64                   # bf16 elements behind the code buffer that must survive


def _setup(R):
    C = _C()
    oc, pts, pyr, ex = sparse_tree(LEVEL, 40, 17)
    bits = C.spc_bitfield(cuda(pts[pyr[1, LEVEL]:pyr[1, LEVEL] + pyr[0, LEVEL]]), LEVEL)
    o, d = make_rays(R, 19, spread=1.2)
    if R > 1:                    # a ray that certainly misses: it looks away from the cube
        d[-1] = o[-1] / np.linalg.norm(o[-1])
    return C, bits, cuda(oc), cuda(ex), cuda(o), cuda(d)


@pytest.mark.parametrize("R", [1, 97, 257])
@pytest.mark.parametrize("with_jitter", [True, False])
def test_emit_coded_equals_emit_plus_dir_code(R, with_jitter):
    C, bits, oc, ex, o, d = _setup(R)
    jit = cuda(np.random.default_rng(23).uniform(size=(R, N)).astype(np.float32)) if with_jitter else None

    def count():
        return C.raymarch_ray_count(bits, oc, ex, o, d, 1.0, 5.0, N, LEVEL, jit, seed=11)

    want = C.raymarch_ray_finish(count(), with_dirs=True)
    got = C.raymarch_ray_finish(count(), with_dirs=True, with_code=True)
    assert len(got) == len(want) + 1
    lens = want[5][1:] - want[5][:-1]
    if R > 1:
        assert int((lens == 0).sum()) >= 1 and int((lens > 0).sum()) >= 1          # some rays miss, some hit
    for name, a, b in zip(("ridx", "samples", "depth", "deltas", "boundary", "offsets", "sample_dirs"), got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), name
    code = got[-1]
    assert code.dtype == torch.bfloat16 and tuple(code.shape) == (R, 32)
    ref = C.nerf_mlp_dir_code(d)
    assert torch.equal(code.view(torch.int16), ref.view(torch.int16).reshape(R, 32))      # bit patterns: every ray, hit or not
    # without the per-sample directions too
    lean = C.raymarch_ray_finish(count(), with_code=True)
    assert len(lean) == 7 and torch.equal(lean[0], want[0]) and torch.equal(lean[6].view(torch.int16), code.view(torch.int16))


def test_emit_coded_writes_nothing_behind_the_code_buffer():
    R = 97
    C, bits, oc, ex, o, d = _setup(R)
    st = C.raymarch_ray_count(bits, oc, ex, o, d, 1.0, 5.0, N, LEVEL, None, seed=5, read_total_async=False)
    S = int(st["offsets"][-1].item())
    assert S > 0
    pad = 16
    ridx = torch.full((S + pad,), -7, dtype=torch.int64, device=DEV)
    samples = torch.full((S + pad, 3), -7.0, device=DEV)
    depth = torch.full((S + pad,), -7.0, device=DEV)
    deltas = torch.full((S + pad,), -7.0, device=DEV)
    boundary = torch.full((S + pad,), 77, dtype=torch.uint8, device=DEV)
    code = torch.full((R * 32 + SENTINEL,), -3.0, dtype=torch.bfloat16, device=DEV)
    params = torch.randn(int(C.lib.wisp_nerf_mlp_param_count(32, 64, 4)), device=DEV)      # given, but with a NULL image: not looked at
    rc = C.lib.wisp_raymarch_ray_emit_coded(C._p(o), C._p(d), R, st["near32"], st["range32"], st["num_samples"], C._p(None), st["seed"],
                                            C._p(st["hitmask"]), C._p(st["offsets"]), C._p(ridx), C._p(samples), C._p(depth),
                                            C._p(deltas), C._p(boundary), C._p(None), 4, C._p(code), C._p(params), 32, 64, C._p(None), C._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((code[R * 32:] == -3.0).all())
    assert torch.equal(code[:R * 32].view(torch.int16), C.nerf_mlp_dir_code(d).view(torch.int16).reshape(-1))
    assert bool((ridx[S:] == -7).all()) and bool((samples[S:] == -7.0).all()) and bool((depth[S:] == -7.0).all())
    assert bool((deltas[S:] == -7.0).all()) and bool((boundary[S:] == 77).all())
    assert bool((ridx[:S] >= 0).all())
    # another view_freqs is refused, not silently encoded with 4
    rc = C.lib.wisp_raymarch_ray_emit_coded(C._p(o), C._p(d), R, st["near32"], st["range32"], st["num_samples"], C._p(None), st["seed"],
                                            C._p(st["hitmask"]), C._p(st["offsets"]), C._p(ridx), C._p(samples), C._p(depth),
                                            C._p(deltas), C._p(boundary), C._p(None), 6, C._p(code), C._p(None), 0, 0, C._p(None), C._stream())
    assert rc != 0


@pytest.mark.parametrize("R", [1, 97, 257])
@pytest.mark.parametrize("in_dim", [32, 5])
def test_trailing_workgroups_build_the_operand_image(R, in_dim):
    C, bits, oc, ex, o, d = _setup(R)
    torch.manual_seed(3)
    params = torch.randn(int(C.lib.wisp_nerf_mlp_param_count(in_dim, 64, 4)), device=DEV)
    want = C.raymarch_ray_finish(C.raymarch_ray_count(bits, oc, ex, o, d, 1.0, 5.0, N, LEVEL, None, seed=11))
    got = C.raymarch_ray_finish(C.raymarch_ray_count(bits, oc, ex, o, d, 1.0, 5.0, N, LEVEL, None, seed=11), image_of=(params, in_dim, 64))
    assert len(got) == 8
    for a, b in zip(got[:6], want):
        assert torch.equal(a, b)
    assert torch.equal(got[6].view(torch.int16), C.nerf_mlp_dir_code(d).view(torch.int16))
    assert torch.equal(got[7], C.nerf_mlp_operand_image(params, in_dim))
    # an image is refused for a shape the image kernels do not exist for
    with pytest.raises(RuntimeError):
        C.raymarch_ray_finish(C.raymarch_ray_count(bits, oc, ex, o, d, 1.0, 5.0, N, LEVEL, None, seed=11, read_total_async=False),
                              image_of=(params, in_dim, 128))
