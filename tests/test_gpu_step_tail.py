"""GPU (MI355X): the step's two closing sums as side workgroups of the hash-grid reduce launch (wisp_hashgrid_interpolate_bwd_adamw_tail,
csrc/step_tail_dev.h) - bit for bit the float32 restatements of tests/step_tail_ref.py applied to the partials read back, bit for bit
the entry points with launches of their own, and a whole native step with the fold on and off."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import hashgrid as ohash
from gpu_helpers import DEV, NGP_RES, _C, cuda, make_rays
import step_tail_ref as R

pytestmark = pytest.mark.gpu

BW = 19                                   # 16 levels in a 2^19-row table: the hashed levels have one owner per bucket (flush with AdamW), the
                                          # dense ones several (atomic flush), level 15 is dead (zero_from_col 30: the tail workgroups)
LR, B1, B2, EPS, WD = 1e-2, 0.9, 0.99, 1e-15, 1e-6


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)                                 # (compared on the device: some of these are whole table levels)
    assert a.shape == b.shape and torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


def _np_bits_equal(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float32).view(np.int32), np.asarray(want, dtype=np.float32).view(np.int32))


# ---------------------------------------------------------------------------------------------------- the carrying launch
def _grid_state(n, seed):
    rng = np.random.default_rng(seed)
    _, begin = ohash.table_layout(NGP_RES, 2 ** BW)
    rows = int(begin[-1])
    param = cuda(rng.normal(size=(rows, 2)).astype(np.float32) * 0.1)
    # Runs of 32 samples a few cells long at the finest level: every tile sends each bucket a fraction of its slot capacity.  (A slot
    # that overflows sends the surplus through float atomics into the gradient table, and so does a sample ON the boundary with its
    # out-of-range corner; where two of those meet in one element their order is free and the owned levels are no longer
    # reproducible from run to run - a handful of elements in a million with tests/gpu_helpers._ray_like_coords at this size.)
    start = rng.uniform(-0.9, 0.9, (n // 32, 1, 3))
    step = rng.normal(size=(n // 32, 1, 3)) * 3e-4
    coords = (start + step * np.arange(32)[None, :, None]).reshape(n, 3).astype(np.float32)
    return dict(n=n, rows=rows, coords=cuda(coords), g=cuda(rng.normal(size=(n, 32)).astype(np.float32) * 1e-3).bfloat16(),
                first=cuda(np.asarray(begin, dtype=np.int64)), param=param, m=torch.zeros_like(param), v=torch.zeros_like(param),
                shadow=param.bfloat16(), grad=torch.zeros_like(param))


def _grid_bwd(st, tail=None):
    """wisp_hashgrid_interpolate_bwd_adamw (tail None) or its _tail form on a copy of `st` -> (state after, covered rows, tail_done)"""
    C = _C()
    st = {k: (v.clone() if torch.is_tensor(v) and k in ("param", "m", "v", "shadow", "grad") else v) for k, v in st.items()}
    n = st["n"]
    _, _, res_ptr = C._host_res(NGP_RES)
    need = int(C.lib.wisp_hashgrid_bwd_workspace_bytes(n, 3, C.BF16, 2, res_ptr, 16, BW, None))
    ws = torch.empty(max(need, 0) + 256, dtype=torch.uint8, device=DEV)
    cov = (ctypes.c_int64 * 16)()
    args = [C._p(st["coords"]), n, 3, C._p(st["g"]), C.BF16, 2, C._p(st["first"]), res_ptr, 16, BW, 30, C._p(st["grad"]), C._p(ws),
            ws.numel(), None, C._p(st["param"]), C._p(st["m"]), C._p(st["v"]), C._p(st["shadow"]), LR, B1, B2, EPS, WD, 1, 1.0,
            ctypes.cast(cov, ctypes.c_void_p)]
    done = ctypes.c_int(-1)
    if tail is None:
        C._check(C.lib.wisp_hashgrid_interpolate_bwd_adamw(*args, C._stream()), "bwd_adamw")
    else:
        C._check(C.lib.wisp_hashgrid_interpolate_bwd_adamw_tail(*args, ctypes.byref(tail), ctypes.byref(done), C._stream()), "bwd_adamw_tail")
    torch.cuda.synchronize()
    return st, list(cov), done.value


_grid_cache = {}


def _grid(n):
    """the input state of the carrying launch and its result WITHOUT side jobs: computed once per size, never changed"""
    if n not in _grid_cache:
        st = _grid_state(n, 900 + n)
        _grid_cache[n] = (st,) + _grid_bwd(st)[:2]
    return _grid_cache[n]


def _check_grid_untouched(after, cov, n):
    """side jobs share nothing with the rest of the grid: the levels updated in the flush by one owner (covered rows) carry the same
    bits as without them; the levels flushed with float atomics (covered 0) are free in their add order and are not compared here"""
    st0, plain, cov0 = _grid(n)
    assert cov == cov0
    first = st0["first"].cpu().tolist()
    owned = 0
    for l, c in enumerate(cov):
        c = min(c, first[l + 1] - first[l])
        if c > 0:
            sl = slice(first[l], first[l] + c)
            for k in ("param", "m", "v", "shadow"):
                a, b = (t[k][sl].float() if k == "shadow" else t[k][sl] for t in (after, plain))
                _same_bits(a, b, f"level {l} {k}")
            owned += 1
    assert owned >= 3                                        # bucket-owned levels and the dead level of the tail workgroups


# ---------------------------------------------------------------------------------------------------- dW
def _decoder_case(S, in_dim, seed):
    C = _C()
    rng = np.random.default_rng(seed)
    rays = max(1, S // 24)
    d = rng.normal(size=(rays, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    nparam = int(C.lib.wisp_nerf_mlp_param_count(in_dim, 64, 4))
    case = dict(S=S, in_dim=in_dim, nparam=nparam,
                feats=cuda(rng.normal(size=(S, in_dim)).astype(np.float32)).bfloat16(),
                ridx=cuda(np.sort(rng.integers(0, rays, size=S)).astype(np.int64)),
                params=cuda((rng.normal(size=nparam) * 0.3).astype(np.float32)),
                g_rgb=cuda(rng.normal(size=(S, 3)).astype(np.float32) * 1e-2), g_density=cuda(rng.normal(size=(S, 1)).astype(np.float32) * 1e-2))
    case["code"] = C.nerf_mlp_dir_code(cuda(d))
    case["image"] = C.nerf_mlp_operand_image(case["params"], in_dim)
    need = int(C.lib.wisp_nerf_mlp_bwd_workspace_bytes(S, 64))
    case["ws_floats"] = need // 4 + 64
    return case


def _decoder_bwd(case, img, grad_params=None):
    """grad_params None: the _partials form -> (workspace, partial_rows); else the entry point that sums into grad_params itself"""
    C = _C()
    ws = torch.zeros(case["ws_floats"], dtype=torch.float32, device=DEV)
    g_feats = torch.empty_like(case["feats"])
    head = [C._p(case["feats"]), C.BF16, C._p(case["code"]), C._p(case["ridx"]), case["S"], case["in_dim"], 64, 4, C._p(case["params"])]
    if img:
        head.append(C._p(case["image"]))
    head += [C._p(case["g_rgb"]), C._p(case["g_density"]), C._p(g_feats)]
    rows = ctypes.c_int(-1)
    if grad_params is None:
        fn = C.lib.wisp_nerf_mlp_bwd_rays_img_partials if img else C.lib.wisp_nerf_mlp_bwd_rays_partials
        C._check(fn(*head, C._p(ws), ws.numel() * 4, ctypes.byref(rows), C._stream()), "bwd_rays_partials")
    else:
        fn = C.lib.wisp_nerf_mlp_bwd_rays_img if img else C.lib.wisp_nerf_mlp_bwd_rays
        C._check(fn(*head, C._p(grad_params), C._p(ws), ws.numel() * 4, C._stream()), "bwd_rays")
    torch.cuda.synchronize()
    return ws, rows.value, g_feats


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# partial rows = min(ceil(ceil(S / 32) / 4), CUs): 4096 samples (the smallest launch that bins) -> 32 rows; 128 -> 1; 2176 -> 17;
# 128 x CUs -> the CU count.  The decoder's sample count is independent of the carrying launch's (4096 throughout).
@pytest.mark.parametrize("in_dim", [32, 30])
@pytest.mark.parametrize("which", ["4096", "one_row", "17_rows", "cu_rows"])
def test_dw_side_job(which, in_dim):
    C = _C()
    S = {"4096": 4096, "one_row": 128, "17_rows": 2176, "cu_rows": 128 * _cus()}[which]
    want_rows = {"4096": 32, "one_row": 1, "17_rows": 17, "cu_rows": _cus()}[which]
    img = which != "17_rows"                                 # both chain kernels are covered
    case = _decoder_case(S, in_dim, 40 + in_dim + S)
    ws, rows, g_feats = _decoder_bwd(case, img)
    assert rows == want_rows
    partials = ws[:rows * R.NPARAM_PAD].cpu().numpy().reshape(rows, R.NPARAM_PAD)
    assert float(np.abs(partials[:, :R.NPARAM]).max()) > 0
    st0 = _grid(4096)[0]
    rng = np.random.default_rng(7)
    for prefill in (False, True):                            # the op is `+=`
        before = (rng.normal(size=case["nparam"]) if prefill else np.zeros(case["nparam"])).astype(np.float32)
        want = R.dw_reduce(partials, rows, in_dim, before)
        dec_grad = cuda(before.copy())
        tail = C.StepTail()
        tail.dw_partials, tail.dec_grad, tail.dw_rows, tail.in_dim = ws.data_ptr(), dec_grad.data_ptr(), rows, in_dim
        after, cov, done = _grid_bwd(st0, tail)
        assert done == 1
        assert _np_bits_equal(dec_grad.cpu().numpy(), want), f"side job vs restatement (prefill {prefill})"
        old = cuda(before.copy())
        _, _, g_feats_old = _decoder_bwd(case, img, grad_params=old)
        _same_bits(dec_grad, old, f"side job vs the launch of its own (prefill {prefill})")
        _same_bits(g_feats.float(), g_feats_old.float(), "grad_feats of the _partials form")
        alone = cuda(before.copy())
        C._check(C.lib.wisp_nerf_mlp_reduce_partials(C._p(ws), rows, in_dim, C._p(alone), C._stream()), "reduce_partials")
        _same_bits(dec_grad, alone, "side job vs wisp_nerf_mlp_reduce_partials")
        _check_grid_untouched(after, cov, 4096)


# ---------------------------------------------------------------------------------------------------- loss
def _loss_case(num_rays, seed, empty=False):
    rng = np.random.default_rng(seed)
    lens = np.zeros(num_rays, dtype=np.int64) if empty else rng.integers(0, 70, size=num_rays)
    if not empty and num_rays >= 4:
        lens[1] = 0; lens[2] = 150                            # an empty ray and one longer than two waves' registers
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S = int(off[-1])
    return dict(R=num_rays, S=S, off=cuda(off), gts=cuda(rng.uniform(size=(num_rays, 3)).astype(np.float32)),
                color=cuda(rng.uniform(size=(max(S, 1), 3)).astype(np.float32)), density=cuda(rng.uniform(0, 40, size=(max(S, 1), 1)).astype(np.float32)),
                deltas=cuda(rng.uniform(1e-3, 0.05, size=(max(S, 1), 1)).astype(np.float32)),
                ws_floats=2 * num_rays if num_rays > 4096 else 8192)          # the native step's sizing (train_step.hip)


def _composite(case, loss=None):
    """loss None: wisp_composite_loss_partials -> (workspace, count, inv_n); else wisp_composite_loss into `loss`"""
    C = _C()
    ws = torch.full((case["ws_floats"],), float("nan"), dtype=torch.float32, device=DEV)
    gc, gd = torch.empty(max(case["S"], 1), 3, device=DEV), torch.empty(max(case["S"], 1), 1, device=DEV)
    bg_arr, bg_ptr = C._host_f32([0.1, 0.2, 0.3])
    head = [C._p(case["color"]), C._p(case["density"]), C._p(case["deltas"]), C._p(case["off"]), case["R"], case["S"], bg_ptr, C._p(case["gts"]),
            0, C._p(gc), C._p(gd), None]
    cnt, inv_n = ctypes.c_int(-1), ctypes.c_float(0.0)
    if loss is None:
        C._check(C.lib.wisp_composite_loss_partials(*head, C._p(ws), ws.numel(), ctypes.byref(cnt), ctypes.byref(inv_n), C._stream()), "partials")
    else:
        C._check(C.lib.wisp_composite_loss(*head, C._p(loss), C._p(ws), ws.numel(), C._stream()), "composite_loss")
    torch.cuda.synchronize()
    return ws, cnt.value, inv_n.value, (gc, gd)


@pytest.mark.parametrize("which", ["1", "4", "4096", "4097", "all_empty"])
def test_loss_side_job(which):
    C = _C()
    num_rays = 300 if which == "all_empty" else int(which)
    case = _loss_case(num_rays, 60 + num_rays, empty=which == "all_empty")
    ws, cnt, inv_n, grads = _composite(case)
    assert cnt == num_rays and inv_n == float(np.float32(1.0) / np.float32(3 * num_rays))
    partials = ws[:cnt].cpu().numpy()
    assert np.all(np.isfinite(partials)) and float(np.abs(partials).sum()) > 0
    want = R.loss_sum(partials, inv_n)
    st0 = _grid(4096)[0]
    loss = torch.full((1,), float("nan"), device=DEV)
    tail = C.StepTail()
    tail.loss_partials, tail.loss, tail.loss_count, tail.inv_n, tail.in_dim = ws.data_ptr(), loss.data_ptr(), cnt, inv_n, 32
    after, cov, done = _grid_bwd(st0, tail)
    assert done == 1
    assert _np_bits_equal(loss.cpu().numpy(), [want]), (float(loss), float(want))
    old = torch.full((1,), float("nan"), device=DEV)
    _, _, _, grads_old = _composite(case, loss=old)
    _same_bits(loss, old, "side job vs wisp_composite_loss")
    if case["S"]:
        _same_bits(grads[0], grads_old[0], "grad_color of the _partials form")
        _same_bits(grads[1], grads_old[1], "grad_density of the _partials form")
    alone = torch.full((1,), float("nan"), device=DEV)
    C._check(C.lib.wisp_loss_sum(C._p(ws), cnt, inv_n, C._p(alone), C._stream()), "loss_sum")
    _same_bits(loss, alone, "side job vs wisp_loss_sum")
    _check_grid_untouched(after, cov, 4096)


# ---------------------------------------------------------------------------------------------------- fall-back
def test_no_binned_launch_is_reported_and_the_standalone_launches_give_the_same_bits():
    """1024 samples: launch_bwd takes the direct-atomics kernel, no reduce launch exists to carry the side jobs"""
    C = _C()
    case = _decoder_case(1024, 32, 71)
    ws, rows, _ = _decoder_bwd(case, True)
    lcase = _loss_case(33, 72)
    lws, cnt, inv_n, _ = _composite(lcase)
    before = np.random.default_rng(73).normal(size=case["nparam"]).astype(np.float32)
    dec_grad, loss = cuda(before.copy()), torch.full((1,), 5.0, device=DEV)
    tail = C.StepTail()
    tail.dw_partials, tail.dec_grad, tail.dw_rows, tail.in_dim = ws.data_ptr(), dec_grad.data_ptr(), rows, 32
    tail.loss_partials, tail.loss, tail.loss_count, tail.inv_n = lws.data_ptr(), loss.data_ptr(), cnt, inv_n
    st = _grid_state(1024, 74)
    after, cov, done = _grid_bwd(st, tail)
    assert done == 0
    assert _np_bits_equal(dec_grad.cpu().numpy(), before) and float(loss) == 5.0          # nothing was summed
    plain, cov0, _ = _grid_bwd(st)
    assert cov == cov0
    C._check(C.lib.wisp_nerf_mlp_reduce_partials(C._p(ws), rows, 32, C._p(dec_grad), C._stream()), "reduce_partials")
    C._check(C.lib.wisp_loss_sum(C._p(lws), cnt, inv_n, C._p(loss), C._stream()), "loss_sum")
    torch.cuda.synchronize()
    partials = ws[:rows * R.NPARAM_PAD].cpu().numpy()
    assert _np_bits_equal(dec_grad.cpu().numpy(), R.dw_reduce(partials, rows, 32, before))
    assert _np_bits_equal(loss.cpu().numpy(), [R.loss_sum(lws[:cnt].cpu().numpy(), inv_n)])


def test_both_side_jobs_in_one_launch():
    C = _C()
    case = _decoder_case(4096, 32, 81)
    ws, rows, _ = _decoder_bwd(case, True)
    lcase = _loss_case(517, 82)
    lws, cnt, inv_n, _ = _composite(lcase)
    dec_grad, loss = torch.zeros(case["nparam"], device=DEV), torch.zeros(1, device=DEV)
    tail = C.StepTail()
    tail.dw_partials, tail.dec_grad, tail.dw_rows, tail.in_dim = ws.data_ptr(), dec_grad.data_ptr(), rows, 32
    tail.loss_partials, tail.loss, tail.loss_count, tail.inv_n = lws.data_ptr(), loss.data_ptr(), cnt, inv_n
    st0 = _grid(4096)[0]
    after, cov, done = _grid_bwd(st0, tail)
    assert done == 1
    partials = ws[:rows * R.NPARAM_PAD].cpu().numpy()
    assert _np_bits_equal(dec_grad.cpu().numpy(), R.dw_reduce(partials, rows, 32, np.zeros(case["nparam"], dtype=np.float32)))
    assert _np_bits_equal(loss.cpu().numpy(), [R.loss_sum(lws[:cnt].cpu().numpy(), inv_n)])
    _check_grid_untouched(after, cov, 4096)


# ---------------------------------------------------------------------------------------------------- the whole step
def _trainer_pair():
    """two trainers over copies of one nerf_hash-shaped field: 16 levels up to 512^3 in a 2^19-row table, so that the fine levels have
    ONE owner per bucket (updated in the flush) and the coarse ones are flushed with float atomics by several workgroups"""
    from wisp.accelstructs import OctreeAS
    from wisp.models import Pipeline
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralRadianceField
    from wisp.tracers import PackedRFTracer
    from wisp.trainers import MultiviewTrainStep
    torch.manual_seed(0)
    P = np.random.default_rng(81).integers(0, 16, size=(1500, 3))
    blas = OctreeAS.from_quantized_points(torch.from_numpy(P).short().to(DEV), 4)
    grid = HashGrid.from_geometric(blas, feature_dim=2, num_lods=16, multiscale_type='cat', feature_std=0.2, codebook_bitwidth=19,
                                   min_grid_res=16, max_grid_res=512)
    nef = NeuralRadianceField(grid, view_embedder='positional', view_multires=4, hidden_dim=64, num_layers=1, bias=True,
                              prune_density_decay=0.95, prune_min_density=0.5).to(DEV)
    mk = lambda n: MultiviewTrainStep(Pipeline(n, PackedRFTracer(raymarch_type='ray', num_steps=2048, bg_color=(0, 0, 0))),
                                      prune_every=-1, enable_amp=True, target_sample_size=2 ** 17)
    return mk(nef), mk(copy.deepcopy(nef))


def test_whole_native_step_with_and_without_the_fold(monkeypatch):
    """One wisp_nerf_step_run from identical state with tail_fold 0 and 1.  Bit-equal: the loss, the decoder's parameters and both
    of its moments, the table levels updated in the flush by one owner.  The coarse levels (covered 0) are flushed with float
    atomics by several workgroups in a free order - two runs of the SAME code differ there - so for them the criterion is the one
    tests/test_gpu_1_selfcheck.py::test_native_step_equals_the_python_issued_step applies to two runs of this step: the first moment
    (0.1 x the gradient) to 1e-5 of its largest entry.  (tests/test_gpu_hashgrid_exact.py compares those levels bit for bit, which
    exact integer inputs allow and a real step's gradients do not.)"""
    from wisp.core import Rays
    from wisp.trainers import _native_step as NS
    tr_off, tr_on = _trainer_pair()
    assert tr_off._native is not None and tr_on._native is not None
    # 2048 candidates per ray: neighbouring samples share cells, the record slots of the owned levels stay far from overflowing (see
    # _grid_state) and those levels are reproducible
    o, d = make_rays(20, 95)
    gts = cuda(np.random.default_rng(96).uniform(size=(20, 3)).astype(np.float32))
    out = {}
    for name, tr, fold in (("off", tr_off, False), ("on", tr_on, True)):
        monkeypatch.setattr(NS, "TAIL_FOLD", fold)
        torch.manual_seed(77)                                 # the jitter seed follows torch's CPU generator
        loss, S = tr.step(Rays(cuda(o), cuda(d), dist_min=1.0, dist_max=5.0), gts)
        tr.wait_for_parameters()
        torch.cuda.synchronize()
        assert tr._native.steps == 1 and tr._native.fallbacks == 0
        out[name] = dict(loss=loss.clone(), S=S, cover=list(tr._native.covered_last), flat=tr.flat, d=tr._direct)
    a, b = out["off"], out["on"]
    print("samples", a["S"], "covered rows", a["cover"])
    assert a["S"] == b["S"] and 4096 <= a["S"] <= 16384, a["S"]
    assert a["cover"] == b["cover"]
    _same_bits(a["loss"], b["loss"], "loss")
    da, db = a["flat"].ranges["decoder"]
    for k in ("data", "exp_avg", "exp_avg_sq"):
        x, y = getattr(a["flat"], k)[da:db], getattr(b["flat"], k)[da:db]
        assert float(x.abs().max()) > 0
        _same_bits(x, y, f"decoder {k}")
    first = a["d"]._first_idx_host
    offs = [next(o_ for p, o_ in s["flat"]._grid_params if p is s["d"].table) for s in (a, b)]
    owned = atomic = 0
    for l, c in enumerate(a["cover"]):
        rows = first[l + 1] - first[l]
        lo = [off + 2 * first[l] for off in offs]
        if c >= rows > 0:
            for k in ("data", "exp_avg", "exp_avg_sq"):
                _same_bits(getattr(a["flat"], k)[lo[0]:lo[0] + 2 * rows], getattr(b["flat"], k)[lo[1]:lo[1] + 2 * rows], f"level {l} {k}")
            owned += 1
        elif c == 0:
            x, y = a["flat"].exp_avg[lo[0]:lo[0] + 2 * rows], b["flat"].exp_avg[lo[1]:lo[1] + 2 * rows]
            assert float((x - y).abs().max()) <= 1e-5 * float(x.abs().max()), f"level {l}"
            atomic += 1
    assert owned >= 2 and atomic >= 1, (owned, atomic, a["cover"])
