"""GPU: the fused training step of a triplanar SDF field (wisp_triplane_sdf_train_step, csrc/triplane_sdf_train.hip) against the
float64 reference of tests/triplane_sdf_step_ref.py - bit for bit on exactly representable inputs (atomics included: exact sums have
no order), against the modular path's own error on generic ones - its forward against wisp_triplane_sdf_query, its repeatability, its
scratch, and what is built on it: SDFTrainStep(fused_triplane=True) eager and graph-captured, and scripts/train_nglod.py --grid
triplanar --fused-kernel.  Every measured margin is appended to the file WISP_TRIPLANE_SDF_STEP_MARGINS names
(profiles/triplane_sdf_step_test_margins.jsonl)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import triplane_sdf_eval_ref as R
import triplane_sdf_step_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DECODER = ("w1", "b1", "w2", "b2")


def record(name, **values):
    path = os.environ.get("WISP_TRIPLANE_SDF_STEP_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, **{k: (float(v) if not isinstance(v, (int, str)) else v) for k, v in values.items()})) + "\n")


def dev_field(fld):
    """the kernels' field dict (kind 'triplane') from a reference field, no nef in between"""
    return dict(kind='triplane', planes=[p.to(DEV).contiguous() for p in fld["planes"]], multiscale=fld["multiscale"],
                w1=fld["w1"].to(DEV).contiguous(), b1=fld["b1"].to(DEV).contiguous(), w2=fld["w2"].to(DEV).contiguous(),
                b2=fld["b2"].to(DEV).contiguous())


def _fill(shape):
    n = int(np.prod(shape))
    v = ((torch.arange(n) % 7).float() - 3.0) / 2.0
    v[v == 0] = S.PREFILL_MAX
    return v.reshape(shape)


def prefill(fld):
    """gradient buffers holding non-zero multiples of 1/2 up to S.PREFILL_MAX (host copies): the step must ADD to them"""
    return dict(planes=[_fill(p.shape) for p in fld["planes"]], **{k: _fill(fld[k].shape) for k in DECODER})


def zeros(fld):
    return dict(planes=[torch.zeros(p.shape) for p in fld["planes"]], **{k: torch.zeros(fld[k].shape) for k in DECODER})


def run_step(dev, coords, gts, before):
    """one step on buffers holding `before` -> dict of host tensors: loss [1], the plane buffers and the four decoder buffers"""
    import wisp._C as C
    planes = [v.to(DEV).contiguous() for v in before["planes"]]
    bufs = {k: before[k].to(DEV).contiguous() for k in DECODER}
    loss = C.triplane_sdf_train_step(coords.to(DEV), gts.to(DEV).reshape(-1, 1), dev, planes, bufs["w1"], bufs["b1"], bufs["w2"], bufs["b2"])
    assert loss.shape == (1,) and loss.dtype == torch.float32
    return dict(loss=loss.cpu(), planes=[v.cpu() for v in planes], **{k: v.cpu() for k, v in bufs.items()})


_cache = {}

# (hidden, F, multiscale, sizes, b): the cases of test_triplane_sdf_step_host.py - hidden 1 / 17 / 128 / 256; 'sum' over 33 alone and
# over 5 + 9 + 17 + 33; 'cat' of 2 and 4 levels, one with K = 48 columns; a plane of size 1; planes of 4 x 129 x 129 = 66564 entries
# (above 2^16: f32 atomics), alone and beside a small plane on the fp64 accumulators
EXACT = [(1, 4, 'sum', (33,), 1), (17, 4, 'sum', (5, 9, 17, 33), 1), (128, 4, 'sum', (33,), 1), (256, 4, 'sum', (5, 9, 17, 33), 1),
         (128, 2, 'cat', (9, 33), 1), (17, 2, 'cat', (5, 9, 17, 33), 1), (256, 4, 'cat', (5, 9, 17, 33), 1), (128, 4, 'sum', (1, 9), 1),
         (128, 4, 'cat', (1, 17), 1), (128, 4, 'sum', (129,), 3), (17, 4, 'cat', (9, 129), 3)]


def exact(hidden, F, multiscale, sizes, b, n, all_miss=False):
    key = ("exact", hidden, F, multiscale, tuple(sizes), b, n, all_miss)
    if key not in _cache:
        case = S.exact_step_case(hidden, F, multiscale, sizes, n, seed=2, b=b, all_miss=all_miss)
        case["dev"] = dev_field(case["field"])
        case["before"] = prefill(case["field"])
        _cache[key] = case
    return _cache[key]


def assert_exact(got, want, before):
    assert torch.equal(got["loss"].double(), want["loss"]), (float(got["loss"]), float(want["loss"]))
    for k in DECODER:
        assert torch.equal(got[k].double(), before[k].double() + want[k].reshape(before[k].shape)), k
    for i, (g, w, b) in enumerate(zip(got["planes"], want["planes"], before["planes"])):
        assert torch.equal(g.double(), b.double() + w), f"plane {i}"


# ------------------------------------------------------------------------------------------------ 1. exact inputs
@pytest.mark.parametrize("n", [1, 16, 512])
@pytest.mark.parametrize("hidden,F,multiscale,sizes,b", EXACT)
def test_step_equals_float64_bit_for_bit_on_exact_inputs(hidden, F, multiscale, sizes, b, n):
    """loss and all gradients, on buffers pre-filled with non-zero values (the sums are ADDED); reflected points, points on the last
    texel line (a corner left out), points on a texel and shared texels are among the inputs (asserted by the generator)"""
    case = exact(hidden, F, multiscale, sizes, b, n)
    want, before = case["want"], case["before"]
    got = run_step(case["dev"], case["coords"], case["gts"], before)
    assert_exact(got, want, before)
    record("exact", hidden=hidden, F=F, multiscale=multiscale, sizes=str(sizes), n=n, bits_used=max(case["spans"].values()),
           plane_entries_moved=int(sum((w != 0).sum() for w in want["planes"])))


def test_all_miss_relu_moves_the_output_bias_alone():
    """every pre-activation negative: the loss and d b2 are written, every other buffer stays bitwise what it was"""
    case = exact(128, 4, 'sum', (33,), 1, 16, all_miss=True)
    want, before = case["want"], case["before"]
    got = run_step(case["dev"], case["coords"], case["gts"], before)
    assert_exact(got, want, before)
    for k in ("w1", "b1", "w2"):
        assert torch.equal(got[k], before[k]), k
    assert all(torch.equal(g, b) for g, b in zip(got["planes"], before["planes"])) and not torch.equal(got["b2"], before["b2"])


def test_a_second_call_adds_to_the_same_buffers():
    """two calls in a row on the same device buffers: twice the gradient on top of the pre-filled values, the loss written anew"""
    import wisp._C as C
    case = exact(128, 2, 'cat', (9, 33), 1, 16)
    want, before = case["want"], case["before"]
    planes = [v.to(DEV).contiguous() for v in before["planes"]]
    bufs = {k: before[k].to(DEV).contiguous() for k in DECODER}
    x, y = case["coords"].to(DEV), case["gts"].to(DEV).reshape(-1, 1)
    losses = [C.triplane_sdf_train_step(x, y, case["dev"], planes, bufs["w1"], bufs["b1"], bufs["w2"], bufs["b2"]).cpu() for _ in range(2)]
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0].double(), want["loss"])
    for k in DECODER:
        assert torch.equal(bufs[k].cpu().double(), before[k].double() + 2.0 * want[k].reshape(before[k].shape)), k
    for i, (g, w, b) in enumerate(zip(planes, want["planes"], before["planes"])):
        assert torch.equal(g.cpu().double(), b.double() + 2.0 * w), i


@pytest.mark.parametrize("hidden,F,multiscale,sizes,b", EXACT)
def test_forward_is_the_querys_value_bit_for_bit(hidden, F, multiscale, sizes, b):
    """one exact sample: d b2 = g = 2 (pred - gt), so pred = gt + g / 2 exactly - the value wisp_triplane_sdf_query returns"""
    import wisp._C as C
    case = exact(hidden, F, multiscale, sizes, b, 1)
    got = run_step(case["dev"], case["coords"], case["gts"], zeros(case["field"]))
    pred = case["gts"].double() + got["b2"].double() / 2.0
    query = C.sdf_query(case["coords"].to(DEV), case["dev"]).cpu()
    assert torch.equal(pred.float(), query.reshape(-1)) and torch.equal(pred, query.double().reshape(-1))
    assert float(got["b2"]) != 0.0


@pytest.mark.parametrize("n", [1, 17, 1000])
def test_forward_is_the_querys_value_on_generic_inputs(n):
    """generic field and points, gt = 0: the loss of a batch of one is fl(pred * pred) in fp32, bit for bit the square of the query's
    value; for a larger batch d b2 = sum 2 pred / n is compared with the same sum of the query's values in float64: every workgroup
    rounds the fp64 sum of its 16 terms to fp32 once and the reduce rounds the fp64 sum of those once more, 2^-24 of the partial sums
    plus 2^-24 of the total - at most 2^-23 sum|g|"""
    import wisp._C as C
    fld = R.generic_field((9, 17, 33), 128, F=4, multiscale='sum', seed=5)
    coords = R.generic_points(n, seed=4)
    dev = dev_field(fld)
    query = C.sdf_query(coords.to(DEV), dev).cpu().reshape(-1)
    if n == 1:
        got = run_step(dev, coords, torch.zeros(1), zeros(fld))
        assert torch.equal(got["loss"], (query * query)) and torch.equal(got["b2"], 2.0 * query)
        return
    got = run_step(dev, coords, torch.zeros(n), zeros(fld))
    g = ((2.0 * query) * float(np.float32(1.0) / np.float32(n))).double()           # (fp32: 2 pred is exact, one rounding for / n)
    assert n <= 16 * 1024                                                           # one pass per workgroup
    assert abs(float(got["b2"]) - float(g.sum())) <= 2.0 ** -23 * float(g.abs().sum())


# ------------------------------------------------------------------------------------------------ 2. generic inputs
# (sizes, hidden, F, multiscale): nglod_triplanar.yaml; 'cat' of three levels with odd hidden width; 'sum' of two levels at the widest
# decoder; one hidden unit; and 4 x 129 x 129 planes on the f32 atomic scatter
GENERIC = [((33,), 128, 4, 'sum'), ((9, 17, 33), 17, 2, 'cat'), ((17, 33), 256, 4, 'sum'), ((33,), 1, 4, 'sum'), ((129,), 128, 4, 'sum')]
# Bound of a generic output: twice the modular path's own largest error against float64 on that output (the standing rule of these
# steps, test_gpu_hash_sdf_step.py), with a floor where that error measures nothing.  The array outputs: one fp32 spacing at the
# output's largest magnitude, 2^-23 max|want| - an fp32 result lies up to half a spacing from the true value however it was summed.  The
# one-element outputs, loss and d b2: there the modular path's error is ONE number, a sum of signed errors that may cancel to anything.
# What does not cancel by luck is what the sum is made of: with e = the modular path's largest error of a PREDICTED DISTANCE against
# float64, d loss <= (2 / n) sum|pred - gt| e and d (d b2) <= 2 e to first order; the floor is twice that - the modular path's own
# error, propagated, times the same factor 2 - plus two fp32 spacings of the result (scalar_floor below).
FLOOR = 2.0 ** -23


def scalar_floor(k, want, gts, e_pred):
    n = gts.numel()
    diff = (want["pred"] - gts.double().reshape(-1)).abs()
    propagated = (2.0 / n) * float(diff.sum()) * e_pred if k == "loss" else 2.0 * e_pred
    return 2.0 * propagated + 2.0 * FLOOR * float(want[k].abs().max())


def nef_of(fld):
    """NeuralSDF over a TriplanarGrid (AABB) carrying a reference field's parameters (training mode); sizes 2^(base + l) + 1"""
    from wisp.accelstructs import AxisAlignedBBoxAS
    from wisp.models.grids import TriplanarGrid
    from wisp.models.nefs import NeuralSDF
    sizes = [int(p.shape[-1]) for p in fld["planes"][::3]]
    base = int(np.log2(sizes[0] - 1))
    assert sizes == [2 ** (base + l) + 1 for l in range(len(sizes))]
    grid = TriplanarGrid(AxisAlignedBBoxAS(), feature_dim=R.plane_features(fld), log_base_resolution=base, num_lods=len(sizes),
                         multiscale_type=fld["multiscale"], feature_std=0.01)
    nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=fld["w1"].shape[0], num_layers=1)
    with torch.no_grad():
        for l, vol in enumerate(grid.features):
            for name, p in zip(("fmx", "fmy", "fmz"), fld["planes"][3 * l:3 * l + 3]):
                getattr(vol, name).copy_(p[None])
        nef.decoder.layers[0].weight.copy_(fld["w1"]); nef.decoder.layers[0].bias.copy_(fld["b1"])
        nef.decoder.lout.weight.copy_(fld["w2"].reshape(1, -1)); nef.decoder.lout.bias.copy_(fld["b2"])
    return nef.to(DEV).train()


def nef_params(nef):
    dec = nef.decoder
    planes = [p for vol in nef.grid.features for p in (vol.fmx, vol.fmy, vol.fmz)]
    return dict(planes=planes, w1=dec.layers[0].weight, b1=dec.layers[0].bias, w2=dec.lout.weight, b2=dec.lout.bias)


def modular_step(nef, coords, gts):
    """the modular path: autograd over wisp_triplane_fwd / _bwd and the decoder, SDFTrainStep's loss"""
    nef.zero_grad(set_to_none=True)
    pred = nef(coords=coords, lod_idx=nef.grid.num_lods - 1, channels="sdf")
    loss = ((pred - gts) ** 2).sum() / coords.shape[0]
    loss.backward()
    prm = nef_params(nef)

    def grad(p):
        return (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu()
    return dict(loss=loss.detach().reshape(1).cpu(), pred=pred.detach().reshape(-1).cpu(), planes=[grad(p)[0] for p in prm["planes"]],
                **{k: grad(prm[k]) for k in DECODER})


def generic_setup(sizes, hidden, F, multiscale, n, seed=3):
    key = ("generic", sizes, hidden, F, multiscale, n, seed)
    if key not in _cache:
        fld = R.generic_field(sizes, hidden, F=F, multiscale=multiscale, seed=seed)
        coords = R.generic_points(n, seed=9)
        gts = R.sphere_sdf(coords)
        _cache[key] = (fld, coords, gts, S.step_reference(fld, coords, gts))
    return _cache[key]


def outputs(res):
    """(name, tensor) of every output of a step: loss, the four decoder gradients, every plane"""
    return [("loss", res["loss"])] + [(k, res[k]) for k in DECODER] + [(f"plane{i}", p) for i, p in enumerate(res["planes"])]


@pytest.mark.parametrize("n", [15, 17, 1000])
@pytest.mark.parametrize("sizes,hidden,F,multiscale", GENERIC)
def test_step_error_is_within_twice_the_modular_paths(sizes, hidden, F, multiscale, n):
    fld, coords, gts, want = generic_setup(sizes, hidden, F, multiscale, n)
    got = run_step(dev_field(fld), coords, gts, zeros(fld))
    mod = modular_step(nef_of(fld), coords.to(DEV), gts.to(DEV).reshape(-1, 1))
    failures = []
    e_pred = float((mod["pred"].double() - want["pred"]).abs().max())
    for (k, g), (_, m), (_, w) in zip(outputs(got), outputs(mod), outputs(want)):
        w = w.reshape(g.shape)
        e_fused, e_mod = float((g.double() - w).abs().max()), float((m.reshape(g.shape).double() - w).abs().max())
        floor = scalar_floor(k, want, gts, e_pred) if k in ("loss", "b2") else FLOOR * float(w.abs().max())
        bound = max(2.0 * e_mod, floor)
        record("generic", sizes=str(sizes), hidden=hidden, F=F, multiscale=multiscale, n=n, output=k, err_fused=e_fused, err_modular=e_mod,
               ratio=e_fused / e_mod if e_mod > 0 else -1.0, bound=bound, floor_decides=int(floor > 2.0 * e_mod), largest=float(w.abs().max()))
        print(f"{sizes} h{hidden} F{F} {multiscale} n{n} {k}: fused {e_fused:.3e} modular {e_mod:.3e} bound {bound:.3e}")
        if not e_fused <= bound:
            failures.append((k, e_fused, e_mod, bound))
    assert not failures, failures
    assert float(want["loss"]) > 0 and all(float(w.abs().max()) > 0 for w in want["planes"]) or hidden == 1


# ------------------------------------------------------------------------------------------------ 3. repeatability, scratch
def test_two_runs_are_bitwise_equal_where_the_sums_have_an_order_or_are_exact():
    fld, coords, gts, _ = generic_setup((33,), 128, 4, 'sum', 1000)
    dev = dev_field(fld)
    a, b = run_step(dev, coords, gts, zeros(fld)), run_step(dev, coords, gts, zeros(fld))
    for k in ("loss",) + DECODER:                                                   # fixed summation order
        assert torch.equal(a[k], b[k]), k
    apart = max(float((p - q).abs().max()) for p, q in zip(a["planes"], b["planes"]))
    scale = max(float(p.abs().max()) for p in a["planes"])
    record("repeat_generic_planes", max_difference=apart, largest=scale)
    assert apart <= 2.0 ** -23 * scale                                              # fp64 atomics in any order, one rounding to fp32
    for shape in ((256, 4, 'sum', (5, 9, 17, 33), 1), (17, 4, 'cat', (9, 129), 3)):  # exact sums have no order: both scatter regimes
        case = exact(*shape, 512)
        a, b = (run_step(case["dev"], case["coords"], case["gts"], case["before"]) for _ in range(2))
        for (k, p), (_, q) in zip(outputs(a), outputs(b)):
            assert torch.equal(p, q), k


@pytest.mark.parametrize("shape,n", [((128, 4, 'sum', (33,), 1), 512), ((17, 4, 'cat', (9, 129), 3), 16), ((256, 4, 'cat', (5, 9, 17, 33), 1), 16)])
def test_the_bytes_around_a_scratch_of_the_declared_size_stay_untouched(shape, n):
    """the entry point called directly with a scratch of exactly wisp_triplane_sdf_train_scratch_bytes inside a guarded buffer: the
    results are the exact ones, and the 4 KiB in front of and behind the scratch still hold their pattern"""
    import wisp._C as C
    case = exact(*shape, n)
    dev, before, want = case["dev"], case["before"], case["want"]
    args, keep = C._triplane_sdf_field_args(dev)
    need = int(C.lib.wisp_triplane_sdf_train_scratch_bytes(n, args[1], args[2], args[3], args[4], args[9]))
    assert need > 0
    guard = 4096
    buf = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    planes = [v.to(DEV).contiguous() for v in before["planes"]]
    bufs = {k: before[k].to(DEV).contiguous() for k in DECODER}
    garr, gptr = C._ptr_array(planes)
    x, y = case["coords"].to(DEV).contiguous(), case["gts"].to(DEV).contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    rc = C.lib.wisp_triplane_sdf_train_step(C._p(x), C._p(y), n, *args, gptr, C._p(bufs["w1"]), C._p(bufs["b1"]), C._p(bufs["w2"]),
                                            C._p(bufs["b2"]), C._p(loss), ctypes.c_void_p(buf.data_ptr() + guard), need, C._stream())
    assert rc == 0, C.lib.wisp_last_error()
    torch.cuda.synchronize()
    got = dict(loss=loss.cpu(), planes=[v.cpu() for v in planes], **{k: v.cpu() for k, v in bufs.items()})
    assert_exact(got, want, before)
    host = buf.cpu()
    assert bool((host[:guard] == 0xA5).all()) and bool((host[guard + need:] == 0xA5).all())
    assert bool((host[guard:guard + need] != 0xA5).any())
    record("scratch", shape=str(shape), n=n, scratch_bytes=need)


# ------------------------------------------------------------------------------------------------ 4. SDFTrainStep(fused_triplane=True)
TRI_FIELD = dict(sizes=(33,), hidden=128, F=4, multiscale='sum')                   # nglod_triplanar.yaml


def trainer_pair(monkeypatch, lr=1e-3, glw=1.0, seed=21):
    """two trainers from equal initial state: the fused triplanar step, and the same trainer kept on its modular launches"""
    from wisp.trainers import SDFTrainStep
    fld = R.generic_field(TRI_FIELD["sizes"], TRI_FIELD["hidden"], F=TRI_FIELD["F"], multiscale=TRI_FIELD["multiscale"], seed=seed)
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED", raising=False)
    fused = SDFTrainStep(nef_of(fld), lr=lr, grid_lr_weight=glw, fused_triplane=True)
    assert fused._fused_field() is not None and fused._fused_field()["triplane"]
    monkeypatch.setenv("WISP_SDF_TRAIN_FUSED", "0")
    modular = SDFTrainStep(nef_of(fld), lr=lr, grid_lr_weight=glw, fused_triplane=True)
    assert modular._fused_field() is None
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED")
    return fld, fused, modular


def batches(steps, n, seed):
    g = torch.Generator().manual_seed(seed)
    xs = torch.rand(steps, n, 3, generator=g) * 2 - 1
    return xs, torch.stack([R.sphere_sdf(x).reshape(-1, 1) for x in xs])


def flat(res):
    """the parameters / gradients of a result dict or nef_params dict as (name, host float64 tensor) pairs"""
    out = [(k, res[k].detach().cpu().double()) for k in DECODER]
    return out + [(f"plane{i}", p.detach().cpu().double().reshape(p.shape[-3:])) for i, p in enumerate(res["planes"])]


def test_trainer_one_step_agrees_with_the_modular_trainer(monkeypatch):
    """Adam's first step moves a parameter by lr * g / (|g| + eps).  Both trainers start from equal state.  With B the generic
    bound of a gradient tensor (twice the modular path's measured error against float64, at least one fp32 spacing at the largest
    entry), both paths' gradients lie within B of the float64 one, so where |g| > 4 B the two updates differ by at most
    lr * 2 B / (|g| - B), plus the fp32 rounding of the update itself (2^-22 of the larger of |p| and lr).  Entries with a smaller
    gradient get the bound that holds for any: there the sign of a rounding decides a full step, so the two lie within 2 lr."""
    lr = 1e-3
    fld, fused, modular = trainer_pair(monkeypatch, lr=lr)
    xs, ys = batches(1, 512, 5)
    want = S.step_reference(fld, xs[0], ys[0])
    mod = modular_step(nef_of(fld), xs[0].to(DEV), ys[0].to(DEV))
    lf = fused.step(xs[0].to(DEV), ys[0].to(DEV))
    lm = modular.step(xs[0].to(DEV), ys[0].to(DEV))
    e_pred = float((mod["pred"].double() - want["pred"]).abs().max())
    assert abs(float(lf) - float(lm)) <= 2.0 * scalar_floor("loss", want, ys[0], e_pred)
    for (k, pf), (_, pm), (_, g), (_, gm), (_, p0) in zip(flat(nef_params(fused.nef)), flat(nef_params(modular.nef)), flat(want), flat(mod),
                                                         flat(fld)):
        g, gm, p0 = g.reshape(pf.shape), gm.reshape(pf.shape), p0.reshape(pf.shape)
        B = max(2.0 * float((gm - g).abs().max()), FLOOR * float(g.abs().max()))
        big = g.abs() > 4.0 * B
        assert int(big.sum()) > 0.5 * int((g != 0).sum()) > 0, k
        allowed = lr * 2.0 * B / (g.abs() - B).clamp(min=B) + 2.0 ** -22 * p0.abs().clamp(min=lr)
        excess = ((pf - pm).abs() - allowed)[big]
        record("trainer_one_step", tensor=k, generic_bound=B, entries=int(big.sum()), max_parameter_difference=float((pf - pm).abs()[big].max()),
               largest_share_of_allowed=float(((pf - pm).abs() / allowed)[big].max()), lr=lr)
        assert float(excess.max()) <= 0.0, (k, float(excess.max()))
        # ... and no entry, whatever its gradient, is further apart than two full Adam steps in opposite directions
        assert float(((pf - pm).abs() - 2.0 * lr - 2.0 ** -22 * p0.abs().clamp(min=lr)).max()) <= 0.0, k
        assert float((pf - p0).abs()[big].min()) > 0.5 * lr                        # a full Adam step where there is a gradient


def test_thirty_steps_follow_adam_on_the_float64_gradients(monkeypatch):
    """loss curve over 30 steps against torch.optim.Adam on the float64-checked gradients (tests/triplane_sdf_step_ref.py, parameters
    kept in float64): the fused trainer's distance from that curve is allowed twice the modular trainer's own, both measured here
    and recorded - no pre-set constant"""
    lr, steps = 1e-3, 30
    fld, fused, modular = trainer_pair(monkeypatch, lr=lr)
    xs, ys = batches(steps, 512, 6)
    names = list(DECODER) + [f"plane{i}" for i in range(len(fld["planes"]))]
    params = [torch.nn.Parameter(fld[k].double().clone()) for k in DECODER] + [torch.nn.Parameter(p.double().clone()) for p in fld["planes"]]
    opt = torch.optim.Adam(params, lr=lr, eps=1e-15)
    curve, lf, lm = [], [], []
    for x, y in zip(xs, ys):
        # (the reference's forward reads f32 planes; their float64 master copies take the update)
        now = dict(multiscale=fld["multiscale"], planes=[p.detach().float() for p in params[4:]], **{k: p.detach() for k, p in zip(DECODER, params)})
        want = S.step_reference(now, x, y)
        curve.append(float(want["loss"]))
        for (k, g), p in zip(flat(want), params):
            p.grad = g.reshape(p.shape).clone()
        opt.step()
        lf.append(float(fused.step(x.to(DEV), y.to(DEV))))
        lm.append(float(modular.step(x.to(DEV), y.to(DEV))))
    curve, lf, lm = np.array(curve), np.array(lf), np.array(lm)
    d_fused, d_mod = float(np.abs(lf - curve).max()), float(np.abs(lm - curve).max())
    record("trainer_thirty_steps", fused_from_float64=d_fused, modular_from_float64=d_mod, first_loss=curve[0], last_loss=curve[-1])
    print(f"30 steps: fused {d_fused:.3e} modular {d_mod:.3e} loss {curve[0]:.4e} -> {curve[-1]:.4e}")
    assert len(names) == len(params) and curve[-1] < curve[0]
    assert d_fused <= 2.0 * d_mod, (d_fused, d_mod)


def texels_shared_by_more_than_two(fld, coords):
    """number of texels that receive more than two non-zero terms from this batch"""
    total = 0
    for plane, (w, off, _, _) in zip(fld["planes"], S.plane_lookups(fld, coords)):
        count = torch.zeros(int(plane.shape[-1]) ** 2)
        count.index_add_(0, off.reshape(-1), (w.reshape(-1) != 0).float())
        total += int((count > 2).sum())
    return total


def test_captured_graph_equals_the_eager_fused_step(monkeypatch):
    """5 steps of 24 coordinates (two workgroups, the second one half empty; no multiple of 16), graph replay against eager launches:
    the loss and the decoder's parameters bitwise - their sums have a fixed order.  The planes' fp64 atomics arrive in any order, so
    the batches are drawn (first seed that qualifies) such that no texel receives more than two terms: addition commutes, a sum of
    two terms on a zeroed accumulator has no order, and the planes - and with them the next step's forward - are bitwise equal too."""
    fld, eager, _ = trainer_pair(monkeypatch)
    _, graph, _ = trainer_pair(monkeypatch)
    seed = next(sd for sd in range(100, 600) if all(texels_shared_by_more_than_two(fld, x) == 0 for x in batches(5, 24, sd)[0]))
    xs, ys = batches(5, 24, seed)
    graph.capture(24)
    assert graph._fused_field() is not None and graph.static_inputs()[0].shape == (24, 3)
    for x, y in zip(xs, ys):
        le, lg = eager.step(x.to(DEV), y.to(DEV)), graph.step(x.to(DEV), y.to(DEV))
        assert torch.equal(le.reshape(-1).cpu(), lg.reshape(-1).cpu())
    for (k, pe), (_, pg), (_, p0) in zip(flat(nef_params(eager.nef)), flat(nef_params(graph.nef)), flat(fld)):
        assert torch.equal(pe, pg), k
        assert not torch.equal(pe, p0.reshape(pe.shape)), k
    record("graph_vs_eager", seed=seed, steps=5, n=24)


def test_captured_graph_at_512_coordinates_equals_eager_after_one_pass(monkeypatch):
    """forward + loss + backward once, eager launches against the replay of the captured graph, on 512 coordinates with contended
    texels: the loss and the decoder's gradients bitwise (fixed summation order); the plane gradients, whose atomics arrive in any
    order, each within the generic bound B of float64 (twice the modular path's measured error, at least one fp32 spacing of the
    largest entry) and therefore within 2 B of each other"""
    fld, eager, _ = trainer_pair(monkeypatch)
    _, graph, _ = trainer_pair(monkeypatch)
    xs, ys = batches(1, 512, 9)
    x, y = xs[0].to(DEV), ys[0].to(DEV)
    want = S.step_reference(fld, xs[0], ys[0])
    mod = modular_step(nef_of(fld), x, y)
    graph.capture(512)
    assert graph._fused_field() is not None
    eager.flat.grad.zero_(); graph.flat.grad.zero_()
    le = eager._forward_backward(x, y)
    gx, gy = graph.static_inputs()
    gx.copy_(x); gy.copy_(y)
    graph._graph.replay()
    assert torch.equal(le.reshape(-1).cpu(), graph._g_loss.reshape(-1).cpu())
    ge = {k: v for k, v in flat({k: ([q.grad for q in p] if k == "planes" else p.grad) for k, p in nef_params(eager.nef).items()})}
    gg = {k: v for k, v in flat({k: ([q.grad for q in p] if k == "planes" else p.grad) for k, p in nef_params(graph.nef).items()})}
    for k in DECODER:
        assert torch.equal(ge[k], gg[k]) and bool((ge[k] != 0).any()), k
    for (k, w), (_, m) in list(zip(flat(want), flat(mod)))[4:]:
        B = max(2.0 * float((m - w).abs().max()), FLOOR * float(w.abs().max()))
        apart = float((ge[k] - gg[k]).abs().max())
        record("graph_vs_eager_512", tensor=k, max_difference=apart, generic_bound=B, eager_from_float64=float((ge[k] - w).abs().max()),
               graph_from_float64=float((gg[k] - w).abs().max()))
        assert float((ge[k] - w).abs().max()) <= B and float((gg[k] - w).abs().max()) <= B, k
        assert apart <= 2.0 * B, k


def test_default_trainer_keeps_the_modular_launches(monkeypatch):
    from wisp.trainers import SDFTrainStep
    import wisp._C as C
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED", raising=False)
    fld = R.generic_field(TRI_FIELD["sizes"], 128, F=4, multiscale='sum', seed=21)
    step = SDFTrainStep(nef_of(fld), lr=1e-3)

    def never(*a, **k):
        raise AssertionError("the default trainer took the fused triplanar step")
    monkeypatch.setattr(C, "triplane_sdf_train_step", never)
    assert not step.fused_triplane and step._fused_field() is None
    xs, ys = batches(2, 512, 8)
    losses = [float(step.step(x.to(DEV), y.to(DEV))) for x, y in zip(xs, ys)]
    want = S.step_reference(fld, xs[0], ys[0])
    assert abs(losses[0] - float(want["loss"])) <= 1e-5 * float(want["loss"]) and all(np.isfinite(losses))


# ------------------------------------------------------------------------------------------------ 5. end to end
SCRIPT_ARGS = ["--grid", "triplanar", "--num-samples", "100000", "--epochs", "3", "--size", "32", "32", "--seed", "0"]


def test_train_nglod_script_trains_a_triplanar_grid_through_the_fused_kernel(tmp_path, capsys):
    """scripts/train_nglod.py --write-test-mesh DIR --grid triplanar --fused-kernel as a process of its own on the procedural torus,
    three epochs.  Its final IoU is compared with the modular trainer's on the same seed (the script's main() called here, three
    times): the modular path's float atomics make its own result vary from run to run, and the fused run may lie below the worst of
    the three by that measured spread (largest minus smallest).  The score is a ratio of sample counts, so three runs can only show
    a spread in whole samples - here they differ by one sample or by none - and a spread of none says the spread is below one
    sample, not that it is zero: the margin is therefore never taken smaller than what four samples move the score by.  One
    sample changing sides moves intersection / union by at most 1 / union (percent: 100 / union), and the union holds at least the
    samples that are inside the shape, counted here on a dataset built the way the script builds it."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train_nglod
    finally:
        sys.path.pop(0)
    script = os.path.join(ROOT, "scripts", "train_nglod.py")
    r = subprocess.run([sys.executable, script, "--write-test-mesh", str(tmp_path / "mesh"), "--fused-kernel", "--out-dir", str(tmp_path / "out")]
                       + SCRIPT_ARGS, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    losses = [float(line.split("l2 loss:")[1]) for line in r.stderr.splitlines() if "l2 loss:" in line]
    assert rec["grid"] == "triplanar" and rec["fused_triplane_step"] is True and rec["fused_step"] is False and rec["fused_hash_step"] is False
    assert rec["fused_triplane_eval"] is True and len(losses) == 3 and losses[-1] < losses[0]
    modular = []
    for i in range(3):
        m = train_nglod.main(["--write-test-mesh", str(tmp_path / f"mesh{i}"), "--out-dir", str(tmp_path / f"out{i}")] + SCRIPT_ARGS)
        assert m["fused_triplane_step"] is False and m["fused_step"] is False
        modular.append(m["iou_after"])
    capsys.readouterr()
    spread = max(modular) - min(modular)
    ds, _ = train_nglod.build(rec["obj"], DEV, num_samples=100000, grid_type="triplanar")
    inside = int((ds.data["sdf"] < 0).sum())
    assert len(ds) == rec["samples"] and inside > 1000
    four_samples = 4.0 * 100.0 / inside
    margin = max(spread, four_samples)
    record("script", iou_before=rec["iou_before"], iou_after_fused=rec["iou_after"], iou_after_modular_min=min(modular),
           iou_after_modular_max=max(modular), modular_spread=spread, samples_inside=inside, four_samples=four_samples, margin=margin,
           seconds=rec["seconds"], first_loss=losses[0], last_loss=losses[-1])
    print(f"IoU fused {rec['iou_after']:.4f} modular {modular} spread {spread:.4f} four samples {four_samples:.4f}")
    assert rec["iou_after"] > rec["iou_before"]
    assert rec["iou_after"] >= min(modular) - margin, (rec["iou_after"], modular, margin)
