"""GPU: the fused training step of a hash-grid SDF field (wisp_hash_sdf_train_step, csrc/hash_sdf_train.hip) against the float64
reference of tests/hash_sdf_step_ref.py - bit for bit on exactly representable inputs (float atomics included: exact sums have no
order), against the modular path's own error on generic ones - its forward against wisp_hash_sdf_query, its repeatability, and what
is built on it: SDFTrainStep(fused_hash=True) eager and graph-captured, and scripts/train_nglod.py --grid hash --fused-step.
Every measured margin is appended to profiles/hash_sdf_step_test_margins.jsonl when WISP_HASH_SDF_STEP_MARGINS names a file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hash_sdf_eval_ref as R
import hash_sdf_step_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GRADS = ("table", "w1", "b1", "w2", "b2")
OUTPUTS = ("loss",) + GRADS


def record(name, **values):
    path = os.environ.get("WISP_HASH_SDF_STEP_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, **{k: (float(v) if not isinstance(v, (int, str)) else v) for k, v in values.items()})) + "\n")


def dev_field(fld):
    """the kernels' field dict (kind 'hash') from a reference field, no nef in between"""
    return dict(kind='hash', codebook=fld["table"].to(DEV).contiguous(), begin_idxes=[int(b) for b in fld["begin"]],
                resolutions=list(fld["resolutions"]), feature_dim=int(fld["table"].shape[1]), codebook_bitwidth=fld["bitwidth"],
                multiscale=fld["multiscale"], zero_from_col=R.zero_from_col(fld), w1=fld["w1"].to(DEV).contiguous(),
                b1=fld["b1"].to(DEV).contiguous(), w2=fld["w2"].to(DEV).contiguous(), b2=fld["b2"].to(DEV).contiguous())


def prefill(fld):
    """gradient buffers holding non-zero multiples of 1/2 up to S.PREFILL_MAX (host copies): the step must ADD to them"""
    out = {}
    for k in GRADS:
        n = fld[k].numel()
        v = ((torch.arange(n) % 7).float() - 3.0) / 2.0
        v[v == 0] = S.PREFILL_MAX
        out[k] = v.reshape(fld[k].shape)
    return out


def run_step(dev, coords, gts, before):
    """one launch pair on buffers holding `before` -> dict of host tensors: loss [1] and the five buffers afterwards"""
    import wisp._C as C
    bufs = {k: v.to(DEV).contiguous() for k, v in before.items()}
    loss = C.hash_sdf_train_step(coords.to(DEV), gts.to(DEV).reshape(-1, 1), dev, bufs["table"], bufs["w1"], bufs["b1"], bufs["w2"],
                                 bufs["b2"])
    assert loss.shape == (1,) and loss.dtype == torch.float32
    return dict(loss=loss.cpu(), **{k: v.cpu() for k, v in bufs.items()})


_cache = {}

# (hidden, F, multiscale, lod_idx, resolutions, bitwidth): hidden 1 / 17 / 128 / 256, F 2 / 4 / 8, 'cat' and 'sum', the last LOD, a
# middle one and 'cat' at LOD 0, tables of 2^6 .. 2^10 rows, one dense + one hashed level (the cases of test_hash_sdf_step_host.py)
EXACT = [(1, 8, 'cat', 3, R.EXACT_RES, 8), (17, 4, 'cat', 2, R.EXACT_RES, 10), (128, 2, 'cat', 0, R.EXACT_RES, 10),
         (256, 8, 'sum', 3, R.EXACT_RES, 7), (128, 4, 'sum', 1, (4, 16), 8), (256, 8, 'cat', 3, R.EXACT_RES, 6),
         (17, 2, 'cat', 1, (4, 16), 8),
         # a level of more than 2^16 entries keeps the f32 atomic scatter, beside small levels on the fp64 accumulators in one launch:
         # hashed (2^14 rows x 8) behind three small dense ones; hashed in the middle of a 'cat' whose last level is not gathered;
         # dense (32^3 rows x 8) at 2^16
         (128, 8, 'sum', 3, R.EXACT_RES, 14), (17, 8, 'cat', 2, (4, 32, 16), 14), (256, 8, 'sum', 3, R.EXACT_RES, 16)]


def exact(hidden, F, multiscale, lod_idx, res, bitwidth, n):
    key = ("exact", hidden, F, multiscale, lod_idx, tuple(res), bitwidth, n)
    if key not in _cache:
        case = S.exact_step_case(hidden, F, multiscale, lod_idx, n, res, bitwidth, seed=2)
        case["dev"] = dev_field(case["field"])
        case["before"] = prefill(case["field"])
        _cache[key] = case
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. exact inputs
@pytest.mark.parametrize("n", [1, 16, 512])
@pytest.mark.parametrize("hidden,F,multiscale,lod_idx,res,bitwidth", EXACT)
def test_step_equals_float64_bit_for_bit_on_exact_inputs(hidden, F, multiscale, lod_idx, res, bitwidth, n):
    """loss and all five gradients, on buffers pre-filled with non-zero values (the sums are ADDED); points outside the cube and on
    cell faces are among the inputs; the rows of the levels that are not gathered stay bitwise what they were"""
    case = exact(hidden, F, multiscale, lod_idx, res, bitwidth, n)
    fld, want, before = case["field"], case["want"], case["before"]
    got = run_step(case["dev"], case["coords"], case["gts"], before)
    assert torch.equal(got["loss"].double(), want["loss"]), (float(got["loss"]), float(want["loss"]))
    for k in GRADS:
        assert torch.equal(got[k].double(), before[k].double() + want[k].reshape(before[k].shape)), k
    if multiscale == 'cat':
        first_dead = int(fld["begin"][lod_idx])
        assert torch.equal(got["table"][first_dead:], before["table"][first_dead:])
        if lod_idx == 0:                                                            # the decoder sees the position alone
            assert torch.equal(got["table"], before["table"]) and torch.equal(got["w1"][:, 3:], before["w1"][:, 3:])
            assert not torch.equal(got["w1"][:, :3], before["w1"][:, :3])
    record("exact", hidden=hidden, F=F, multiscale=multiscale, lod_idx=lod_idx, bitwidth=bitwidth, n=n,
           bits_used=max(case["spans"].values()), table_entries_moved=int((want["table"] != 0).sum()))


@pytest.mark.parametrize("hidden,F,multiscale,lod_idx,res,bitwidth", EXACT)
def test_forward_is_the_querys_value_bit_for_bit(hidden, F, multiscale, lod_idx, res, bitwidth):
    """one exact sample: d b2 = g = 2 (pred - gt), so pred = gt + g / 2 exactly - the value wisp_hash_sdf_query returns"""
    import wisp._C as C
    case = exact(hidden, F, multiscale, lod_idx, res, bitwidth, 1)
    zero = {k: torch.zeros_like(v) for k, v in case["before"].items()}
    got = run_step(case["dev"], case["coords"], case["gts"], zero)
    pred = case["gts"].double() + got["b2"].double() / 2.0
    query = C.sdf_query(case["coords"].to(DEV), case["dev"]).cpu()
    assert torch.equal(pred.float(), query.reshape(-1)) and torch.equal(pred, query.double().reshape(-1))
    assert float(got["b2"]) != 0.0


# ------------------------------------------------------------------------------------------------ 2. generic inputs
# (resolution list, hidden, F, multiscale, lod_idx, codebook bitwidth).  At 2^12 rows every level has at most 2^16 entries and takes
# the fp64 accumulators; the last two fields mix them with levels on the f32 atomic scatter in one launch: resolutions 80 and 406
# hashed into 2^14 rows x 8, and the dense 40^3 rows x 2 at 2^16
GENERIC = [(0, 128, 8, 'cat', 3, 12), (1, 128, 8, 'cat', 3, 12), (0, 17, 4, 'cat', 2, 12), (1, 256, 8, 'sum', 3, 12),
           (0, 128, 2, 'sum', 1, 12), (1, 1, 8, 'cat', 0, 12), (1, 128, 8, 'cat', 3, 14), (0, 128, 2, 'sum', 3, 16)]
# Bound of a generic output: twice the modular path's own largest error against float64 on that output (the form of
# test_gpu_hash_sdf_eval.py's generic query cases), with a floor where that error measures nothing.  The array outputs: one fp32
# spacing at the output's largest magnitude, 2^-23 max|want| - an fp32 result lies up to half a spacing from the true value however it
# was summed.  The one-element outputs, loss and d b2: there the modular path's error is ONE number, a sum of signed errors that may
# cancel to anything.  What does not cancel by luck is what the sum is made of: with e = the modular path's largest error of a
# PREDICTED DISTANCE against float64, d loss <= (2 / n) sum|pred - gt| e and d (d b2) <= 2 e to first order; the floor is twice that
# - the modular path's own error, propagated, times the same factor 2 - plus two fp32 spacings of the result (scalar_floor below).
FLOOR = 2.0 ** -23


def scalar_floor(k, want, gts, e_pred):
    n = gts.numel()
    diff = (want["pred"] - gts.double().reshape(-1)).abs()
    propagated = (2.0 / n) * float(diff.sum()) * e_pred if k == "loss" else 2.0 * e_pred
    return 2.0 * propagated + 2.0 * FLOOR * float(want[k].abs().max())


def nef_of(fld):
    """NeuralSDF over a HashGrid carrying a reference field's parameters (training mode, gradients on)"""
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import NeuralSDF
    F = int(fld["table"].shape[1])
    grid = HashGrid.from_resolutions(None, feature_dim=F, resolutions=list(fld["resolutions"]), multiscale_type=fld["multiscale"],
                                     feature_std=0.01, codebook_bitwidth=fld["bitwidth"])
    nef = NeuralSDF(grid, pos_embedder='none', position_input=True, hidden_dim=fld["w1"].shape[0], num_layers=1)
    with torch.no_grad():
        assert grid.codebook.feats.shape == fld["table"].shape
        grid.codebook.feats.data = fld["table"].clone()
        nef.decoder.layers[0].weight.copy_(fld["w1"]); nef.decoder.layers[0].bias.copy_(fld["b1"])
        nef.decoder.lout.weight.copy_(fld["w2"].reshape(1, -1)); nef.decoder.lout.bias.copy_(fld["b2"])
    return nef.to(DEV).train()


def nef_params(nef):
    dec = nef.decoder
    return dict(table=nef.grid.codebook.feats, w1=dec.layers[0].weight, b1=dec.layers[0].bias, w2=dec.lout.weight, b2=dec.lout.bias)


def modular_step(nef, lod_idx, coords, gts):
    """the modular path: autograd over wisp.ops.grid.hashgrid and the decoder, SDFTrainStep's loss"""
    nef.zero_grad(set_to_none=True)
    pred = nef(coords=coords, lod_idx=lod_idx, channels="sdf")
    loss = ((pred - gts) ** 2).sum() / coords.shape[0]
    loss.backward()
    prm = nef_params(nef)
    return dict(loss=loss.detach().reshape(1).cpu(), pred=pred.detach().reshape(-1).cpu(),
                **{k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().reshape(p.shape) for k, p in prm.items()})


def generic_setup(res, hidden, F, multiscale, lod_idx, n, bitwidth=12):
    key = ("generic", res, hidden, F, multiscale, lod_idx, n, bitwidth)
    if key not in _cache:
        fld = R.generic_field(R.GENERIC_RES[res], hidden, F=F, multiscale=multiscale, lod_idx=lod_idx, seed=3 + res, bitwidth=bitwidth)
        coords = R.generic_points(n, seed=9)
        gts = R.sphere_sdf(coords)
        _cache[key] = (fld, coords, gts, S.step_reference(fld, coords, gts))
    return _cache[key]


@pytest.mark.parametrize("n", [15, 17, 1000])
@pytest.mark.parametrize("res,hidden,F,multiscale,lod_idx,bitwidth", GENERIC)
def test_step_error_is_within_twice_the_modular_paths(res, hidden, F, multiscale, lod_idx, bitwidth, n):
    fld, coords, gts, want = generic_setup(res, hidden, F, multiscale, lod_idx, n, bitwidth)
    entries = [int(fld["begin"][l + 1] - fld["begin"][l]) * F for l, _ in S.live_levels(fld)]
    assert (bitwidth > 12) == any(e > 2 ** 16 for e in entries) and (lod_idx == 0 or any(e <= 2 ** 16 for e in entries))
    zero = {k: torch.zeros(fld[k].shape) for k in GRADS}
    got = run_step(dev_field(fld), coords, gts, zero)
    mod = modular_step(nef_of(fld), lod_idx, coords.to(DEV), gts.to(DEV).reshape(-1, 1))
    failures = []
    e_pred = float((mod["pred"].double() - want["pred"]).abs().max())
    for k in OUTPUTS:
        w = want[k].reshape(got[k].shape)
        e_fused, e_mod = float((got[k].double() - w).abs().max()), float((mod[k].reshape(got[k].shape).double() - w).abs().max())
        bound = max(2.0 * e_mod, scalar_floor(k, want, gts, e_pred) if k in ("loss", "b2") else FLOOR * float(w.abs().max()))
        record("generic", res=str(R.GENERIC_RES[res]), hidden=hidden, F=F, multiscale=multiscale, lod_idx=lod_idx, bitwidth=bitwidth, n=n, output=k,
               err_fused=e_fused, err_modular=e_mod, bound=bound, largest=float(w.abs().max()))
        print(f"{R.GENERIC_RES[res]} h{hidden} F{F} {multiscale} lod{lod_idx} n{n} {k}: fused {e_fused:.3e} modular {e_mod:.3e} bound {bound:.3e}")
        if not e_fused <= bound:
            failures.append((k, e_fused, e_mod, bound))
    assert not failures, failures
    if multiscale == 'cat':
        assert bool((got["table"][int(fld["begin"][lod_idx]):] == 0).all())
    assert float(want["loss"]) > 0 and (lod_idx == 0 or float(want["table"].abs().max()) > 0)


# ------------------------------------------------------------------------------------------------ 3. repeatability
def test_two_runs_are_bitwise_equal_where_the_sums_have_an_order_or_are_exact():
    fld, coords, gts, _ = generic_setup(1, 128, 8, 'cat', 3, 1000)
    zero = {k: torch.zeros(fld[k].shape) for k in GRADS}
    dev = dev_field(fld)
    a, b = run_step(dev, coords, gts, zero), run_step(dev, coords, gts, zero)
    for k in ("loss", "w1", "b1", "w2", "b2"):                                     # fixed summation order
        assert torch.equal(a[k], b[k]), k
    scale = float(a["table"].abs().max())
    record("repeat_generic_table", max_difference=float((a["table"] - b["table"]).abs().max()), largest=scale)
    assert float((a["table"] - b["table"]).abs().max()) <= 1e-5 * scale             # float atomics: arrival order
    case = exact(256, 8, 'sum', 3, R.EXACT_RES, 7, 512)
    a, b = (run_step(case["dev"], case["coords"], case["gts"], case["before"]) for _ in range(2))
    for k in OUTPUTS:                                                               # exact sums have no order
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 4. SDFTrainStep(fused_hash=True)
HASH_FIELD = dict(resolutions=R.GENERIC_RES[1], hidden=128, F=8, multiscale='cat')     # nglod_hash.yaml with tables of 2^12 rows


def trainer_pair(monkeypatch, lr=1e-3, glw=1.0, seed=21, bitwidth=12):
    """two trainers from equal initial state: the fused hash step, and the same trainer kept on its modular launches.  At 2^14 rows
    the levels of resolution 80 and 406 (131072 entries) take the f32 atomic scatter, the level of resolution 16 the fp64 one."""
    from wisp.trainers import SDFTrainStep
    fld = R.generic_field(HASH_FIELD["resolutions"], HASH_FIELD["hidden"], F=HASH_FIELD["F"], multiscale=HASH_FIELD["multiscale"],
                          seed=seed, bitwidth=bitwidth)
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED", raising=False)
    fused = SDFTrainStep(nef_of(fld), lr=lr, grid_lr_weight=glw, fused_hash=True)
    assert fused._fused_field() is not None and fused._fused_field()["hash"]
    monkeypatch.setenv("WISP_SDF_TRAIN_FUSED", "0")
    modular = SDFTrainStep(nef_of(fld), lr=lr, grid_lr_weight=glw, fused_hash=True)
    assert modular._fused_field() is None
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED")
    return fld, fused, modular


def batches(steps, n, seed):
    g = torch.Generator().manual_seed(seed)
    xs = torch.rand(steps, n, 3, generator=g) * 2 - 1
    return xs, torch.stack([R.sphere_sdf(x).reshape(-1, 1) for x in xs])


@pytest.mark.parametrize("bitwidth", [12, 14])
def test_trainer_one_step_agrees_with_the_modular_trainer(monkeypatch, bitwidth):
    """Adam's first step moves a parameter by lr * g / (|g| + eps).  Both trainers start from equal state.  With B the generic
    bound of a gradient tensor (twice the modular path's measured error against float64, at least one fp32 spacing at the largest
    entry), both paths' gradients lie within B of the float64 one, so where |g| > 4 B the two updates differ by at most
    lr * 2 B / (|g| - B), plus the fp32 rounding of the update itself (2^-22 of the larger of |p| and lr).  Entries with a smaller
    gradient get the bound that holds for any: there the sign of a rounding decides a full step, so the two lie within 2 lr."""
    lr = 1e-3
    fld, fused, modular = trainer_pair(monkeypatch, lr=lr, bitwidth=bitwidth)
    xs, ys = batches(1, 512, 5)
    want = S.step_reference(fld, xs[0], ys[0])
    mod = modular_step(nef_of(fld), 3, xs[0].to(DEV), ys[0].to(DEV))
    lf = fused.step(xs[0].to(DEV), ys[0].to(DEV))
    lm = modular.step(xs[0].to(DEV), ys[0].to(DEV))
    e_pred = float((mod["pred"].double() - want["pred"]).abs().max())
    assert abs(float(lf) - float(lm)) <= 2.0 * scalar_floor("loss", want, ys[0], e_pred)
    for k in GRADS:
        pf, pm = nef_params(fused.nef)[k].detach().cpu().double(), nef_params(modular.nef)[k].detach().cpu().double()
        g = want[k].reshape(pf.shape)
        p0 = fld[k].reshape(pf.shape).double()
        B = max(2.0 * float((mod[k].reshape(pf.shape).double() - g).abs().max()), FLOOR * float(g.abs().max()))
        big = g.abs() > 4.0 * B
        assert int(big.sum()) > 0.5 * int((g != 0).sum()) > 0, k
        allowed = lr * 2.0 * B / (g.abs() - B).clamp(min=B) + 2.0 ** -22 * p0.abs().clamp(min=lr)
        excess = ((pf - pm).abs() - allowed)[big]
        record("trainer_one_step", bitwidth=bitwidth, tensor=k, generic_bound=B, entries=int(big.sum()), max_parameter_difference=float((pf - pm).abs()[big].max()),
               largest_share_of_allowed=float(((pf - pm).abs() / allowed)[big].max()), lr=lr)
        assert float(excess.max()) <= 0.0, (k, float(excess.max()))
        # ... and no entry, whatever its gradient, is further apart than two full Adam steps in opposite directions
        assert float(((pf - pm).abs() - 2.0 * lr - 2.0 ** -22 * p0.abs().clamp(min=lr)).max()) <= 0.0, k
        assert float((pf - p0).abs()[big].min()) > 0.5 * lr                        # a full Adam step where there is a gradient
    dead = int(fld["begin"][3])
    assert torch.equal(nef_params(fused.nef)["table"].detach().cpu()[dead:], fld["table"][dead:])      # the finest level: no gradient


def test_thirty_steps_follow_adam_on_the_float64_gradients(monkeypatch):
    """loss curve over 30 steps against torch.optim.Adam on the float64-checked gradients (tests/hash_sdf_step_ref.py, parameters
    kept in float64): the fused trainer's distance from that curve is allowed twice the modular trainer's own, both recorded"""
    lr, steps = 1e-3, 30
    fld, fused, modular = trainer_pair(monkeypatch, lr=lr)
    xs, ys = batches(steps, 512, 6)
    ref = {k: fld[k].double().clone() for k in GRADS}
    params = [torch.nn.Parameter(ref[k]) for k in GRADS]
    opt = torch.optim.Adam(params, lr=lr, eps=1e-15)
    curve, lf, lm = [], [], []
    for x, y in zip(xs, ys):
        now = dict(fld, **{k: p.detach().float() if k == "table" else p.detach() for k, p in zip(GRADS, params)})
        # (the reference's forward reads an f32 table; its float64 master copy takes the update)
        want = S.step_reference(now, x, y)
        curve.append(float(want["loss"]))
        for k, p in zip(GRADS, params):
            p.grad = want[k].reshape(p.shape).clone()
        opt.step()
        lf.append(float(fused.step(x.to(DEV), y.to(DEV))))
        lm.append(float(modular.step(x.to(DEV), y.to(DEV))))
    curve, lf, lm = np.array(curve), np.array(lf), np.array(lm)
    d_fused, d_mod = float(np.abs(lf - curve).max()), float(np.abs(lm - curve).max())
    record("trainer_thirty_steps", fused_from_float64=d_fused, modular_from_float64=d_mod, first_loss=curve[0], last_loss=curve[-1])
    print(f"30 steps: fused {d_fused:.3e} modular {d_mod:.3e} loss {curve[0]:.4e} -> {curve[-1]:.4e}")
    assert curve[-1] < curve[0]
    assert d_fused <= 2.0 * d_mod, (d_fused, d_mod)


def rows_shared_by_more_than_two(fld, coords):
    """number of table rows of the gathered levels that receive more than two non-zero terms from this batch"""
    count = torch.zeros(fld["table"].shape[0])
    corners = S.level_corners(fld, coords)
    for l, _ in S.live_levels(fld):
        w, rows = corners[l]
        count.index_add_(0, rows.reshape(-1), (w.reshape(-1) != 0).float())
    return int((count > 2).sum())


def test_captured_graph_equals_the_eager_fused_step(monkeypatch):
    """5 steps of 24 coordinates (two workgroups, the second one half empty), graph replay against eager launches: the loss and the
    decoder's parameters bitwise - their sums have a fixed order.  The table's float atomics arrive in any order, so the batches
    are drawn (first seed that qualifies) such that no table row receives more than two terms: fp32 addition commutes, a sum of two
    terms on a zeroed gradient has no order, and the table - and with it the next step's forward - is bitwise equal as well."""
    fld, eager, _ = trainer_pair(monkeypatch)
    _, graph, _ = trainer_pair(monkeypatch)
    seed = next(sd for sd in range(100, 400) if all(rows_shared_by_more_than_two(fld, x) == 0 for x in batches(5, 24, sd)[0]))
    xs, ys = batches(5, 24, seed)
    graph.capture(24)
    assert graph._fused_field() is not None and graph.static_inputs()[0].shape == (24, 3)
    for x, y in zip(xs, ys):
        le, lg = eager.step(x.to(DEV), y.to(DEV)), graph.step(x.to(DEV), y.to(DEV))
        assert torch.equal(le.reshape(-1).cpu(), lg.reshape(-1).cpu())
    pe, pg = nef_params(eager.nef), nef_params(graph.nef)
    for k in GRADS:
        assert torch.equal(pe[k].detach().cpu(), pg[k].detach().cpu()), k
    assert not torch.equal(pe["table"].detach().cpu(), fld["table"])
    record("graph_vs_eager", seed=seed, steps=5, n=24, table_entries_moved=int((pe["table"].detach().cpu() != fld["table"]).sum()))


@pytest.mark.parametrize("bitwidth", [12, 14])
def test_captured_graph_at_512_coordinates_equals_eager_after_one_pass(monkeypatch, bitwidth):
    """forward + loss + backward once, eager launches against the replay of the captured graph, on 512 coordinates with contended
    table rows: the loss and the decoder's gradients bitwise (fixed summation order); the table gradients, whose atomics arrive in
    any order, each within the generic bound B of float64 (twice the modular path's measured error, at least one fp32 spacing of the
    largest entry) and therefore within 2 B of each other"""
    fld, eager, _ = trainer_pair(monkeypatch, bitwidth=bitwidth)
    _, graph, _ = trainer_pair(monkeypatch, bitwidth=bitwidth)
    xs, ys = batches(1, 512, 9)
    x, y = xs[0].to(DEV), ys[0].to(DEV)
    want = S.step_reference(fld, xs[0], ys[0])
    mod = modular_step(nef_of(fld), 3, x, y)
    graph.capture(512)
    assert graph._fused_field() is not None
    eager.flat.grad.zero_(); graph.flat.grad.zero_()
    le = eager._forward_backward(x, y)
    gx, gy = graph.static_inputs()
    gx.copy_(x); gy.copy_(y)
    graph._graph.replay()
    assert torch.equal(le.reshape(-1).cpu(), graph._g_loss.reshape(-1).cpu())
    ge = {k: p.grad.detach().cpu() for k, p in nef_params(eager.nef).items()}
    gg = {k: p.grad.detach().cpu() for k, p in nef_params(graph.nef).items()}
    for k in ("w1", "b1", "w2", "b2"):
        assert torch.equal(ge[k], gg[k]) and bool((ge[k] != 0).any()), k
    w = want["table"]
    B = max(2.0 * float((mod["table"].double() - w).abs().max()), FLOOR * float(w.abs().max()))
    apart = float((ge["table"] - gg["table"]).abs().max())
    record("graph_vs_eager_512", bitwidth=bitwidth, table_max_difference=apart, generic_bound=B, eager_from_float64=float((ge["table"].double() - w).abs().max()),
           graph_from_float64=float((gg["table"].double() - w).abs().max()))
    assert float((ge["table"].double() - w).abs().max()) <= B and float((gg["table"].double() - w).abs().max()) <= B
    assert apart <= 2.0 * B


def test_default_trainer_keeps_the_modular_launches(monkeypatch):
    from wisp.trainers import SDFTrainStep
    import wisp._C as C
    monkeypatch.delenv("WISP_SDF_TRAIN_FUSED", raising=False)
    fld = R.generic_field(HASH_FIELD["resolutions"], 128, F=8, multiscale='cat', seed=21)
    step = SDFTrainStep(nef_of(fld), lr=1e-3)

    def never(*a, **k):
        raise AssertionError("the default trainer took the fused hash step")
    monkeypatch.setattr(C, "hash_sdf_train_step", never)
    assert not step.fused_hash and step._fused_field() is None
    xs, ys = batches(2, 512, 8)
    losses = [float(step.step(x.to(DEV), y.to(DEV))) for x, y in zip(xs, ys)]
    want = S.step_reference(fld, xs[0], ys[0])
    assert abs(losses[0] - float(want["loss"])) <= 1e-5 * float(want["loss"]) and all(np.isfinite(losses))


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_train_nglod_script_trains_a_hash_grid_through_the_fused_step(tmp_path):
    """scripts/train_nglod.py --grid hash --fused-step on the procedural torus with small tables for two epochs"""
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_nglod.py"), "--write-test-mesh", str(tmp_path / "mesh"),
                        "--grid", "hash", "--fused-step", "--codebook-bitwidth", "12", "--level", "5", "--epochs", "2",
                        "--size", "64", "64", "--out-dir", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    losses = [float(line.split("l2 loss:")[1]) for line in r.stderr.splitlines() if "l2 loss:" in line]
    record("script", iou_before=rec["iou_before"], iou_after=rec["iou_after"], seconds=rec["seconds"], first_loss=losses[0],
           last_loss=losses[-1])
    assert rec["grid"] == "hash" and rec["fused_step"] is True and rec["fused_hash_step"] is True
    assert len(losses) == 2 and losses[-1] < losses[0]
    assert rec["iou_after"] > rec["iou_before"]
