"""GPU: the fused training step of an image field (wisp_image_field_train_step, csrc/image_field_train.hip) against the float64
reference of tests/image_step_ref.py - bit for bit on exactly representable inputs ("twin levels": float atomics included, exact
sums have no order), against the modular path's own error on generic ones - its forward against wisp_image_field_render, its
repeatability, and what is built on it: ImageTrainStep(fused=True) eager and graph-captured, and scripts/train_image.py
--fused-kernel.  Every measured margin is appended to profiles/image_step_test_margins.jsonl when WISP_IMAGE_STEP_MARGINS names a
file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_ref
import image_step_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GRADS = S.GRADS
OUTPUTS = ("loss",) + GRADS


def record(name, **values):
    path = os.environ.get("WISP_IMAGE_STEP_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=name, **{k: (float(v) if not isinstance(v, (int, str)) else v) for k, v in values.items()})) + "\n")


def dev_field(fld):
    """the kernel's field dict from a reference field, no nef in between"""
    return dict(codebook=fld["table"].to(DEV).contiguous(), begin_idxes=[int(b) for b in fld["begin"]],
                resolutions=list(fld["resolutions"]), codebook_bitwidth=fld["bitwidth"], active_lods=fld["active"],
                **{k: fld[k].to(DEV).contiguous() for k in ("w1", "b1", "w2", "b2")})


def prefill(fld):
    """gradient buffers holding non-zero multiples of 1/2 up to S.PREFILL_MAX (host copies): the step must ADD to them"""
    out = {}
    for k in GRADS:
        n = fld[k].numel()
        v = ((torch.arange(n) % 7).float() - 3.0) / 2.0
        v[v == 0] = S.PREFILL_MAX
        out[k] = v.reshape(fld[k].shape)
    return out


def run_step(dev, coords, rgb, before, want_pred=True):
    """one step on buffers holding `before` -> dict of host tensors: loss [1], pred [n, 3] and the five buffers afterwards"""
    import wisp._C as C
    bufs = {k: v.to(DEV).contiguous() for k, v in before.items()}
    loss, pred = C.image_field_train_step(coords.to(DEV), rgb.to(DEV), dev, bufs["table"], bufs["w1"], bufs["b1"], bufs["w2"], bufs["b2"],
                                          want_pred=want_pred)
    assert loss.shape == (1,) and loss.dtype == torch.float32 and (pred is None) == (not want_pred)
    return dict(loss=loss.cpu(), pred=None if pred is None else pred.cpu(), **{k: v.cpu() for k, v in bufs.items()})


def zeros(fld):
    return {k: torch.zeros(fld[k].shape) for k in GRADS}


_cache = {}


def exact(res, active, bitwidth, hidden, n):
    key = ("exact", tuple(res), active, bitwidth, hidden, n)
    if key not in _cache:
        case = S.exact_case(res, active, bitwidth, hidden, n, seed=2)
        case["dev"] = dev_field(case["field"])
        case["before"] = prefill(case["field"])
        _cache[key] = case
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1. exact inputs
@pytest.mark.parametrize("n", S.EXACT_N)
@pytest.mark.parametrize("res,active,bitwidth,hidden", S.EXACT_FIELDS)
def test_step_equals_float64_bit_for_bit_on_exact_inputs(res, active, bitwidth, hidden, n):
    """loss, table gradient, d W2, d b2, d b1 and the feature columns of d W1, on buffers pre-filled with non-zero values (the sums
    are ADDED); every colour is exactly 1/2; the rows of dead and of unread levels stay bitwise what they were.  (The embedding
    columns of d W1 are not exact - dh * sin is not: the generic comparison covers them.)"""
    case = exact(res, active, bitwidth, hidden, n)
    fld, want, before = case["field"], case["want"], case["before"]
    L2 = 2 * len(res)
    got = run_step(case["dev"], case["coords"], case["rgb"], before)
    assert torch.equal(got["loss"].double(), want["loss"]), (float(got["loss"]), float(want["loss"]))
    assert torch.equal(got["pred"], torch.full((n, 3), 0.5))
    for k in ("table", "b1", "w2", "b2"):
        assert torch.equal(got[k].double(), before[k].double() + want[k].reshape(before[k].shape)), k
    assert torch.equal(got["w1"][:, :L2].double(), before["w1"][:, :L2].double() + want["w1"][:, :L2])
    assert bool(torch.isfinite(got["w1"]).all())
    begin = fld["begin"]
    for l in case["unread"] + list(range(active, len(res))):
        a, b = int(begin[l]), int(begin[l + 1])
        assert torch.equal(got["table"][a:b], before["table"][a:b]), l
        if l >= active:                                                            # a dead level's W1 columns: zero added
            assert torch.equal(got["w1"][:, 2 * l:2 * l + 2], before["w1"][:, 2 * l:2 * l + 2]), l
    record("exact", res=str(tuple(res)), active=active, bitwidth=bitwidth, hidden=hidden, n=n,
           quanta_used=max(case["spans"].values()), table_entries_moved=int((want["table"] != 0).sum()))


# ------------------------------------------------------------------------------------------------ 2. the forward
def render(fld, coords):
    """wisp_image_field_render's colours at `coords` for a reference field"""
    import wisp._C as C
    d = {k: fld[k].to(DEV) for k in ("w1", "b1", "w2", "b2")}
    packed, hp = C.image_field_pack_weights(d["w1"], d["b1"], d["w2"], d["b2"], len(fld["resolutions"]))
    n = coords.shape[0]
    return C.image_field_render(1, 1, 0, n, fld["table"].to(DEV), fld["begin"].to(DEV), list(fld["resolutions"]), fld["bitwidth"],
                                fld["active"], packed, hp, coords=coords.to(DEV))[0].cpu()


def actives(L):
    return sorted({0, L - 1, L})


FORWARD = [(H, L, a, bw) for H in (1, 17, 64, 128) for L in (1, 5, 16) for a in actives(L) for bw in (8, 12)] + [(64, 16, 15, 19)]


@pytest.mark.parametrize("hidden,L,active,bitwidth", FORWARD)
def test_predicted_colours_are_the_render_kernels_bit_for_bit(hidden, L, active, bitwidth):
    """generic fields; coordinates outside [-1, 1] and on cell faces among them; 1, 63, 65 and 1000 pixels"""
    fld = S.generic_field(L, hidden, active, bitwidth, seed=5)
    dev = dev_field(fld)
    for n in (1, 63, 65, 1000):
        coords, rgb = S.generic_points(n, seed=n), S.generic_targets(n, seed=n)
        got = run_step(dev, coords, rgb, zeros(fld))
        want = render(fld, coords)
        assert torch.equal(got["pred"], want), (n, float((got["pred"] - want).abs().max()))
        assert bool(((got["pred"] > 0) & (got["pred"] < 1)).all())
        if n == 1000:
            assert bool((coords.abs() > 1).any())


# ------------------------------------------------------------------------------------------------ 3. generic gradients
# (hidden, L, active, bitwidth): the forward's grid thinned to a dozen shapes
GENERIC = [(1, 1, 1, 8), (1, 5, 4, 12), (17, 1, 0, 12), (17, 5, 5, 8), (17, 16, 15, 12), (64, 5, 4, 12), (64, 16, 15, 8), (64, 16, 16, 12),
           (128, 1, 1, 12), (128, 5, 0, 8), (128, 16, 15, 12), (64, 16, 15, 19)]
# Bound of a generic output: twice the modular path's own largest error against float64 on that output, with a floor where that
# error measures nothing (the floors of test_gpu_hash_sdf_step.py).  Array outputs: one fp32 spacing at the output's largest
# magnitude, 2^-23 max|want| - an fp32 result lies up to half a spacing from the true value however it was summed.  The
# one-element loss and each entry of d b2: there the modular path's error is ONE number per entry, a sum of signed errors that may
# cancel to anything.  What does not cancel by luck is what the sum is made of.  With e = the modular path's largest error of a
# predicted COLOUR s against float64, to first order in e:
#     loss = sum (s - t)^2 / (3 n)                    ->  |d loss|    <= (2 / (3 n)) sum |s - t| e
#     d b2_k = sum_i (2 (s - t) / (3 n)) s (1 - s)    ->  |d (d b2_k)| <= (2 / (3 n)) sum_i |s (1 - s) + (s - t) (1 - 2 s)| e
# (the derivative of (s - t) s (1 - s) with respect to s); the floor is twice that - the modular path's own error, propagated, times
# the same factor 2 - plus two fp32 spacings of the result.
FLOOR = 2.0 ** -23


def scalar_floor(k, want, rgb, e_pred):
    n = rgb.shape[0]
    s, t = want["pred"], rgb.double()
    if k == "loss":
        propagated = (2.0 / (3 * n)) * float((s - t).abs().sum()) * e_pred
    else:
        propagated = (2.0 / (3 * n)) * float((s * (1 - s) + (s - t) * (1 - 2 * s)).abs().sum(0).max()) * e_pred
    return 2.0 * propagated + 2.0 * FLOOR * float(want[k].abs().max())


def nef_of(fld, coord_dim=2):
    """ImageNeuralField over a HashGrid carrying a reference field's parameters (training mode, gradients on)"""
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import ImageNeuralField
    grid = HashGrid.from_resolutions(None, feature_dim=2, resolutions=list(fld["resolutions"]), multiscale_type='cat', feature_std=0.01,
                                     codebook_bitwidth=fld["bitwidth"], coord_dim=coord_dim)
    nef = ImageNeuralField(grid, hidden_dim=fld["w1"].shape[0])
    with torch.no_grad():
        assert grid.codebook.feats.shape == fld["table"].shape
        grid.codebook.feats.data = fld["table"].clone()
        nef.decoder.layers[0].weight.copy_(fld["w1"]); nef.decoder.layers[0].bias.copy_(fld["b1"])
        nef.decoder.lout.weight.copy_(fld["w2"]); nef.decoder.lout.bias.copy_(fld["b2"])
    return nef.to(DEV).train()


def nef_params(nef):
    dec = nef.decoder
    return dict(table=nef.grid.codebook.feats, w1=dec.layers[0].weight, b1=dec.layers[0].bias, w2=dec.lout.weight, b2=dec.lout.bias)


def fld_of(nef):
    """the reference's field dict from a nef (host copies; rgb()'s default blends the levels below the finest)"""
    grid = nef.grid
    prm = {k: v.detach().cpu().clone() for k, v in nef_params(nef).items()}
    return dict(begin=grid.codebook.begin_idxes.cpu().clone(), resolutions=[int(r) for r in grid.resolutions],
                bitwidth=int(grid.codebook_bitwidth), active=grid.num_lods - 1, **prm)


def modular_step(nef, active, coords, rgb):
    """the modular path: autograd over nef.rgb (wisp.ops.grid.hashgrid, the embedder, the decoder, the sigmoid) and F.mse_loss"""
    nef.zero_grad(set_to_none=True)
    pred = nef.rgb(coords, lod=active)
    loss = torch.nn.functional.mse_loss(pred, rgb)
    loss.backward()
    prm = nef_params(nef)
    return dict(loss=loss.detach().reshape(1).cpu(), pred=pred.detach().cpu(),
                **{k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().reshape(p.shape) for k, p in prm.items()})


def generic_setup(hidden, L, active, bitwidth, n):
    key = ("generic", hidden, L, active, bitwidth, n)
    if key not in _cache:
        fld = S.generic_field(L, hidden, active, bitwidth, seed=3)
        coords, rgb = S.generic_points(n, seed=9), S.generic_targets(n, seed=9)
        _cache[key] = (fld, coords, rgb, S.step_reference(fld, coords, rgb))
    return _cache[key]


@pytest.mark.parametrize("n", [15, 65, 1000])
@pytest.mark.parametrize("hidden,L,active,bitwidth", GENERIC)
def test_step_error_is_within_twice_the_modular_paths(hidden, L, active, bitwidth, n):
    fld, coords, rgb, want = generic_setup(hidden, L, active, bitwidth, n)
    got = run_step(dev_field(fld), coords, rgb, zeros(fld))
    mod = modular_step(nef_of(fld), active, coords.to(DEV), rgb.to(DEV))
    failures = []
    e_pred = float((mod["pred"].double() - want["pred"]).abs().max())
    for k in OUTPUTS:
        w = want[k].reshape(got[k].shape)
        e_fused, e_mod = float((got[k].double() - w).abs().max()), float((mod[k].reshape(got[k].shape).double() - w).abs().max())
        bound = max(2.0 * e_mod, scalar_floor(k, want, rgb, e_pred) if k in ("loss", "b2") else FLOOR * float(w.abs().max()))
        record("generic", hidden=hidden, L=L, active=active, bitwidth=bitwidth, n=n, output=k, err_fused=e_fused, err_modular=e_mod,
               bound=bound, largest=float(w.abs().max()))
        print(f"h{hidden} L{L} active{active} bw{bitwidth} n{n} {k}: fused {e_fused:.3e} modular {e_mod:.3e} bound {bound:.3e}")
        if not e_fused <= bound:
            failures.append((k, e_fused, e_mod, bound))
    assert not failures, failures
    assert bool((got["table"][int(fld["begin"][active]):] == 0).all()) and bool((got["w1"][:, 2 * active:2 * L] == 0).all())
    assert float(want["loss"]) > 0 and (active == 0 or float(want["table"].abs().max()) > 0)


# ------------------------------------------------------------------------------------------------ 4. repeatability
def test_two_runs_are_bitwise_equal_where_the_sums_have_an_order_or_are_exact():
    fld, coords, rgb, _ = generic_setup(64, 16, 15, 19, 1000)              # levels on the fp64 accumulators and on f32 atomics
    dev = dev_field(fld)
    a, b = run_step(dev, coords, rgb, zeros(fld)), run_step(dev, coords, rgb, zeros(fld))
    for k in ("loss", "pred", "w1", "b1", "w2", "b2"):                     # fixed summation order
        assert torch.equal(a[k], b[k]), k
    scale = float(a["table"].abs().max())
    apart = float((a["table"] - b["table"]).abs().max())
    record("repeat_generic_table", max_difference=apart, largest=scale)
    assert apart <= 1e-5 * scale                                           # atomics: arrival order
    case = exact(S.EIGHT_PAIRS, 15, 10, 128, 1024)
    a, b = (run_step(case["dev"], case["coords"], case["rgb"], case["before"]) for _ in range(2))
    for k in OUTPUTS + ("pred",):                                          # exact sums have no order
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 5. ImageTrainStep(fused=True)
# the settings of test_gpu_image_app.py's ImageTrainStep-against-Adam test: hidden 64 over 16 levels 16 .. 128 at 2^14 rows, table
# entries N(0, 0.05), lr 1e-3, eps 1e-15, grid lr x 2, 512 pixels of a 64 x 64 image
LR, EPS, GLW = 1e-3, 1e-15, 2.0


def app_field(seed):
    from wisp.models.grids import HashGrid
    from wisp.models.nefs import ImageNeuralField
    torch.manual_seed(seed)
    grid = HashGrid.from_geometric(None, feature_dim=2, num_lods=16, multiscale_type='cat', feature_std=0.05, codebook_bitwidth=14,
                                   min_grid_res=16, max_grid_res=128)
    return ImageNeuralField(grid, hidden_dim=64).to(DEV)


def trainer_pair(monkeypatch, seed=5):
    """two trainers from equal initial state: the fused step, and the same trainer kept on its modular launches"""
    from wisp.trainers import ImageTrainStep
    monkeypatch.delenv("WISP_IMAGE_TRAIN_FUSED", raising=False)
    fused = ImageTrainStep(app_field(seed), lr=LR, eps=EPS, grid_lr_weight=GLW, fused=True)
    assert fused._fused_field() is not None
    monkeypatch.setenv("WISP_IMAGE_TRAIN_FUSED", "0")
    modular = ImageTrainStep(app_field(seed), lr=LR, eps=EPS, grid_lr_weight=GLW, fused=True)
    assert modular._fused_field() is None
    monkeypatch.delenv("WISP_IMAGE_TRAIN_FUSED")
    return fld_of(fused.nef), fused, modular


def batches(steps, n, seed):
    import wisp._C as C
    bank = torch.from_numpy(image_ref.procedural_image(64, 64)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(steps):
        s = C.image_sample(bank, torch.randint(0, 64 * 64, (n,), device=DEV, generator=g))
        out.append((s["coords"], s["rgb"]))
    return out


def test_trainer_one_step_agrees_with_the_modular_trainer(monkeypatch):
    """Adam's first step moves a parameter by lr * g / (|g| + eps).  Both trainers start from equal state.  With B the generic
    bound of a gradient tensor (twice the modular path's measured error against float64, at least one fp32 spacing at the largest
    entry), both paths' gradients lie within B of the float64 one, so where |g| > 4 B the two updates differ by at most
    lr * 2 B / (|g| - B), plus the fp32 rounding of the update itself (2^-22 of the larger of |p| and lr).  Entries with a smaller
    gradient get the bound that holds for any: there the sign of a rounding decides a full step, so the two lie within 2 lr."""
    fld, fused, modular = trainer_pair(monkeypatch)
    (x, y), = batches(1, 512, 5)
    want = S.step_reference(fld, x.cpu(), y.cpu())
    mod = modular_step(app_field(5).train(), 15, x, y)
    lf, lm = fused.step(x, y), modular.step(x, y)
    e_pred = float((mod["pred"].double() - want["pred"]).abs().max())
    assert abs(float(lf) - float(lm)) <= 2.0 * scalar_floor("loss", want, y.cpu(), e_pred)
    for k in GRADS:
        lr = LR * (GLW if k == "table" else 1.0)
        pf, pm = nef_params(fused.nef)[k].detach().cpu().double(), nef_params(modular.nef)[k].detach().cpu().double()
        g = want[k].reshape(pf.shape)
        p0 = fld[k].reshape(pf.shape).double()
        B = max(2.0 * float((mod[k].reshape(pf.shape).double() - g).abs().max()), FLOOR * float(g.abs().max()))
        big = g.abs() > 4.0 * B
        assert int(big.sum()) > 0, k
        allowed = lr * 2.0 * B / (g.abs() - B).clamp(min=B) + 2.0 ** -22 * p0.abs().clamp(min=lr)
        excess = ((pf - pm).abs() - allowed)[big]
        record("trainer_one_step", tensor=k, generic_bound=B, entries=int(big.sum()), nonzero_entries=int((g != 0).sum()), max_parameter_difference=float((pf - pm).abs()[big].max()),
               largest_share_of_allowed=float(((pf - pm).abs() / allowed)[big].max()), lr=lr)
        assert float(excess.max()) <= 0.0, (k, float(excess.max()))
        # ... and no entry, whatever its gradient, is further apart than two full Adam steps in opposite directions
        assert float(((pf - pm).abs() - 2.0 * lr - 2.0 ** -22 * p0.abs().clamp(min=lr)).max()) <= 0.0, k
        assert float((pf - p0).abs()[big].min()) > 0.5 * lr                        # a full Adam step where there is a gradient
    dead = int(fld["begin"][15])
    assert torch.equal(nef_params(fused.nef)["table"].detach().cpu()[dead:], fld["table"][dead:])      # the finest level: no gradient


def test_thirty_steps_follow_adam_on_the_float64_gradients(monkeypatch):
    """loss curve over 30 steps against torch.optim.Adam on the float64-checked gradients (tests/image_step_ref.py, parameters kept
    in float64): the fused trainer's distance from that curve is allowed twice the modular trainer's own, both recorded"""
    steps = 30
    fld, fused, modular = trainer_pair(monkeypatch)
    data = batches(steps, 512, 6)
    params = [torch.nn.Parameter(fld[k].double().clone()) for k in GRADS]
    opt = torch.optim.Adam([dict(params=params[:1], lr=LR * GLW), dict(params=params[1:], lr=LR)], eps=EPS)
    curve, lf, lm = [], [], []
    for x, y in data:
        now = dict(fld, **{k: p.detach().float() if k == "table" else p.detach() for k, p in zip(GRADS, params)})
        # (the reference's forward reads an f32 table; its float64 master copy takes the update)
        want = S.step_reference(now, x.cpu(), y.cpu())
        curve.append(float(want["loss"]))
        for k, p in zip(GRADS, params):
            p.grad = want[k].reshape(p.shape).clone()
        opt.step()
        lf.append(float(fused.step(x, y)))
        lm.append(float(modular.step(x, y)))
    curve, lf, lm = np.array(curve), np.array(lf), np.array(lm)
    d_fused, d_mod = float(np.abs(lf - curve).max()), float(np.abs(lm - curve).max())
    record("trainer_thirty_steps", fused_from_float64=d_fused, modular_from_float64=d_mod, first_loss=curve[0], last_loss=curve[-1])
    print(f"30 steps: fused {d_fused:.3e} modular {d_mod:.3e} loss {curve[0]:.4e} -> {curve[-1]:.4e}")
    assert curve[-1] < curve[0] and lf[-1] < lf[0]
    assert d_fused <= 2.0 * d_mod, (d_fused, d_mod)


def test_captured_graph_equals_the_eager_fused_step(monkeypatch):
    """capture(80), then five replays against five eager fused steps from equal state.  First step: the loss and - their gradient
    sums having a fixed order - the decoder's parameters bitwise.  Over the five steps: test 4 lets two runs' table gradients
    differ by 1e-5 of the largest entry (atomics arrive in any order); Adam turns a gradient difference into a parameter
    difference of at most two steps per update where the gradient is small, so every parameter stays within 5 x 2 lr, the loss
    within 1e-5 relative per step taken, and all but a small share of the entries within lr x 1e-3."""
    _, eager, _ = trainer_pair(monkeypatch)
    _, graph, _ = trainer_pair(monkeypatch)
    data = batches(5, 80, 11)
    graph.capture(80)
    assert graph._fused_field() is not None and graph.static_inputs()[0].shape == (80, 2)
    for it, (x, y) in enumerate(data):
        le, lg = eager.step(x, y), graph.step(x, y)
        if it == 0:
            assert torch.equal(le.reshape(-1).cpu(), lg.reshape(-1).cpu())
            for k in ("w1", "b1", "w2", "b2"):
                assert torch.equal(nef_params(eager.nef)[k].detach().cpu(), nef_params(graph.nef)[k].detach().cpu()), k
        record("graph_vs_eager_loss", step=it, eager=float(le), graph=float(lg))
        assert abs(float(le) - float(lg)) <= 1e-5 * (it + 1) * max(1.0, abs(float(le))), it
    pe, pg = nef_params(eager.nef), nef_params(graph.nef)
    for k in GRADS:
        lr = LR * (GLW if k == "table" else 1.0)
        a, b = pe[k].detach().cpu().double(), pg[k].detach().cpu().double()
        apart = (a - b).abs()
        record("graph_vs_eager", tensor=k, max_parameter_difference=float(apart.max()), share_beyond_a_thousandth_step=float((apart > 1e-3 * lr).double().mean()))
        assert float(apart.max()) <= 5 * 2.0 * lr, k
        assert float((apart > 1e-3 * lr).double().mean()) <= 0.01, k
    assert not torch.equal(pe["table"].detach().cpu(), fld_of(app_field(5))["table"])


def test_default_trainer_keeps_the_modular_launches(monkeypatch):
    from wisp.trainers import ImageTrainStep
    import wisp._C as C
    monkeypatch.delenv("WISP_IMAGE_TRAIN_FUSED", raising=False)
    nef = app_field(5)
    fld = fld_of(nef)
    step = ImageTrainStep(nef, lr=LR, eps=EPS, grid_lr_weight=GLW)

    def never(*a, **k):
        raise AssertionError("the default trainer took the fused image step")
    monkeypatch.setattr(C, "image_field_train_step", never)
    assert not step.fused and step._fused_field() is None
    data = batches(2, 512, 8)
    losses = [float(step.step(x, y)) for x, y in data]
    want = S.step_reference(fld, data[0][0].cpu(), data[0][1].cpu())
    assert abs(losses[0] - float(want["loss"])) <= 1e-5 * float(want["loss"]) and all(np.isfinite(losses))


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_train_image_script_trains_through_the_fused_kernel(tmp_path):
    """scripts/train_image.py --fused-kernel on its procedural 64 x 64 picture for two epochs of 256-pixel steps"""
    img, log_dir = str(tmp_path / "test.png"), str(tmp_path / "run")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_image.py"), "--write-test-image", img, "--size", "64", "64",
                        "--epochs", "2", "--num-pixels", "256", "--fused-kernel", "--log-dir", log_dir],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    record("script", psnr_first_epoch=rec["psnr_first_epoch"], psnr=rec["psnr"], seconds=rec["seconds"], ms_per_step=rec["ms_per_step"])
    assert rec["step"] == "ImageTrainStep" and rec["fused_image_step"] is True
    assert np.isfinite(rec["psnr"]) and rec["psnr"] > rec["psnr_first_epoch"], rec
