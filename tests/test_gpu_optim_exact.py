"""Rounding-faithful tests of the optimizer kernels (csrc/misc.hip) and of the AdamW step folded into the hash-grid reduce kernel's
flush (csrc/hashgrid.hip), against tests/optim_exact_ref.py.

AdamW: NO TOLERANCE ANYWHERE.  wisp_adamw_update is mul, add, fma, sqrt and div with contraction pinned, each correctly rounded, so
param, exp_avg, exp_avg_sq, the zeroed gradient and the bf16 shadow must equal the fp32 restatement (exact fma, the C library's
powf for the bias corrections) in `torch.equal` AND in the bit patterns of the magnitudes - denormal second moments included.  A
bit that differs is a defect of the kernel or of its build flags: tests/test_optim_exact_host.py rules out the reference (against
exact rationals), asserts the regime shares below and shows that each check can fail.  Every failure names the element, the got
and want bits and the g, m and v that went in.

Adam with L2 decay and RMSprop (kinds 1 and 2): the compiler chooses the contractions, so each step is held inside a running
bound around the float64 value that is DERIVED FROM OPERATION COUNTS - 2^-24 of the result's magnitude per fp32 operation, 2^-150
where a product or quotient can be denormal, propagated through the following operations, no other factor.  Every step starts
from the kernel's own previous state, so bounds do not compound; the shadow must be bfloat16() of the parameter the kernel wrote.

What each test reaches (shares of the elements, asserted on the host for sizes 1023, 1025, 65 539 and the wrap buffer):
  flat AdamW (wisp_adamw_step, wisp_adamw_step_groups, wisp_optim_step_groups kind 0), three hyper-parameter sets (nerf_hash.yaml's
    betas and eps = 1e-15; 0.85 / 0.99 with eps = 1e-8 and weight decay 0 and 1e-2), grad_scale 1, 1/128 and 2^-30, steps 1, 2, 3
    from a fresh state and steps 1000 and 30000 (bias corrections exactly 1) from a mid-training state: a denormal v (9 % of 65 539
    elements), v == 0 under a non-zero gradient (6 to 33 %), eps decides (39 to 80 %), eps invisible (5 to 45 %), a parameter that
    keeps its bits (weight decay 0: 41 to 64 %) or moves by weight decay alone (19 to 64 %), planted shadow ties (3 %), +0 and -0
    gradients;
    sizes 1, 3, 4, 5, 1023, 1025, 65 539: the scalar tail of adamw_kernel, ragged last chunks, more than one workgroup;
    groups beginning at 0, 1, 2, 3 mod 4 and on the 8-byte path, lengths no multiples of 4, gaps that stay untouched, five groups
    (two launches of the wrapper); kind 0 of wisp_optim_step_groups takes four 16-byte aligned groups (all it accepts);
    GUARD elements on both sides of every buffer; the zeroed gradient, and the gradient left alone without zero_grad;
  the wrap buffer (4096 x 256 x 4 + 4 x 256 + 3 elements): the second trip of the grid-stride loop and its ragged end, all three
    launches;
  Adam / RMSprop (with and without momentum): the same sizes, starts and scales, and the wrap buffer;
  folded AdamW: the F = 2 pair path of a dense multi-bucket level with one owner (strips) at an odd first row, of a hashed level
    with one owner, the tail workgroups of a dead suffix (weight decay alone), rows of split levels that stay the caller's, a
    denormal v through grad_scale 2^-70, fp32 and compact bf16 records; the oddly-aligned fallbacks of both flushes, which the
    kernel takes when a caller's tensors lie 4 bytes off an 8-byte boundary (a level's odd first row does NOT reach them: with
    F = 2 every row is 8 bytes).  There is no generic-F fold: the launcher compiles the fused flush for F = 2 only, and the F = 4
    and F = 8 cases must report nothing covered, leave the state alone and hold the plain gradient.
"""
import numpy as np
import pytest
import torch

import hashgrid_exact_ref as H
import optim_exact_ref as O
from gpu_helpers import DEV, _C

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements in front of and behind every buffer that a kernel must leave alone
SENTINEL = 7.0
APIS = ("adamw_step", "adamw_step_groups", "optim_step_groups")
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _cache.clear()
    H._cases.clear()
    _C()._slot_fits.clear()


# ---------------------------------------------------------------------------------------------------- buffers and comparison
def _guarded(x, dtype=torch.float32, shift=0):
    """the values x [n] (numpy, or a count of sentinels) inside an allocation with GUARD sentinels on either side; shift: extra
    elements in front (an oddly aligned buffer)"""
    n = x if isinstance(x, int) else x.shape[0]
    whole = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=dtype, device=DEV)[shift:]
    if not isinstance(x, int):
        whole[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return whole


def _in(whole):
    return whole[GUARD:whole.numel() - GUARD]


def _set(whole, x):
    _in(whole).copy_(torch.from_numpy(np.ascontiguousarray(x)))


def _host(t):
    """a host copy that later launches cannot reach"""
    return t.detach().cpu().clone()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _hex(t, i):
    return f"{int(_bits(t)[i]) & (0xFFFFFFFF if t.dtype == torch.float32 else 0xFFFF):#x}"


def _going_in(before, i):
    return ", ".join(f"{k} = {float(t[i])!r} ({_hex(t, i)})" for k, t in before.items() if 0 <= i < t.numel())


def _same(got, want, what, before):
    """whole guarded buffers, bit for bit on the host: values and the bit patterns of the magnitudes (an equality that flushed
    denormals would not do).  before: g, m, v going in, indexed like `got`."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if torch.equal(got, want) and torch.equal(_bits(got.abs()), _bits(want.abs())):
        return
    bad = torch.nonzero((got != want) | (_bits(got.abs()) != _bits(want.abs()))).flatten()
    lines = [f"element {i - GUARD}: got {float(got[i])!r} ({_hex(got, i)}), want {float(want[i])!r} ({_hex(want, i)}); going in: "
             f"{_going_in(before, i)}" for i in bad[:6].tolist()]
    raise AssertionError(f"{what}: {bad.numel()} of {got.numel() - 2 * GUARD} elements (+ guards) differ\n  " + "\n  ".join(lines))


def _inside(what, name, got, val, err, before):
    """kinds 1 and 2: |got - float64 value| <= running bound, element by element (bound 0 outside the groups)"""
    got = got.detach().cpu()[GUARD:-GUARD].double().numpy()
    assert np.isfinite(got).all(), (what, name)
    bad = np.flatnonzero(~(np.abs(got - val) <= err))
    if bad.size:
        lines = [f"element {i}: got {got[i]!r}, float64 {val[i]!r}, off by {abs(got[i] - val[i]):.3e}, bound {err[i]:.3e}; going in: "
                 f"{_going_in(before, i + GUARD)}" for i in bad[:6].tolist()]
        raise AssertionError(f"{what}: {name} leaves the running bound on {bad.size} of {got.size} elements\n  " + "\n  ".join(lines))


def _window(before, begin, length):
    """the guarded window of a group's elements: indexed like the group's guarded shadow"""
    return {k: t[begin:begin + length + 2 * GUARD] for k, t in before.items()}


# ---------------------------------------------------------------------------------------------------- flat launches
def _layout(api, n, wd):
    """-> [(begin, len, lr, wd)] and which groups write a shadow"""
    wds = (wd, wd, 0.0, wd, 1e-2)
    if api == "adamw_step_groups":
        groups = O.group_layout(n, 5, (0, 1, 2, 3, 2), wds)
    elif api == "optim_step_groups":
        groups = O.group_layout(n, 4, (0, 0, 0, 0), wds)
    else:
        return None, [True]
    return groups, [k % 2 == 0 for k in range(len(groups))]


def _launch(api, W, SH, groups, h, step, gs, zero_grad, kind="adamw"):
    C = _C()
    p, g, m, v = (_in(W[k]) if W[k] is not None else None for k in "pgmv")
    sh = [_in(s) if s is not None else None for s in SH]
    if api == "adamw_step":
        (_, _, lr, wd), = groups
        C.adamw_step(p, g, m, v, lr, h["beta1"], h["beta2"], h["eps"], wd, step, grad_scale=gs, zero_grad=zero_grad, bf16_shadow=sh[0])
    else:
        spec = [(b, ln, lr, wd, sh[k]) for k, (b, ln, lr, wd) in enumerate(groups)]
        if api == "adamw_step_groups":
            C.adamw_step_groups(p, g, m, v, spec, h["beta1"], h["beta2"], h["eps"], step, grad_scale=gs, zero_grad=zero_grad)
        else:
            C.optim_step_groups(kind, p, g, m, v, spec, h["beta1"], h["beta2"], h["eps"], step, grad_scale=gs, zero_grad=zero_grad)
    torch.cuda.synchronize()


def _adamw_step_checked(api, W, SH, groups, h, step, gs, zero_grad, what):
    """one launch from the state in W, every buffer compared whole (guards, gaps between the groups) with the restatement fed the
    same state"""
    before = {k: _host(W[k]) for k in "pmvg"}
    sh_before = [_host(s) if s is not None else None for s in SH]
    _launch(api, W, SH, groups, h, step, gs, zero_grad)
    host = {k: before[k][GUARD:-GUARD].numpy() for k in "pmvg"}
    ref = O.adamw_groups(host["p"], host["m"], host["v"], host["g"], [(b, ln, lr, wd, SH[k] is not None) for k, (b, ln, lr, wd) in enumerate(groups)],
                         h["beta1"], h["beta2"], h["eps"], step, gs, zero_grad)
    ctx = {k: before[k] for k in "gmv"}
    for k, name in (("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("g", "grad")):
        want = before[k].clone()
        want[GUARD:-GUARD] = torch.from_numpy(ref[k])
        _same(W[k], want, f"{what}: {name}", ctx)
    for k, s in enumerate(SH):
        if s is not None:
            want = sh_before[k].clone()
            want[GUARD:-GUARD] = ref["shadows"][k]
            _same(s, want, f"{what}: bf16 shadow of group {k}", _window(ctx, groups[k][0], groups[k][1]))


def _flat_buffers(n, groups, shadowed, step):
    x = O.start_state(n, step, O.decay_of(n, groups))
    W = {k: _guarded(x[k]) for k in "pmvg"}
    SH = [_guarded(ln, torch.bfloat16) if shadowed[k] else None for k, (_, ln, _, _) in enumerate(groups)]
    return W, SH


# (first step, steps) of the runs from one start state: 1, 2, 3 from a fresh one, 1000 and 30000 from a mid-training one
RUNS = [(1, O.FRESH_STEPS)] + [(s, (s,)) for s in O.MID_STEPS]


@pytest.mark.parametrize("hyper", sorted(O.HYPER))
@pytest.mark.parametrize("api", APIS)
def test_adamw_equals_the_fp32_restatement_bit_for_bit(api, hyper):
    h = O.HYPER[hyper]
    for n in O.SIZES:
        groups, shadowed = _layout(api, n, h["wd"])
        if groups is None:
            groups = [(0, n, h["lr"], h["wd"])]
        for gs in O.GRAD_SCALES:
            for first, steps in RUNS:
                W, SH = _flat_buffers(n, groups, shadowed, first)
                for step in steps:
                    if step != first:
                        _set(W["g"], O.step_gradient(n, step))
                    _adamw_step_checked(api, W, SH, groups, h, step, gs, zero_grad=step % 2 == 1 or step == 1000,
                                        what=f"{api}, {hyper}, n = {n}, grad_scale {gs!r}, step {step}, groups {groups if len(groups) > 1 else '-'}")


@pytest.mark.parametrize("api", APIS)
def test_adamw_grid_stride_wrap_and_ragged_tail(api):
    """4096 x 256 x 4 + 4 x 256 + 3 elements: every thread of the capped grid comes round a second time and the last chunk is ragged;
    one step at 1000 from the mid-training state, nerf_hash.yaml's hyper-parameters, grad_scale 1 / 128"""
    h = O.HYPER["hash"]
    if api == "adamw_step":
        n, groups, shadowed = O.WRAP_N, [(0, O.WRAP_N, h["lr"], h["wd"])], [True]
    else:
        n, groups = O.wrap_layout(5 if api == "adamw_step_groups" else 4, (h["wd"],))
        shadowed = [k % 2 == 0 for k in range(len(groups))]
    W, SH = _flat_buffers(n, groups, shadowed, 1000)
    _adamw_step_checked(api, W, SH, groups, h, 1000, 1.0 / 128.0, True, f"{api}, wrap buffer of {n} elements, groups {groups}")


# ---------------------------------------------------------------------------------------------------- Adam and RMSprop
def _kind_step_checked(kind, W, SH, groups, hy, step, gs, zero_grad, what):
    names = "pmvg" if W["m"] is not None else "pvg"
    before = {k: _host(W[k]) for k in names}
    sh_before = [_host(s) if s is not None else None for s in SH]
    h = dict(beta1=hy["h0"], beta2=hy["h1"], eps=hy["eps"])
    _launch("optim_step_groups", W, SH, groups, h, step, gs, zero_grad, kind=kind)
    host = {k: before[k][GUARD:-GUARD].numpy() for k in names}
    ref = O.bounded_groups(kind, host["p"], host.get("m"), host["v"], host["g"], [(b, ln, lr, wd, None) for b, ln, lr, wd in groups],
                           hy["h0"], hy["h1"], hy["eps"], step, gs, zero_grad)
    ctx = {k: before[k] for k in names if k != "p"}
    for k, r, name in (("p", "p", "param"), ("m", "s1", "state1"), ("v", "s2", "state2")):
        if W[k] is None:
            continue
        _inside(what, name, W[k], ref[r][0], ref[r][1], ctx)
        got = W[k].cpu()
        assert torch.equal(got[:GUARD], before[k][:GUARD]) and torch.equal(got[-GUARD:], before[k][-GUARD:]), f"{what}: guards of {name}"
    want = before["g"].clone()
    want[GUARD:-GUARD] = torch.from_numpy(ref["g"])
    _same(W["g"], want, f"{what}: grad", ctx)
    p_now = W["p"].cpu()[GUARD:-GUARD]
    for k, s in enumerate(SH):
        if s is not None:
            b, ln = groups[k][:2]
            want = sh_before[k].clone()
            want[GUARD:-GUARD] = p_now[b:b + ln].bfloat16()
            _same(s, want, f"{what}: bf16 shadow of group {k}", _window(ctx, b, ln))


def _kind_buffers(kind, hy, n, groups, step):
    x = O.start_state(n, step)
    W = {k: _guarded(x[k]) for k in "pmvg"}
    if kind == "rmsprop" and hy["h1"] == 0.0:
        W["m"] = None
    SH = [_guarded(ln, torch.bfloat16) if k % 2 == 0 else None for k, (_, ln, _, _) in enumerate(groups)]
    return W, SH


@pytest.mark.parametrize("kind,k", [("adam", 0), ("adam", 1), ("rmsprop", 0), ("rmsprop", 1)])
def test_adam_and_rmsprop_stay_inside_the_running_bound(kind, k):
    hy = O.KIND_HYPER[kind][k]
    for n in O.SIZES:
        groups = O.group_layout(n, 4, (0, 0, 0, 0), (hy["wd"], 0.0, 1e-2))
        for gs in O.GRAD_SCALES:
            for first, steps in RUNS:
                W, SH = _kind_buffers(kind, hy, n, groups, first)
                for step in steps:
                    if step != first:
                        _set(W["g"], O.step_gradient(n, step))
                    _kind_step_checked(kind, W, SH, groups, hy, step, gs, step % 2 == 1 or step == 1000,
                                       f"{kind} {hy}, n = {n}, grad_scale {gs!r}, step {step}, groups {groups if len(groups) > 1 else '-'}")


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_adam_and_rmsprop_grid_stride_wrap_and_ragged_tail(kind):
    hy = O.KIND_HYPER[kind][1]
    n, groups = O.wrap_layout(4, (hy["wd"],))
    W, SH = _kind_buffers(kind, hy, n, groups, 1000)
    _kind_step_checked(kind, W, SH, groups, hy, 1000, 1.0 / 128.0, True, f"{kind} {hy}, wrap buffer of {n} elements, groups {groups}")


# ---------------------------------------------------------------------------------------------------- the folded step
def _folded_case(name):
    if name not in _cache:
        case = H.bwd_case(name)
        td = H.DTYPES[case["dtype"]]
        dev = dict(coords=case["coords"].to(DEV), grad_out=case["grad_out"].float().to(td).to(DEV), first_idx=case["first_idx"].to(DEV))
        _cache[name] = (case, H.reference_backward(case)["grad"], dev)
    return _cache[name]


def _folded_launch(case, dev, W, hyper, step, gs):
    rows, F = case["rows"], case["F"]
    view = lambda t: _in(t).view(rows, F)
    _, covered = _C().hashgrid_interpolate_backward(
        dev["coords"], dev["grad_out"], (rows, F), dev["first_idx"], case["res"], case["bitwidth"], case["zero_from_col"], out=view(W["g"]),
        adamw=dict(param=view(W["p"]), exp_avg=view(W["m"]), exp_avg_sq=view(W["v"]), shadow=view(W["s"]), step=step, grad_scale=gs, **hyper))
    torch.cuda.synchronize()
    return covered


def _folded_buffers(case, shift=0):
    n = case["rows"] * case["F"]
    x = O.inputs(n, 77, "fresh")
    W = {k: _guarded(x[k], shift=shift) for k in "pmv"}
    W["g"] = _guarded(np.zeros(n, np.float32), shift=shift)
    W["s"] = _guarded(n, torch.bfloat16, shift=shift)
    return W


def _folded_step_checked(name, W, step, seeded, what, want_paths=True):
    """one launch of the backward with the step folded in; the gradient that reaches the update is exact by construction (seed +
    float64 reference, an fp32 value), so every covered row must equal the restatement fed that gradient, and every other row
    keeps its state and holds that gradient"""
    case, grad64, dev = _folded_case(name)
    gs = O.FOLDED[name][0] if name in O.FOLDED else 2.0 ** -7
    hy = O.FOLDED_HYPER
    seeds = case["seeds"] if seeded else torch.zeros_like(grad64)
    g_in = (grad64 + seeds).float().reshape(-1)
    assert torch.equal(g_in.double(), (grad64 + seeds).reshape(-1))
    _set(W["g"], seeds.float().reshape(-1).numpy())
    before = {k: _host(W[k]) for k in "pmvs"}
    g_whole = _host(W["g"])
    g_whole[GUARD:-GUARD] = g_in
    covered = _folded_launch(case, dev, W, hy, step, gs)
    paths, host_covered = O.folded_paths(case)
    assert covered == host_covered, f"{what}: the launch covers {covered}, bin_geometry says {host_covered}"
    first = case["first_idx"]
    if want_paths:
        assert set(O.FOLDED[name][1]) <= paths
        assert any(c > 0 and c >= min(int(first[l + 1] - first[l]), H.bin_geometry(case)[l]["rows"]) for l, c in enumerate(covered)), covered
    groups = O.folded_groups(case, covered)
    host = {k: before[k][GUARD:-GUARD].numpy() for k in "pmv"}
    ref = O.adamw_groups(host["p"], host["m"], host["v"], g_in.numpy(), groups, hy["beta1"], hy["beta2"], hy["eps"], step, gs, zero_grad=True)
    ctx = dict(g=g_whole, m=before["m"], v=before["v"])
    for k, nm in (("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq")):
        want = before[k].clone()
        want[GUARD:-GUARD] = torch.from_numpy(ref[k])
        _same(W[k], want, f"{what}: {nm}", ctx)
    want = g_whole.clone()
    want[GUARD:-GUARD] = torch.from_numpy(ref["g"])                    # covered rows leave a zero, the others hold the exact gradient
    _same(W["g"], want, f"{what}: gradient left in `out`", ctx)
    want = before["s"].clone()
    for (b, ln, *_), sh in zip(groups, ref["shadows"]):
        want[GUARD + b:GUARD + b + ln] = sh
    _same(W["s"], want, f"{what}: bf16 shadow", ctx)
    return covered


@pytest.mark.parametrize("name", sorted(O.FOLDED))
def test_folded_adamw_equals_the_restatement_on_exact_gradients(name):
    """two steps from the kernel's own state: step 1 into a zero `out`, step 2 onto the integer seeds"""
    W = _folded_buffers(_folded_case(name)[0])
    for step, seeded in ((1, False), (2, True)):
        _folded_step_checked(name, W, step, seeded, f"{name}, step {step}, {'seeded' if seeded else 'zero'} out")


@pytest.mark.parametrize("name", ["adam dense one owner f32 F2 2d n5000", "adam hashed one owner f32 F2 2d n5000"])
def test_folded_adamw_with_oddly_aligned_tensors(name):
    """param, moments and `out` 4 bytes off an 8-byte boundary: the element-by-element fallback of the strip flush (dense level) and
    of the slice flush (hashed level) instead of the float2 pair path"""
    W = _folded_buffers(_folded_case(name)[0], shift=1)
    assert all(_in(W[k]).data_ptr() % 8 == 4 for k in "pmvg")
    _folded_step_checked(name, W, 1, False, f"{name}, tensors 4 bytes off an 8-byte boundary")


@pytest.mark.parametrize("name", O.FOLDED_NOT_FUSED)
def test_wide_feature_tables_are_left_to_the_caller(name):
    """F = 4 and 8: no fold is compiled; nothing is covered, the state is untouched and `out` holds the exact gradient"""
    W = _folded_buffers(_folded_case(name)[0])
    covered = _folded_step_checked(name, W, 1, False, name, want_paths=False)
    assert covered == [0] * len(covered)
