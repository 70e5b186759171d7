"""Host checks of the rounding-faithful optimizer tests (tests/optim_exact_ref.py): the fp32 restatement of wisp_adamw_update against
the same formula in exact rationals with one rounding per operation, the exact fma against the rational fma on adversarial
triples, the C library's powf against the exact power, the three formulas against torch.optim in float64; that the inputs of
tests/test_gpu_optim_exact.py reach the regimes they are there for; and that the checks can fail: every mutant of the restatement
changes bits, every legal contraction of kinds 1 and 2 stays inside the running bound and every formula mutant leaves it."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import hashgrid_exact_ref as H
import optim_exact_ref as O

F32 = np.float32
FLAT_RUNS = [(step, gs) for step in (1,) + O.MID_STEPS for gs in O.GRAD_SCALES]              # (first step, grad_scale) of the GPU file


def _frac(x):
    return Fraction(float(x))


# ---------------------------------------------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("hyper", sorted(O.HYPER))
def test_restatement_equals_one_rounding_per_operation_in_rationals(hyper):
    """350 elements per (start, grad_scale): values compared as rationals (a zero's sign is numpy's own IEEE arithmetic)"""
    h = O.HYPER[hyper]
    for step, gs in FLAT_RUNS:
        x = O.start_state(350, step)
        bc1, bc2 = O.bias_corrections(h["beta1"], h["beta2"], step)
        g = x["g"] * F32(gs)
        p, m, v = O.adamw_update(x["p"], x["m"], x["v"], g, h["lr"], h["wd"], h["beta1"], h["beta2"], h["eps"], bc1, bc2)
        for i in range(350):
            want = O.adamw_update_fraction(x["p"][i], x["m"][i], x["v"][i], g[i], h["lr"], h["wd"], h["beta1"], h["beta2"], h["eps"], bc1, bc2)
            assert (_frac(p[i]), _frac(m[i]), _frac(v[i])) == want, (hyper, step, gs, i, float(x["g"][i]), float(x["m"][i]), float(x["v"][i]))
        assert np.any((v != 0) & (np.abs(v) < F32(O.MIN_NORMAL))) and np.any((v == 0) & (g != 0))


def _fma_triples():
    rng = np.random.default_rng(11)
    a = (rng.standard_normal(400) * 2.0 ** rng.integers(-40, 40, 400)).astype(F32)
    b = (rng.standard_normal(400) * 2.0 ** rng.integers(-40, 40, 400)).astype(F32)
    prod = a * b
    out = [(a, b, -prod), (a, b, np.nextafter(-prod, F32(np.inf))), (a, b, np.nextafter(-prod, F32(-np.inf)))]   # cancel to the last bit
    # the float64 sum is a tie: the lowest set bit j of the 48-bit product is half an ulp of 2^(j + 53) + product
    ia, ib = rng.integers(2 ** 23, 2 ** 24, 400) | 1, rng.integers(2 ** 23, 2 ** 24, 400) | 1
    j = np.array([int(x * y & -(x * y)).bit_length() - 1 for x, y in zip(ia.tolist(), ib.tolist())])
    c = (2.0 ** (j + 53)).astype(F32)
    out += [(ia.astype(F32), ib.astype(F32), c), (ia.astype(F32), ib.astype(F32), -c)]
    # the exact sum lies 2 i^2 under a tie of fp32 whose even neighbour is the upper one; float64 rounds it onto the tie
    i = np.arange(1, 301)
    near = ((2 ** 23 + i).astype(F32), (2 ** 24 - 2 * i).astype(F32), np.full(300, 2.0 ** 71 + 2.0 ** 48, dtype=F32))
    out += [near, (near[0], -near[1], -near[2])]
    # denormal results and products far under the addend
    out.append((a * F32(2.0 ** -60), b * F32(2.0 ** -60), (rng.standard_normal(400) * 2.0 ** -140).astype(F32)))
    return out, near


def test_fma_emulation_equals_the_rational_fma_on_adversarial_triples():
    triples, near = _fma_triples()
    for a, b, c in triples:
        got = O.fma32(a, b, c)
        for k in range(a.size):
            assert _frac(got[k]) == O.round32(_frac(a[k]) * _frac(b[k]) + _frac(c[k])), (float(a[k]), float(b[k]), float(c[k]), float(got[k]))
    assert np.array_equal(O.fma32(*near), near[2])                                   # rounds down, onto the addend
    assert np.any(O.fma32_twice_rounded(*near) != near[2])                           # product + add + cast does not qualify
    assert O.fma32(F32(3.0), F32(0.5), F32(0.25)) == F32(1.75)                       # scalars


def test_the_c_librarys_powf_is_within_one_ulp_of_the_exact_power():
    for beta in (0.85, 0.9, 0.99, 0.999):
        b = _frac(F32(beta))
        for step in range(1, 401):
            got, exact = _frac(O.powf(beta, step)), b ** step
            assert abs(got - exact) <= _frac(np.spacing(F32(float(got)))), (beta, step)
    bc1, bc2 = O.bias_corrections(0.9, 0.999, 30000)
    assert bc1 == F32(1.0) and bc2 == F32(1.0)                                       # late steps: the corrections are exactly 1


def test_float64_formulas_equal_torch_optim():
    """five steps of torch.optim.AdamW, Adam (L2 decay) and RMSprop (with and without momentum) in float64, to 1e-12 relative"""
    n, lr, wd = 300, 1e-2, 1e-2
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n) for _ in range(5)]

    def run_torch(opt_cls, **kw):
        t = torch.from_numpy(p0.copy()).requires_grad_(True)
        opt = opt_cls([t], lr=lr, weight_decay=wd, **kw)
        for g in grads:
            t.grad = torch.from_numpy(g.copy())
            opt.step()
        return t.detach().numpy()

    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for k, g in enumerate(grads):
        p, m, v = O.adamw_update_f64(p, m, v, g, lr, wd, 0.9, 0.999, 1e-8, k + 1)
    close(p, run_torch(torch.optim.AdamW, betas=(0.9, 0.999), eps=1e-8))
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for k, g in enumerate(grads):
        bc1, bc2 = 1.0 - 0.9 ** (k + 1), np.sqrt(1.0 - 0.999 ** (k + 1))
        p, m, v = (t.v for t in O.kind_update_bounded("adam", p, m, v, g, lr, wd, 0.9, 0.999, 1e-8, bc1, bc2, 1.0))
    close(p, run_torch(torch.optim.Adam, betas=(0.9, 0.999), eps=1e-8))
    for mom in (0.0, 0.9):
        p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
        for g in grads:
            tp, t1, t2 = O.kind_update_bounded("rmsprop", p, m, v, g, lr, wd, 0.99, mom, 1e-8, 1.0, 1.0, 1.0)
            p, m, v = tp.v, (t1.v if t1 is not None else m), t2.v
        close(p, run_torch(torch.optim.RMSprop, alpha=0.99, momentum=mom, eps=1e-8))


# ---------------------------------------------------------------------------------------------------- the inputs reach the regimes
def _relied(h):
    return ("denormal_v", "v_zero_g_nonzero", "eps_decides", "eps_invisible", "shadow_ties", "decay_only" if h["wd"] > 0 else "unchanged")


@pytest.mark.parametrize("n", [1023, 1025, 65539])
@pytest.mark.parametrize("hyper", sorted(O.HYPER))
def test_flat_inputs_reach_every_regime_the_gpu_tests_rely_on(hyper, n):
    """at least 1 % of the elements each, for every start the GPU file runs and through steps 2 and 3 of the restatement's own
    trajectory: a condition on the seeds, asserted.  (Sizes 1 to 5 are there for the kernels' edges, not for the regimes.)"""
    h = O.HYPER[hyper]
    decay = O.ONE - F32(h["lr"]) * F32(h["wd"])
    for step, gs in FLAT_RUNS:
        x = O.start_state(n, step, decay)
        for s in (O.FRESH_STEPS if step == 1 else (step,)):
            g = x["g"] if s == step else O.step_gradient(n, s)
            shares = O.reaches(dict(x, g=g, **h, step=s, grad_scale=gs))
            for k in _relied(h):
                if k == "shadow_ties" and s != step:
                    continue                                             # (planted for the first step of a run)
                assert shares[k] >= 0.01, (hyper, n, s, gs, k, shares)
            out = O.adamw_step(x["p"], x["m"], x["v"], g, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], s, gs)
            x = dict(x, p=out["p"], m=out["m"], v=out["v"])


def test_wrap_buffer_and_group_layouts():
    """the big buffer takes the grid-stride loop twice (more than 4096 x 256 chunks of 4) and ends ragged; group begins cover 0, 1, 2
    and 3 mod 4 plus the 8-byte path, lengths are no multiples of 4, five groups split over two launches, four fit one"""
    assert O.WRAP_N > 4096 * 256 * 4 and (O.WRAP_N - 4096 * 256 * 4) // 4 == 256 and O.WRAP_N % 4 == 3
    for n in (1023, 1025, 65539):
        g5 = O.group_layout(n, 5, (0, 1, 2, 3, 2), (0.0, 1e-2))
        assert [b % 4 for b, *_ in g5] == [0, 1, 2, 3, 2] and all(ln % 4 for _, ln, *_ in g5) and g5[-1][0] + g5[-1][1] <= n
        g4 = O.group_layout(n, 4, (0, 0, 0, 0), (0.0, 1e-2))
        assert all(b % 4 == 0 for b, *_ in g4) and len(g4) == 4
    size, groups = O.wrap_layout(5, (1e-6,))
    assert groups[0][1] == O.WRAP_N and [b % 4 for b, *_ in groups] == [0, 1, 2, 3, 2] and groups[-1][0] + groups[-1][1] < size
    h = O.HYPER["hash"]
    x = O.start_state(O.WRAP_N, 1000, O.ONE - F32(h["lr"]) * F32(h["wd"]))
    shares = O.reaches(dict(x, **h, step=1000, grad_scale=1.0 / 128.0))
    assert all(shares[k] >= 0.01 for k in _relied(h)), shares


# ---------------------------------------------------------------------------------------------------- the checks can fail
def _differs(a, b):
    return any(not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in "pmv")


def _concerns(mutant, h, step, gs):
    if mutant == "coupled_decay":
        return h["wd"] > 0
    if mutant == "bc2_no_sqrt":
        return O.bias_corrections(h["beta1"], h["beta2"], step)[1] != F32(1.0)       # (step 30000: the correction is exactly 1)
    if mutant == "unfused_moments":
        # a fresh m = v = 0 fuses to the same bits; and a gradient scaled by 2^-30 onto a mid-training state of the unscaled
        # gradient's size lies under half an ulp of beta * state: both forms round to the same neighbour
        return step != 1 and not (step in O.MID_STEPS and gs == 2.0 ** -30)
    return True


@pytest.mark.parametrize("mutant", O.MUTANTS + ("shadow_trunc",))
def test_every_mutant_of_the_restatement_changes_bits(mutant):
    """eps inside the square root, coupled decay, bc2 without its root, unfused moment fmas, a flushed denormal v, a reciprocal in
    place of the division, a truncated shadow: each differs from the restatement in at least one output of every run it concerns"""
    seen = 0
    for hyper, h in O.HYPER.items():
        for step, gs in FLAT_RUNS:
            x = O.start_state(1025, step, O.ONE - F32(h["lr"]) * F32(h["wd"]))
            for s in (O.FRESH_STEPS if step == 1 else (step,)):
                g = x["g"] if s == step else O.step_gradient(1025, s)
                args = (x["p"], x["m"], x["v"], g, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], s, gs)
                good = O.adamw_step(*args, shadow=True)
                if mutant == "shadow_trunc":
                    assert not torch.equal(good["shadow"], O.shadow_of(good["p"], truncate=True))
                    seen += 1
                elif _concerns(mutant, h, s, gs):
                    bad = O.adamw_step(*args, mutant=mutant)
                    assert _differs(good, bad), (mutant, hyper, s, gs)
                    seen += 1
                x = dict(x, p=good["p"], m=good["m"], v=good["v"])
    assert seen >= 9


KIND_CASES = [(kind, k, step) for kind in ("adam", "rmsprop") for k in (0, 1) for step in (1, 1000)]
# share of the elements on which a formula mutant leaves the running bound in at least one output: the measured minimum over the
# KIND_CASES the mutant concerns, cut to two digits (the inputs are seeded: the shares do not vary)
MUTANT_SHARES = {("adam", "eps_in_sqrt"): 0.63, ("adam", "decoupled_decay"): 0.75, ("adam", "bc2_no_sqrt"): 0.91,
                 ("rmsprop", "eps_in_sqrt"): 0.25, ("rmsprop", "decoupled_decay"): 0.87}


def _kind_case(kind, k, step, n=1025):
    hy = O.KIND_HYPER[kind][k]
    x = O.start_state(n, step)
    s1 = x["m"] if (kind == "adam" or hy["h1"] > 0) else None
    bound = O.bounded_groups(kind, x["p"], s1, x["v"], x["g"], [(0, n, 1e-2, hy["wd"], None)], hy["h0"], hy["h1"], hy["eps"], step, 1.0 / 128.0)
    bc1, bc2 = O.kind_scalars(kind, hy["h0"], hy["h1"], step)
    args = (kind, x["p"], s1, x["v"], x["g"], 1e-2, hy["wd"], hy["h0"], hy["h1"], hy["eps"], bc1, bc2, 1.0 / 128.0)
    return hy, bound, args


def _outside(bound, got):
    out = np.zeros(bound["p"][0].size, dtype=bool)
    for k, a in zip(("p", "s1", "s2"), got):
        if a is not None and bound[k] is not None:
            out |= np.abs(a.astype(np.float64) - bound[k][0]) > bound[k][1]
    return out


@pytest.mark.parametrize("kind,k,step", KIND_CASES)
def test_every_legal_contraction_of_adam_and_rmsprop_stays_inside_the_running_bound(kind, k, step):
    """every fma / no-fma choice of the sums (either product of a two-product sum may be the fused one): 54 variants of Adam, 36 of
    RMSprop.  The bound is not slack either: some variant uses more than half of it."""
    hy, bound, args = _kind_case(kind, k, step)
    worst = 0.0
    for choice in itertools.product(*(range(c) for c in O.KIND_CHOICES[kind])):
        got = O.kind_update_f32(*args, choice=choice)
        bad = _outside(bound, got)
        assert not bad.any(), (kind, hy, step, choice, int(bad.sum()), int(np.flatnonzero(bad)[0]))
        used = np.abs(got[0].astype(np.float64) - bound["p"][0]) / np.maximum(bound["p"][1], 1e-300)
        worst = max(worst, float(used.max()))
    assert 0.5 < worst <= 1.0, worst


@pytest.mark.parametrize("kind,mutant", sorted(MUTANT_SHARES))
def test_formula_mutants_of_adam_and_rmsprop_leave_the_running_bound(kind, mutant):
    """measured shares of the 1025 elements outside the bound, per (hyper-parameter set, start) of KIND_CASES the mutant concerns:
    adam eps_in_sqrt 0.741, 0.636, 0.813, 0.730; adam decoupled_decay 0.810, 0.754, 1.0, 1.0; adam bc2_no_sqrt 1.0, 1.0, 1.0, 0.919;
    rmsprop eps_in_sqrt 0.357, 0.254, 0.821, 0.740; rmsprop decoupled_decay 0.999, 0.876.  Asserted at their minimum (MUTANT_SHARES)."""
    shares = []
    for kd, k, step in KIND_CASES:
        hy, bound, args = _kind_case(kd, k, step)
        if kd != kind or (mutant == "decoupled_decay" and hy["wd"] == 0) or (mutant == "bc2_no_sqrt" and args[-2] == F32(1.0)):
            continue
        shares.append(float(_outside(bound, O.kind_update_f32(*args, mutant=mutant)).mean()))
    print(kind, mutant, "shares outside the bound:", shares)
    assert shares and min(shares) >= MUTANT_SHARES[(kind, mutant)], f"{kind} {mutant}: shares outside the bound {shares}"


# ---------------------------------------------------------------------------------------------------- the folded step's cases
@pytest.mark.parametrize("name", sorted(O.FOLDED))
def test_folded_cases_reach_their_paths(name):
    """bin_geometry / reaches of the hash-grid cases the folded-AdamW test runs: claims hold, the gradient is exact, the paths the
    test is there for are reached and at least one level is covered whole"""
    case = H.bwd_case(name)
    assert set(case["claims"]) <= H.reaches(case), (case["claims"], H.reaches(case))
    H.reference_backward(case)
    paths, covered = O.folded_paths(case)
    assert set(O.FOLDED[name][1]) <= paths, (paths, covered)
    first = case["first_idx"]
    assert any(c > 0 and c >= min(int(first[l + 1] - first[l]), H.bin_geometry(case)[l]["rows"]) for l, c in enumerate(covered)), covered
    gs = O.FOLDED[name][0]
    assert np.log2(gs) == int(np.log2(gs))


def test_wide_feature_cases_are_not_folded():
    for name in O.FOLDED_NOT_FUSED:
        assert O.folded_paths(H.bwd_case(name)) == (set(), [0] * H.bwd_case(name)["L"])
