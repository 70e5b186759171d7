"""Host checks of the exact-arithmetic octree / codebook grid tests (tests/spc_exact_ref.py): the float64 reference against fp32
autograd through the oracle's lookups - exactly, because the inputs are exact -, the builder's own exactness assertions for the
cases tests/test_gpu_spc_exact.py runs, and what each sample order reaches in the merge kernel of csrc/spc_grad.hip."""
import numpy as np
import pytest
import torch

import spc_exact_ref as R
from oracle import octree_grid as og, spc as ospc


def _mtype(case):
    return "sum" if case["sum"] else "cat"


def _same(got, want):
    return all(torch.equal(a.double(), b) for a, b in zip(got, want))


@pytest.mark.parametrize("order", ["few", "many", "mixed"])
@pytest.mark.parametrize("mtype", ["sum", "cat"])
def test_reference_equals_fp32_autograd_of_the_octree_oracle(mtype, order):
    """pins the corner order, the trinket indexing, the chain columns and the 'sum' / 'cat' columns of the gradient"""
    t = R.tree()
    case = R.multi_case(order, 5, mtype == "sum")
    ref = R.reference(case)
    chain = ospc.query(t.octree, t.exsum, case["coords"].numpy(), 5, with_parents=True)
    assert np.array_equal(chain[:, list(case["levels"])], case["chain"].numpy())
    feats = [f.clone().requires_grad_(True) for f in case["feats"]]
    out = og.octree_grid_interpolate(t.oracle_blas(), t.trinkets, feats, case["coords"], 3, 2, list(case["levels"]), mtype, 5, half_round=False)
    (out * case["grad_out"]).sum().backward()
    assert torch.equal(out.detach().double(), ref["out"])
    assert _same([f.grad for f in feats], ref["grads"])
    assert all(float(g.abs().max()) > 0 for g in ref["grads"]) and float(ref["out"].abs().max()) > 0
    w = R.weights(case, 3)[0][(case["chain"][:, 3] >= 0).numpy()]
    assert max(float(g.abs().max()) for g in ref["grads"]) < 100 and float(w.max()) == 1.0 and float(w.min()) == 0.0     # offset 0 occurs


def test_reference_with_half_rounding_equals_the_oracle_on_two_levels():
    """integer features and two levels: every per-level result is an fp16 value, so the reference's half rounding changes nothing;
    with the two coarser levels it would (2^-9 / 2^-12 steps), which is why the GPU file runs fp16 on two levels only"""
    t = R.tree()
    case = R.multi_case("mixed", 5, True, levels=(4, 5))
    ref = R.reference(case)
    assert ref["half_ok"] and not R.reference(R.multi_case("mixed", 5, True))["half_ok"]
    out = og.octree_grid_interpolate(t.oracle_blas(), t.trinkets, case["feats"], case["coords"], 1, 4, [4, 5], "sum", 5, half_round=True)
    assert torch.equal(out.double(), ref["out"])


@pytest.mark.parametrize("S", [1, 4, 16])
def test_leaf_reference_equals_fp32_autograd_of_interpolate_trilinear(S):
    t = R.tree()
    case = R.leaf_case(5, S, 5)
    ref = R.reference(case)
    V = case["N"] // S
    pidx = case["chain"][::S, 0]
    assert int((pidx < 0).sum()) > 0
    f = case["feats"][0].clone().requires_grad_(True)
    out = og.interpolate_trilinear(case["coords"].view(V, S, 3), pidx, t.points, t.trinkets, f, 5)
    (out * case["grad_out"].view(V, S, 5)).sum().backward()
    assert torch.equal(out.detach().double().view(-1, 5), ref["out"]) and torch.equal(f.grad.double(), ref["grads"][0])
    assert ref["half_ok"]
    assert torch.equal(og.interpolate_trilinear(case["coords"].view(V, S, 3), pidx, t.points, t.trinkets, case["feats"][0], 5,
                                                half_round=True).double().view(-1, 5), ref["out"])


@pytest.mark.parametrize("K,F", [(16, 5), (8, 3)])
@pytest.mark.parametrize("mtype", ["sum", "cat"])
@pytest.mark.parametrize("mode", ["onehot", "uniform"])
def test_codebook_reference_equals_fp32_autograd_of_the_codebook_oracle(mode, mtype, K, F):
    """the straight-through softmax of codebook_grid.py:103-136 on logits that make it exact"""
    t = R.tree()
    case, cb = R.codebook_case(mode, K, F, mtype == "sum")
    ref = R.codebook_reference(case, cb)
    lg = [x.clone().requires_grad_(True) for x in cb["logits"]]
    dc = [x.clone().requires_grad_(True) for x in cb["dicts"]]
    out = og.codebook_grid_interpolate(t.oracle_blas(), t.trinkets, lg, dc, case["coords"], 3, list(case["levels"]), mtype, F, True)
    (out * case["grad_out"]).sum().backward()
    assert torch.equal(out.detach().double(), ref["out"])
    assert _same([x.grad for x in lg], ref["grad_logits"]) and _same([x.grad for x in dc], ref["grad_dicts"])
    with torch.no_grad():
        ev = og.codebook_grid_interpolate(t.oracle_blas(), t.trinkets, lg, dc, case["coords"], 3, list(case["levels"]), mtype, F, False)
    assert torch.equal(ev.double(), ref["out"])
    assert all(float(g.abs().max()) > 0 for g in ref["grad_dicts"])
    if mode == "onehot":
        assert all(float(g.abs().max()) == 0 for g in ref["grad_logits"])
        assert all(int((g.abs().sum(1) > 0).sum()) == K for g in ref["grad_dicts"][1:])          # every key is some row's
    else:
        assert all(float(g.abs().max()) > 0 for g in ref["grad_logits"])
        assert all(float(g[1:].abs().max()) == 0 for g in ref["grad_dicts"])


def test_the_builder_rejects_inexact_inputs():
    case = R.multi_case("mixed", 5, True)
    R.reference(case)
    bad = dict(case, coords=case["coords"].clone())
    valid = int(torch.nonzero(case["chain"][:, 3] >= 0)[0])
    cell = np.floor((bad["coords"][valid].numpy().astype(np.float64) * 0.5 + 0.5) * 32)
    bad["coords"][valid] = torch.from_numpy(((cell + 1.0 / 3.0) / 32 * 2 - 1).astype(np.float32))          # offset 1/3
    with pytest.raises(AssertionError, match="inputs are not exact"):
        R.reference(bad)
    bad = dict(case, grad_out=case["grad_out"].clone())
    bad["grad_out"][valid] = 0.1
    with pytest.raises(AssertionError, match="inputs are not exact|off the grid"):
        R.reference(bad)
    with pytest.raises(AssertionError, match="inputs are not exact"):
        R.make_case(R.tree(), R.cells_of("mixed"), R.LEVELS4, 5, True, scale_exp=-150)                    # below the denormals
    with pytest.raises(AssertionError, match="inputs are not exact"):
        R.reference(dict(case, grad_out=case["grad_out"] * 4096.0))                                       # sum |w g| past 2^24 quanta
    case, cb = R.codebook_case("uniform", 16, 5, True)
    cb["dicts"][0][3, 2] = 0.3
    with pytest.raises(AssertionError):
        R.codebook_reference(case, cb)


def test_every_case_of_the_gpu_file_passes_the_builders_assertions():
    """(the GPU file computes the same references; here they are known to hold without a GPU)"""
    for channels in R.MERGE_CHANNELS + R.WIDE_CHANNELS + (5,):
        for s in (True, False):
            R.reference(R.multi_case("mixed", channels, s))
    for channels in (5, 16):
        R.reference(R.multi_case("mixed", channels, channels == 5, grad="mix"))
        base = R.reference(R.multi_case("mixed", channels, True))
        for e in R.LOSS_SCALES:
            scaled = R.reference(R.multi_case("mixed", channels, True, scale_exp=e))
            assert all(torch.equal(a, b * 2.0 ** e) for a, b in zip(scaled["grads"], base["grads"]))
        for levels in ((5,), (4, 5), (3, 4, 5)):
            R.reference(R.multi_case("mixed", channels, False, levels=levels))
        for S in (1, 4, 16):
            assert R.reference(R.leaf_case(5, S, channels))["half_ok"]
        for n in R.SMALL_N:
            R.reference(R.truncated(R.multi_case("mixed", channels, True), n))
    R.reference(R.multi_case("mixed", 16, True, n=R.N_SPLIT_BIG))
    for channels, n in ((5, 4500), (72, R.N_MAIN)):
        for levels in (R.LEVELS4, (4, 5)):
            for s in (True, False):
                assert R.reference(R.multi_case("mixed", channels, s, levels, n=n))["half_ok"] == (len(levels) == 2)
    for mode in ("onehot", "uniform"):
        for K, F in ((16, 5), (8, 3)):
            for level, S, V in ((5, 4, 600), (3, 4, 800)):
                R.codebook_reference(*R.codebook_leaf_case(mode, K, F, level, S, V))


def test_the_smallest_scale_has_a_denormal_maximum_and_the_largest_case_selects_the_float_path():
    case = R.multi_case("mixed", 5, True, scale_exp=-130)
    assert 0 < float(case["grad_out"].abs().max()) < 2.0 ** -126                   # denormal: the exponent field of M is 0
    ref = R.reference(case)
    assert min(float(g[g != 0].abs().min()) for g in ref["grads"]) >= 2.0 ** -142
    for channels in (5, 16):
        case = R.huge_case(channels)
        ref = R.reference(case)
        w = R.weights(case, 3)[0][(case["grad_out"] != 0).any(1).numpy() & (case["chain"][:, 3] >= 0).numpy()]
        assert float(w.max()) == 1.0                                                # offset 0 present: M = 2^121, exponent field 0xf8
        assert R.max_adds_per_row(case) <= R.HUGE_ADDS and max(float(a.max()) for a in ref["abs_sums"]) < 2.0 ** 127
        assert int((case["grad_out"] != 0).any(1).sum()) > 128                      # more than one block of live samples


# ---------------------------------------------------------------------------------------------------- what the orders reach
def _reports(order, levels=R.LEVELS4):
    case = R.multi_case(order, 5, True, levels)
    return case, R.report(R.tree(), case["chain"].numpy())


def test_the_long_run_orders_never_link_and_the_walk_does():
    for order in ("few",):
        _, rep = _reports(order)
        assert all(int(r["tails_per_wave"].max()) <= R.LINK_TAILS for r in rep)
        assert all(r["cross_row"] > 50 and r["cross_wave"] > 5 and r["cross_block"] > 5 for r in rep)
    case, rep = _reports("many")
    fine = rep[-1]
    assert float((fine["tails_per_wave"] > R.LINK_TAILS).mean()) > 0.9 and fine["shared4"] > 500 and fine["shared8"] > 50
    assert any(int(r["tails_per_wave"].min()) <= R.LINK_TAILS for r in rep)          # coarse levels: both modes in one launch
    regrouped = R.report(R.tree(), R.permuted(case, R.regroup(R.tree(), 5, R.cells_of("many")))["chain"].numpy())
    assert all(int(r["tails_per_wave"].max()) <= R.LINK_TAILS for r in regrouped)


def test_the_mixed_order_reaches_what_it_claims():
    case, rep = _reports("mixed")
    fine = rep[-1]
    assert int(fine["tails_per_wave"].max()) > R.LINK_TAILS and int(fine["tails_per_wave"].min()) <= R.LINK_TAILS
    assert fine["cross_row"] > 50 and fine["cross_wave"] > 5 and fine["cross_block"] > 5 and fine["miss_inside"] > 10
    assert fine["shared8"] > 0                                                       # a run cut by a row boundary, in links mode
    chain = case["chain"].numpy()
    assert int(((chain[:, 3] < 0) & (chain[:, 2] >= 0)).sum()) > 5                    # no finest cell, cells above it
    assert int((chain < 0).all(1).sum()) > 10
    # the first 129 samples: a run across lane 63 and one across sample 128
    first = R.report(R.tree(), chain[:129])[-1]
    assert first["cross_wave"] == 1 and first["cross_block"] == 1


def test_touched_rows_get_a_gradient_or_the_reason_is_known():
    """over the three orders: a touched row without a gradient was reached with zero weights or zero gradients only (abs sum 0)
    or its contributions cancelled - the latter is what cancel_case is for"""
    t = R.tree()
    touched = [torch.zeros(t.rows(l), dtype=torch.bool) for l in R.LEVELS4]
    live = [torch.zeros(t.rows(l), dtype=torch.bool) for l in R.LEVELS4]
    for order in ("few", "many", "mixed"):
        ref = R.reference(R.multi_case(order, 5, True))
        for li in range(4):
            touched[li] |= ref["touched"][li]
            live[li] |= (ref["grads"][li] != 0).any(1)
            silent = ref["touched"][li] & ~(ref["grads"][li] != 0).any(1)
            zero_in = (ref["abs_sums"][li].sum(1) == 0)
            assert bool((silent <= (zero_in | R.cancelled_rows(ref)[li])).all())
    for li in range(4):
        assert float((live[li] & touched[li]).sum()) >= 0.9 * float(touched[li].sum())
    ref = R.reference(R.cancel_case(5))
    gone = R.cancelled_rows(ref)
    assert all(int(m.sum()) > 0 for m in gone) and all(float(g.abs().max()) > 0 for g in ref["grads"])
