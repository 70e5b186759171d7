"""CPU: the float64 restatement of the two fused octree SDF steps (tests/sdf_step_exact_ref.py) pinned bit for bit to torch autograd
through oracle.octree_grid.octree_grid_interpolate and the oracle's decoder on the exact cases, the gradient at a == 0 pinned to
torch.relu's, and the coverage the GPU file (tests/test_gpu_sdf_step_exact.py) claims: every gradient element live in some pattern,
samples on the relu edge, the share of zero results, and which (levels, n) pairs reach a tail pass, idle lane groups or a second
grid-stride pass."""
import numpy as np
import pytest
import torch

import sdf_step_exact_ref as X
from oracle import spc as ospc

ST_GROUPS = 16                 # csrc/spc_grad.hip: lane groups per workgroup, one per (sample, level) of a pass
GRID_CAP = 1024                # csrc/spc_grad.hip st_grid: workgroups at most
OUT = ("loss", "w1", "b1", "w2", "b2")


def _equal(want, got, dtype, what, half_round=False):
    """half_round: the oracle's feats.half() sends the table gradient back through fp16 (the cast's backward), which the kernels do
    not do: the tables are compared after that same rounding"""
    for k in OUT:
        assert torch.equal(want[k].reshape(-1), got[k].double().reshape(-1)), (what, k)
    for li, (a, b) in enumerate(zip(want["tables"], got["tables"])):
        assert torch.equal(a.float().half().double() if half_round else a, b.double()), (what, "table", li)
    assert torch.equal(want["pred"], got["pred"].double()), (what, "pred")


PIN = [dict(tex=False, pos_input=1, half_round=False), dict(tex=False, pos_input=1, half_round=True),
       dict(tex=True, pos_input=1, half_round=False), dict(tex=True, pos_input=0, half_round=False),
       dict(tex=True, pos_input=1, half_round=True), dict(tex=True, pos_input=0, half_round=True)]


@pytest.mark.parametrize("kw", PIN, ids=lambda k: "-".join(f"{a}{int(b)}" for a, b in k.items()))
@pytest.mark.parametrize("tree,levels,n,hidden", [("small", (3, 4, 5), 64, 24), ("small", (1, 3, 5), 16, 17), ("deep", (2, 5, 9), 64, 16)])
def test_restatement_equals_autograd_through_the_oracle_bit_for_bit(tree, levels, n, hidden, kw):
    """float64 and fp32 autograd; the exact cases have no rounding anywhere, so both must give the restatement's bits.  The chain of
    the case (spc_exact_ref.make_case) is the oracle's query as well."""
    case = X.exact_case(tree, levels, n, hidden, **kw)
    tr = case["tree"]
    chain = ospc.query(tr.octree, tr.exsum, case["coords"].numpy(), levels[-1], with_parents=True)
    assert np.array_equal(chain[:, list(levels)], case["chain"].numpy())
    assert case["report"]["edge"] >= 1 and case["report"]["relu_both"]
    for dtype in (torch.float64, torch.float32):
        _equal(case["want"], X.autograd_reference(case, dtype), dtype, (dtype, kw), kw["half_round"])


@pytest.mark.parametrize("modes", [("low", "low", "low"), ("high", "high", "high"), ("low", "half", "high")])
def test_saturated_colour_modes_equal_fp32_autograd(modes):
    """b2 = -128 / +128: fp32 expf is exactly +inf / 0, the colour exactly 0 / 1 and its gradient exactly 0 - in fp32 autograd as in the
    kernel (float64 keeps 2.6e-56 of the colour, so only the fp32 pin holds bit for bit here)"""
    case = X.exact_case("small", (3, 4, 5), 64, 24, tex=True, modes=modes)
    got = X.autograd_reference(case, torch.float32)
    _equal(case["want"], got, torch.float32, modes)
    for o, m in enumerate(modes):
        assert bool((case["want"]["w2"][o] != 0).any()) == (m == "half") and (m == "half" or float(case["want"]["b2"][o]) == 0.0)
    assert float(case["want"]["loss"][2]) > 0


def test_gradient_at_zero_preactivation_is_relus_zero():
    x = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    torch.relu(x).sum().backward()
    assert torch.equal(x.grad, torch.zeros(3, dtype=torch.float64))
    case = X.exact_case("small", (3, 4, 5), 64, 24)
    p = X.decoder_parts(case)
    on_edge = (p["a"] == 0) & (p["gh"].abs().sum(1) != 0)
    assert int(on_edge.sum()) == case["report"]["edge"] >= 1
    assert bool((p["ga"][on_edge] == 0).all())
    # a kernel that let the edge through (a >= 0) would change d b1 of the edge unit
    leaked = torch.where(p["a"] >= 0, p["gh"].sum(1), torch.zeros_like(p["a"])).sum(0)
    assert not torch.equal(leaked, case["want"]["b1"])


@pytest.mark.parametrize("tex", [False, True])
def test_every_decoder_gradient_element_is_live_in_some_pattern(tex):
    hidden = 128
    live = None
    for pattern in range(X.n_patterns(hidden, tex)):
        case = X.exact_case("small", (3, 4, 5), 64, hidden, tex=tex, pattern=pattern)
        now = {k: case["want"][k] != 0 for k in ("w1", "b1", "w2", "b2")}
        live = now if live is None else {k: live[k] | now[k] for k in now}
    for k, v in live.items():
        assert bool(v.all()), (k, int((~v).sum()))


def test_zero_results_stay_under_the_caps():
    for tree, levels in X.LEVEL_LISTS:
        for n in (16, 512):
            rep = X.exact_case(tree, levels, n, 16)["report"]
            assert rep["table_zero"] <= 0.15 * rep["table_touched"] and rep["dec_zero"] <= 0.15 * rep["dec_live"], (levels, n, rep)
            assert rep["edge"] >= 1 and 2 * rep["nonzero_diff"] >= n


def _shape(num_lods, n):
    spb = ST_GROUPS // num_lods
    grid = min(-(-n // spb), GRID_CAP)
    passes = [len(range(b * spb, n, grid * spb)) for b in range(grid)]
    return spb, ST_GROUPS - spb * num_lods, n % spb != 0, min(passes), max(passes)


def test_what_the_level_lists_and_batch_sizes_reach():
    assert X.ST_GROUPS == ST_GROUPS and X.GRID_CAP == GRID_CAP
    spbs = sorted({_shape(len(l), 1)[0] for _, l in X.LEVEL_LISTS})
    assert spbs == [1, 2, 3, 4, 5, 8, 16]
    idle = {len(l): _shape(len(l), 1)[1] for _, l in X.LEVEL_LISTS}
    assert idle == {1: 0, 2: 0, 3: 1, 4: 0, 5: 1, 6: 4, 8: 0, 9: 7}
    # a tail pass (s >= n inside a pass): n = 1, 2 wherever spb > n; 16 / 64 / 512 at 3 and 5 levels (spb 5 and 3)
    for num_lods, n, tail in ((1, 1, True), (1, 16, False), (3, 16, True), (3, 64, True), (3, 512, True), (5, 16, True), (5, 512, True),
                              (6, 1, True), (6, 2, False), (9, 1, False), (4, 2, True), (4, 512, False)):
        assert _shape(num_lods, n)[2] == tail, (num_lods, n)
    for (tree, levels, n), (lo, hi) in zip(X.BIG, ((2, 2), (1, 2))):       # every workgroup two passes; some two, some one
        s = _shape(len(levels), n)
        assert (s[3], s[4]) == (lo, hi), (levels, n, s)
        d = X.launch_shape(len(levels), n)
        assert d["second_pass_all"] == (lo == 2) and d["second_pass_some"] == (lo == 1)
    for _, levels in X.LEVEL_LISTS:
        for n in X.NS + X.INEXACT_NS:
            assert _shape(len(levels), n)[4] == 1 or len(levels) >= 9      # below the cap nothing strides; 9 levels: 512 / 1 <= 1024 too
    assert _shape(9, 512)[4] == 1 and _shape(6, 2049)[4] == 2 and _shape(6, 2049)[3] == 1


def test_half_round_cases_differ_without_the_input_rounding():
    case = X.exact_case("small", (3, 4, 5), 64, 16, half_round=True)
    feat, _ = X.features(case)
    unrounded = dict(case, tables=[t.clone() for t in case["tables"]], half_round=False)
    plain, _ = X.features(unrounded)
    assert not torch.equal(feat, plain)
    assert all(torch.equal(t.half().float().round(), t.half().float()) for t in case["tables"])


def test_family_b_bounds_are_positive_where_a_term_exists_and_zero_elsewhere():
    case = X.inexact_case(X.exact_case("small", (3, 4, 5), 64, 16), 37)
    before = dict(tables=[torch.full(t.shape, 0.5) for t in case["tables"]], **{k: torch.full(case[k].shape, 0.5) for k in ("w1", "b1", "w2", "b2")})
    bounds = X.derived_bounds(case, before)
    for k in ("w1", "b1", "w2", "b2"):
        assert bounds[k].shape == case[k].shape and bool((bounds[k] > 0).all()) and float(bounds[k].max()) < 1e-4
    p = X.decoder_parts(case)
    w, rows, valid = p["parts"][0]
    untouched = torch.ones(case["tables"][0].shape[0], dtype=torch.bool)
    untouched[rows[valid].reshape(-1)] = False
    assert bool(untouched.any()) and float(bounds["tables"][0][untouched].max()) <= 2 * 2.0 ** -24 * 0.5
