"""Host checks of the exact-arithmetic decoder tests (tests/decoder_exact_ref.py): the float64 reference against fp32
autograd of the oracle's modules - exactly, because the inputs are exact -, the conditions on the pattern set, and the
generator's own exactness assertions for the cases tests/test_gpu_decoder_exact.py runs."""
import functools

import pytest
import torch

import decoder_exact_ref as R
from oracle import nerf as onerf


def _oracle_modules(case):
    H, I = case["hidden"], case["in_dim"]
    P = R.unpack(case["params"], H, I)
    dd = onerf.OracleDecoder(I, 16, H, 1, True)
    dc = onerf.OracleDecoder(R.X2, 3, H, 2, True)
    with torch.no_grad():
        for lin, w, b in ((dd.layers[0], "W1", "b1"), (dd.lout, "W2", "b2"), (dc.layers[0], "W3", "b3"), (dc.layers[1], "W4", "b4"),
                          (dc.lout, "W5", "b5")):
            lin.weight.copy_(P[w]); lin.bias.copy_(P[b])
    return dd, dc


def _autograd(case, grad_rgb):
    """nerf.py:245-264 with the oracle's modules, fp32 autograd on the CPU: (density, z, rgb, grad_feats, packed grads)"""
    dd, dc = _oracle_modules(case)
    f = case["feats"].clone().requires_grad_(True)
    dfeat = dd(f)
    fdir = torch.cat([dfeat, onerf.positional_embed(case["dirs"], 4, include_input=True)], dim=-1)
    z = dc(fdir[..., 1:])
    rgb, den = torch.sigmoid(z), torch.relu(dfeat[..., 0:1])
    ((rgb * grad_rgb).sum() + (den * case["grad_density"]).sum()).backward()
    lins = (dd.layers[0], dd.lout, dc.layers[0], dc.layers[1], dc.lout)
    packed = torch.cat([t.grad.reshape(-1) for lin in lins for t in (lin.weight, lin.bias)])
    return den.detach(), z.detach(), rgb.detach(), f.grad, packed


@pytest.mark.parametrize("in_dim", [5, 32])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("hidden,pattern", [(64, 0), (64, 5), (64, 13), (128, 7)])
def test_reference_equals_fp32_autograd_of_the_oracle_modules(hidden, pattern, mode, in_dim):
    """pins the reference's layer order, the y[0] split, the embedding columns and the packed parameter order"""
    case = R.make_case(hidden, in_dim, 517, pattern, mode)
    ref = R.run_reference(case)
    den, z, rgb, gf, gp = _autograd(case, case["grad_rgb"])
    assert torch.equal(ref["density"].float(), den)
    assert torch.equal(ref["z"].float(), z)
    assert float((ref["rgb"] - rgb.double()).abs().max()) <= 1e-7
    assert torch.equal(ref["grad_feats"].float(), gf)
    assert torch.equal(ref["grad_params"].float(), gp)
    assert float(gp.abs().max()) > 0 and float(gf.abs().max()) > 0
    if mode == "paired":
        assert float(z.abs().max()) == 0.0 and bool((rgb == 0.5).all())
    else:
        # the sigmoid's derivative, which the exact cases never exercise away from z = 0: to fp32 rounding
        g = torch.Generator().manual_seed(3)
        gr = torch.randn(517, 3, generator=g)
        soft = R.reference(case["params"], case["feats"], case["dirs"], gr, case["grad_density"], hidden, check=False)
        _, _, _, gf2, gp2 = _autograd(case, gr)
        assert float((soft["grad_params"] - gp2.double()).abs().max()) <= 1e-5 * float(gp2.abs().max())
        assert float((soft["grad_feats"] - gf2.double()).abs().max()) <= 1e-5 * float(gf2.abs().max())


def test_embedding_columns_equal_the_oracle_embedder():
    d = torch.tensor([[0.3, -0.7, 0.2], [0.0, 0.0, 0.0]], dtype=torch.float64)
    assert torch.equal(R.embed(d), onerf.positional_embed(d, R.NF, include_input=True))
    e0 = R.embed(d[1:])[0]
    assert torch.equal(e0, torch.cat([torch.zeros(3 + 3 * R.NF), torch.ones(3 * R.NF)]).double())      # exactly 0 / 1 at d = 0


def test_packed_index_names_layer_row_and_column():
    for hidden, in_dim in ((64, 5), (128, 32)):
        n = R.param_count(hidden, in_dim)
        marks = R.unpack(torch.arange(n), hidden, in_dim)
        assert R.locate(int(marks["W1"][3, 2]), hidden, in_dim) == ("W1", 3, 2)
        assert R.locate(int(marks["W3"][hidden - 1, 41]), hidden, in_dim) == ("W3", hidden - 1, 41)
        assert R.locate(int(marks["b4"][7]), hidden, in_dim) == ("b4", 7, 0)
        assert R.locate(n - 1, hidden, in_dim) == ("b5", 2, 0)


_grad_seen = {}


@functools.lru_cache(maxsize=None)
def _main_stats(hidden, mode):
    """the statistics of every main case (S = 5003, in_dim 32); also notes which elements of grad_params were ever non-zero"""
    stats = []
    for p in range(R.num_patterns(hidden)):
        out = R.run_reference(R.make_case(hidden, 32, R.S_MAIN, p, mode))
        _grad_seen[hidden] = _grad_seen.get(hidden, False) | (out["grad_params"] != 0)
        stats.append(out["stats"])
    return stats


@pytest.mark.parametrize("hidden", R.HIDDENS)
def test_pattern_set_conditions(hidden):
    n = R.num_patterns(hidden)
    for in_dim in (1, 2, 5, 32):
        seen = torch.zeros(R.param_count(hidden, in_dim), dtype=torch.bool)
        for mode in R.MODES:
            for p in range(n):
                seen |= R.make_params(hidden, in_dim, p, mode) != 0
        missing = [R.locate(int(i), hidden, in_dim) for i in torch.nonzero(~seen).flatten()[:5]]
        assert not missing, f"never non-zero over the patterns: {missing}"
        # every W1 row uses every input column over the pattern set (and in every pattern where the row is that narrow)
        used = torch.zeros(hidden, in_dim, dtype=torch.bool)
        for p in range(n):
            W1 = R.unpack(R.make_params(hidden, in_dim, p, "general"), hidden, in_dim)["W1"]
            used |= W1 != 0
            assert bool(((W1 != 0).sum(1) == min(3, in_dim)).all())
        assert bool(used.all())
    # the paired mode: mirrored units carry equal values, z = 0, and NO gradient tensor vanishes - in particular dW3 / db3 and
    # the colour chain's share of dY2 (they cancel if the paired rows of W4 read the same columns)
    assert len({tuple(R.pairing(hidden, p)[0].tolist()) for p in range(n)}) == 3
    for p in range(n):
        case = R.make_case(hidden, 32, 257, p, "paired")
        q = R.mirror_maps(hidden, 32, p)
        assert all(torch.equal(m[m], torch.arange(m.numel())) for m in q.values())
        assert int((q["h3"] != torch.arange(hidden)).sum()) == hidden
        P = R.unpack(case["params"], hidden, 32)
        assert torch.equal(P["W5"][:, q["h3"]], -P["W5"]) and not bool(P["b5"].any()) and bool((P["W5"] != 0).any(0).all())
        out = R.run_reference(case)
        G = R.unpack(out["grad_params"], hidden, 32)
        assert all(float(G[name].abs().max()) > 0 for name in R.NAMES), p
        assert float((G["W3"] != 0).double().mean()) > 0.3 and float((G["W4"] != 0).double().mean()) > 0.3
        no_colour = R.run_reference(dict(case, grad_rgb=torch.zeros_like(case["grad_rgb"])))
        assert not torch.equal(no_colour["grad_feats"], out["grad_feats"])          # the colour gradient reaches the features
    # a zero feature row (what a dead lane of a tail tile computes on) has a positive density pre-activation: a kernel that
    # lets such a lane keep its grad_density changes dW2 / db2
    # (in the patterns of the ragged shape cases, and in most of the others: S = 5003 has a tail tile too)
    def dead_lane_y0(p, in_dim):
        P = R.unpack(R.make_params(hidden, in_dim, p, "paired"), hidden, in_dim)
        h1 = torch.relu(P["b1"])
        return float((h1 @ P["W2"].T + P["b2"])[0]), float((h1 * P["W2"][0]).abs().sum())
    for p, in_dim in [(R.SHAPE_PATTERN, 32)] + [(R.WIDTH_PATTERN, w) for w in R.WIDTHS]:
        y0, reach = dead_lane_y0(p, in_dim)
        assert y0 > 0 and reach > 0
    assert sum(dead_lane_y0(p, 32)[0] > 0 for p in range(n)) >= 18


@pytest.mark.parametrize("hidden", R.HIDDENS)
def test_units_are_active_and_idle_and_the_sigmoid_is_off_saturation(hidden):
    """S = 5003, in_dim 32, every pattern.  Measured share of units both active and idle: h1 1.0; h2 / h3 >= 0.82 (paired),
    >= 0.91 (general); general mode: >= 0.44 of the |z| <= 4 (hidden 64: 0.60).  Asserted with room to spare."""
    for mode in R.MODES:
        for p, st in enumerate(_main_stats(hidden, mode)):
            for layer in ("h1", "h2", "h3"):
                assert st["both"][layer] >= 0.6, (mode, p, layer, st["both"][layer])
            assert st["max_abs"] <= 128 and st["max_sum_dy_x"] < 2.0 ** 20
            assert 0.25 <= st["density_active"] <= 0.998, (mode, p, st["density_active"])
            if mode == "general":
                assert st["z_small"] >= 0.25, (p, st["z_small"])


@pytest.mark.parametrize("hidden", R.HIDDENS)
def test_every_element_of_grad_params_is_non_zero_in_some_pattern(hidden):
    """A gradient element that is zero in every case is compared against nothing but zero: the kernel's product behind it (a
    row of a transposed weight image, a column of an accumulator) would go untested.  Over the main cases every element of
    grad_params is non-zero at least once - apart from the dW3 columns of the input and sine columns of the view embedding,
    which are exactly 0 at direction 0 (the limit of the technique).  In particular every row of dW2 / db2:
    the unpaired one of the 15 geometry features, whose colour gradient is zero, rotates with the pattern."""
    for mode in R.MODES:
        _main_stats(hidden, mode)
    seen = R.unpack(_grad_seen[hidden], hidden, 32)
    zero_embedding = torch.zeros(R.X2, dtype=torch.bool)
    zero_embedding[15:15 + 3 + 3 * R.NF] = True
    for name in R.NAMES:
        never = ~seen[name] if name != "W3" else ~seen[name] & ~zero_embedding[None, :]
        assert not bool(never.any()), (name, torch.nonzero(never)[:5].tolist())
    assert not bool(seen["W3"][:, zero_embedding].any())
    # the geometry rows of dW2 / db2 get their gradient from the colour chain alone, i.e. from the paired mode
    for p in range(R.num_patterns(hidden)):
        q = R.mirror_maps(hidden, 32, p)["y"]
        assert int((q == torch.arange(15)).sum()) == 1 and int(q[p % 15]) == p % 15


def test_generator_assertions_hold_for_the_cases_of_the_gpu_file():
    """reference() asserts the exactness conditions itself; the two largest sizes are checked once on the GPU in float64"""
    big = sorted({c[2] for c in R.gpu_cases()})[-2:]
    assert big == [70001, R.S_TWO_CHUNKS]
    for hidden in R.HIDDENS:                                  # the main cases
        for mode in R.MODES:
            assert len(_main_stats(hidden, mode)) == R.num_patterns(hidden)
    for hidden, in_dim, S, p, mode, cancel in R.gpu_cases():
        if S in big or S == R.S_MAIN:
            continue
        out = R.run_reference(R.make_case(hidden, in_dim, S, p, mode, cancel))
        assert S < 31 or out["grad_params"].abs().max() > 0


@pytest.mark.parametrize("hidden", R.HIDDENS)
def test_b2_cancel_case_needs_the_bias_before_the_bf16_pack(hidden):
    case = R.make_case(hidden, 32, R.S_CANCEL, R.SHAPE_PATTERN, "paired", b2_cancel=True)
    R.run_reference(case)                                     # y[1:16] itself is exact ...
    P = R.unpack(case["params"].double(), hidden, 32)
    pre = torch.relu(case["feats"].double() @ P["W1"].T + P["b1"]) @ P["W2"].T
    lossy = pre[:, 1:].to(torch.bfloat16).double() != pre[:, 1:]
    assert float(lossy.double().mean()) > 0.2                 # ... the value before the bias is not, on many samples
    assert bool(lossy.any(0).all())                           # in every geometry feature


def test_reference_refuses_inputs_that_are_not_exact():
    case = R.make_case(64, 32, 64, 0, "paired")
    bad = dict(case, feats=case["feats"] + 1.0 / 512)         # x + 2^-9 needs more than 8 bits
    with pytest.raises(AssertionError, match="not exact"):
        R.run_reference(bad)
    bad = dict(case, grad_rgb=case["grad_rgb"] * 2.0 ** 22)
    with pytest.raises(AssertionError, match="not exact"):
        R.run_reference(bad)
    general = R.make_case(64, 32, 64, 0, "general")
    with pytest.raises(AssertionError, match="not exact"):   # a gradient through the sigmoid away from z = 0
        R.run_reference(dict(general, grad_rgb=torch.full((64, 3), 4.0)))
