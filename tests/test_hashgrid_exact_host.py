"""Host checks of the exact-arithmetic hash-grid tests (tests/hashgrid_exact_ref.py): the float64 reference against the oracle's
fp32 arithmetic - exactly, because the inputs are exact -, the builder's refusal of each kind of inexact input, its assertions and
the cancellation cap for every case tests/test_gpu_hashgrid_exact.py runs, and what each case reaches."""
import numpy as np
import pytest
import torch

import hashgrid_exact_ref as R
from oracle import hashgrid as ohash


def _oracle_args(case):
    return case["first_idx"], case["res"], case["bitwidth"]


@pytest.mark.parametrize("dim,dtype,F", [(3, "f32", 2), (3, "bf16", 4), (2, "f16", 2), (2, "f32", 8)])
def test_reference_equals_the_oracle_forward_and_backward(dim, dtype, F):
    """pins the corner order, the level columns and the table layout; fp32 accumulation of the oracle is exact on these inputs"""
    case = R.fwd_case(dtype, F, dim, 5)
    td = R.DTYPES[dtype]
    want = ohash.hashgrid_forward(case["coords"], case["table"].float().to(td), *_oracle_args(case))
    got = R.reference_forward(case)
    assert got.dtype == td and torch.equal(got, want) and float(got.float().abs().max()) > 0
    ref = R.reference_backward(case)
    grad = ohash.hashgrid_backward(case["coords"], case["grad_out"].float(), (case["rows"], F), *_oracle_args(case), accum_dtype=torch.float32)
    assert torch.equal(grad.double(), ref["grad"]) and float(grad.abs().max()) > 0
    w = R.level_weights(case, case["L"] - 1)[0]
    assert float(w.max()) == 1.0 and float(w.min()) == 0.0            # offset 0 occurs


def test_reference_models_spill_rows_as_the_oracle_does():
    """c = +1 at res >= 258: corner index `res`, weight exactly 0.  The oracle reads the next level's row (any finite row does: the
    weight is 0; rows appended behind the table stand in for the reference's read past the last level) and adds 0 to it."""
    case = R.fwd_spill_cases()[-1]
    assert "spill" in R.reaches(case) and case["res"] == [512, 1024, 512]
    td = R.DTYPES[case["dtype"]]
    padded = torch.cat([case["table"], torch.ones(2048, case["F"], dtype=torch.float64)]).float().to(td)
    want = ohash.hashgrid_forward(case["coords"], padded, *_oracle_args(case))
    assert torch.equal(R.reference_forward(case), want)
    grad = ohash.hashgrid_backward(case["coords"], case["grad_out"].float(), (case["rows"] + 2048, case["F"]), *_oracle_args(case))
    assert int(grad[case["rows"]:].count_nonzero()) == 0
    assert torch.equal(grad[:case["rows"]].double(), R.reference_backward(case)["grad"])


@pytest.mark.parametrize("dtype", R.FWD_DTYPES)
def test_reference_equals_the_oracle_grad_coords(dtype):
    for n, dim in ((257, 3), (65, 2)):
        case = R.grad_coords_case(dtype, 4, n, dim)
        td = R.DTYPES[dtype]
        want = ohash.hashgrid_grad_coords(case["coords"], case["grad_out"].float().to(td), case["table"].float().to(td), *_oracle_args(case))
        got = R.reference_grad_coords(case)
        assert torch.equal(got, want) and (float(got.abs().max()) > 0) == (dim == 3)


@pytest.mark.parametrize("probe_bitwidth", [0, 1])
@pytest.mark.parametrize("dtype", R.FWD_DTYPES)
def test_reference_equals_the_oracle_query_backward(dtype, probe_bitwidth):
    case = R.make_query_case(dtype, probe_bitwidth)
    got = R.reference_query_backward(case)
    want = ohash.hashgrid_query_backward(case["coords"], case["grad_out"].float(), case["res"], case["bitwidth"], case["F"], probe_bitwidth,
                                         half_path=dtype != "f32", acc_dtype=torch.float32)
    assert all(torch.equal(a.double(), b.double()) for a, b in zip(got, want))
    assert all(a.dtype == R.DTYPES[dtype] for a in got)


def test_builder_rejects_inexact_inputs():
    ok = R.make_case("ok", 3, R.R3W, 16, 2, "f32", n=2000, gmax=4)
    R.reference_backward(ok)
    with pytest.raises(AssertionError, match="rounds in fp32"):                     # an offset with too many bits
        R.reference_backward(R.make_case("bits", 3, R.R3W, 16, 2, "f32", n=2000, b=9))
    nudged = dict(ok)
    nudged["coords"] = ok["coords"] + 2.0 ** -20
    with pytest.raises(AssertionError, match="too many bits"):
        R.reference_backward(nudged)
    top = R.max_numerator(R.R3W, 1)
    m = ok["m"].copy()
    m[7, 1] = top + 1                                                               # res 8: x = 7 = res - 1 on that level
    clamped = R.make_case("clamped", 3, R.R3W, 16, 2, "f32", samples=(m, ok["run"]))
    with pytest.raises(AssertionError, match="clamped at res 8 < 258"):
        R.reference_backward(clamped)
    with pytest.raises(AssertionError, match="2\\^24 bound"):
        R.reference_backward(R.make_case("big g", 3, R.R3W, 16, 2, "f32", n=4096, gmax=1 << 14))
    with pytest.raises(AssertionError, match="2\\^17 bound"):
        R.reference_backward(R.make_case("compact", 3, R.R3W, 16, 2, "bf16", n=4096, gmax=2))
    with pytest.raises(AssertionError, match="not a bf16 value"):
        R.make_case("bf16 g", 3, R.R3, 16, 2, "bf16", n=100, gmax=1000)
    with pytest.raises(AssertionError, match="sum \\|g\\|"):
        R.reference_query_backward(R.make_query_case("bf16", 0, n=300, bitwidth=4, gmax=8))


EXPECT = {"direct": {"direct"}, "generic": {"binned", "generic", "merge"}, "compact f": {"binned", "compact", "merge"},
          "compact bf": {"binned", "compact", "merge"}, "compact direct": {"direct", "compact"}, "no merge": {"direct"},
          "merge f32 F8 2d": {"binned", "merge", "generic"}, "no bins": {"direct", "merge", "emit_lds_over"},
          "odd start f32": {"binned", "generic"}, "odd start bf16": {"binned", "compact"}, "dead suffix": {"binned"},
          "spill f32": {"binned", "generic"}, "spill bf16": {"binned", "compact"}, "big bf16": {"binned", "compact"},
          "big f32": {"binned", "generic"}}


@pytest.mark.parametrize("name", R.BWD_NAMES + R.BIG_NAMES)
def test_backward_cases_are_exact_and_reach_what_they_claim(name):
    case = R.bwd_case(name)
    ref = R.reference_backward(case)                  # asserts the 2^24, 2^17 and 2^-38 bounds
    shares = [z for z in ref["zero_share"] if z is not None]
    assert shares and max(shares) <= R.ZERO_CAP, (name, ref["zero_share"])
    got = R.reaches(case)
    assert set(case["claims"]) <= got, (name, sorted(set(case["claims"]) - got))
    keys = [k for k in EXPECT if name.startswith(k)]
    assert len(keys) == 1 and EXPECT[keys[0]] <= got, (name, keys, sorted(got))
    assert ("merge" in got) == (not name.startswith("no merge"))
    print(name, case["n"], case["res"], sorted(got), f"zero share {max(shares):.3f}, 2^{np.log2(ref['max_quanta']):.1f} quanta")
    if name in R.BIG_NAMES:
        R._cases.pop(name)


def test_backward_case_list_covers_every_path():
    """every dispatch decision, emitter, bucket geometry and flush width named in the module is claimed by some case (and the
    claims are verified above)"""
    claimed = set()
    for name in R.BWD_NAMES:
        claimed |= set(dict(R._BWD_SPECS)[name]["claims"])
    assert {"dense", "hashed", "multi_bucket", "sub_bucket", "one_owner", "split", "odd_start", "spill", "dead_levels", "emit_lds_over"} <= claimed
    ns = {dict(R._BWD_SPECS)[n]["n"] for n in R.BWD_NAMES}
    assert {4095, 4096, 4097, 5000, 8193} <= ns
    for form in ("compact", "generic"):
        assert {4096, 4097, 5000, 8193} <= {dict(R._BWD_SPECS)[n]["n"] for n in R.BWD_NAMES if n.startswith(form)}
    assert set(R.ORDER_NAMES) | set(R.LOSS_NAMES) <= set(R.BWD_NAMES)


@pytest.mark.parametrize("name", R.ORDER_NAMES)
def test_orders_are_one_multiset_and_the_deal_does_not_merge(name):
    case = R.bwd_case(name)
    want = R.reference_backward(case)["grad"]
    rows = lambda c: sorted(map(tuple, torch.cat([c["coords"].double(), c["grad_out"]], 1).tolist()))
    for order in ("perm", "alt"):
        other = R.reordered(case, order)
        assert rows(other) == rows(case)
        assert torch.equal(R.reference_backward(other)["grad"], want)
    run = R.reordered(case, "alt")["run"]
    assert int((np.diff(run) == 0).sum()) == 0                      # neighbours always belong to different runs
    assert int((np.diff(case["run"]) == 0).sum()) > case["n"] // 2   # while the run order is made of runs
    lengths = np.bincount(case["run"])
    assert set(R.RUNS) <= set(lengths.tolist())


@pytest.mark.parametrize("name", R.LOSS_NAMES)
def test_loss_scaled_cases_are_exact(name):
    base = R.reference_backward(R.bwd_case(name))["grad"]
    cases = R.loss_scale_cases(name)
    assert [e for _, e in cases] == ([16, 24] if " f16 " in name else [16, 24, -30])
    for case, e in cases:
        ref = R.reference_backward(case)
        assert max(z for z in ref["zero_share"] if z is not None) <= R.ZERO_CAP
        if " f16 " not in name:
            assert torch.equal(ref["grad"], base * 2.0 ** e)


def test_forward_cases_are_exact_and_reach_what_they_claim():
    cases = R.fwd_cases_all()
    seen = set()
    for case in cases:
        R.reference_forward(case)                     # asserts exact weights and 24-bit sums
        got = R.reaches(case)
        assert set(case["claims"]) <= got, (case["name"], sorted(set(case["claims"]) - got))
        seen.add((case["dtype"], case["F"], case["dim"], case["L"] & (case["L"] - 1) == 0))
    assert len({s[:3] for s in seen}) == 24 and len({s for s in seen if s[3]}) == 24 and len({s for s in seen if not s[3]}) >= 24
    # every 2-D / 3-D layout has a dense level below 258
    for dim in (2, 3):
        case = R.fwd_case("f32", 2, dim, 4)
        assert any(g["dense"] and g["res"] < 258 for g in R.bin_geometry(case))
    assert sorted(R.FWD_WIDTHS) == [1, 2, 4, 8, 16]
    for W, (dt, F) in R.FWD_WIDTHS.items():
        assert F * (4 if dt == "f32" else 2) // 4 == W


@pytest.mark.parametrize("dtype", R.FWD_DTYPES)
def test_grad_coords_and_query_cases_are_exact(dtype):
    for F in (2, 4):
        for n in R.GC_N:
            out = R.reference_grad_coords(R.grad_coords_case(dtype, F, n))
            assert out.shape == (n, 3) and (n == 1 or float(out.abs().max()) > 0)
    for p in (0, 1):
        R.reference_query_backward(R.make_query_case(dtype, p))
