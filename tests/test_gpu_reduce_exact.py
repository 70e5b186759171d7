"""The fused-optimizer reduce launch of the hash-grid backward (csrc/hashgrid.hip) at the smallest shape that has every kind of
workgroup the 2^18-sample step has - split coarse buckets (their number follows the launch size, coarse_level_wgs), single-owner
strip-dealt and consecutive buckets with their AdamW flush, tail workgroups on dead levels - and the native step's shared timing
events (csrc/train_step.hip), on the GPU.  The cases are the ones a change to a workgroup's order of loads, to the flush or to the
dead levels' loop can break: odd starts, ragged strips and ranges, tensors off an 8-byte boundary, residue left by overflowing
slots, the fp32 accumulators.

Bit for bit, no tolerance: the gradients are exact by construction (tests/hashgrid_exact_ref.py) and the reference of the update is
the fp32 restatement of tests/optim_exact_ref.py fed that gradient - not a second route through the library.

One table, 3-D, F = 2, bitwidth 19, bf16 (compact records) and f32 gradients, n = 5000 samples (5 emitting pieces):
  level 0  res 16   dense, 4096 rows, one bucket split over 5 workgroups: rows that stay the caller's (uncovered);
  level 1  res 65   dense, 274 625 rows = 34 strip-dealt buckets with ragged last strips, one owner each; one unused row in front of
                    it, so it starts on an odd row;
  level 2  res 128  hashed, 2^19 rows = 64 full buckets of 8192 pairs, one owner each: both round trips of a flush;
  levels 3, 4 res 128 behind zero_from_col with one unused row between them: the tail workgroups step 2^20 + 1 rows, a float count
                    that is no multiple of 4, and with the tensors shifted by one float the range starts on an odd float.
Res 65 is no power of two, which hashgrid_exact_ref.reference_backward asks for; the samples here lie on multiples of 1/16 of the
unit cube's 256 steps, where 65 x is a multiple of 1/16 as well: every weight is a multiple of 2^-12, every product and sum exact
(asserted below like level_weights asserts it), and the reference is the same float64 scatter-add of the oracle's weights.

The non-finite case: the launch-wide maximum is not finite, so every workgroup accumulates in fp32.  The run merge of the emit
kernel scans a wave's 64 samples with v += shifted(v) * take, and 0 * inf leaks a NaN into the other runs of that wave on that level
and feature (tail_compute says so).  So feature 0 of the rows that the 64 samples of the inf's tile touch on its level is left out of the
comparison - NaN payloads, and how far the leak goes, are not specified - the element under the inf's corner of weight 1 must be
non-finite, and every other element of the table equals the restatement bit for bit."""
import numpy as np
import pytest
import torch

import hashgrid_exact_ref as H
import optim_exact_ref as O
from oracle import hashgrid as ohash
from gpu_helpers import DEV, _C, cuda, make_rays

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 7.0
RES, BW, F, N = (16, 65, 128, 128, 128), 19, 2, 5000
# the same table with a res-64 level in the place of the res-65 one: 32 buckets, the most a level that is SPLIT over workgroups can
# have - two owners per bucket at any launch size, so it stays the caller's (bin_plan keeps a level that 64 workgroups would split
# at no fewer than two owners)
RES_SPLIT = (16, 64, 128, 128, 128)
GEOMETRY = {RES: dict(owners=[5, 1, 1], buckets=[1, 34, 64], paths={"dense_one_owner", "hashed_one_owner", "tail", "odd_start", "uncovered"}),
            RES_SPLIT: dict(owners=[5, 2, 1], buckets=[1, 32, 64], paths={"hashed_one_owner", "tail", "odd_start", "uncovered"})}
PAD = (0, 1, 0, 0, 1)
ZERO_FROM_COL = 3 * F
GS = 2.0 ** -7
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    _C()._slot_fits.clear()


def _samples():
    """numerators m = 16 j (j in 0 .. 14) of c = m / 256 * 2 - 1 per axis, in runs of 1, 2, 3 equal samples"""
    rng = np.random.default_rng(65)
    run = H._lay_runs(N, (1, 2, 3))
    cells = rng.integers(0, 15, size=(int(run[-1]) + 1, 3))
    return (cells[run] * 16).astype(np.int64), run


def _case(dtype, res=RES):
    if (dtype, res) not in _cache:
        case = H.make_case(f"reduce {dtype} res {res[1]}", 3, res, BW, F, dtype, b=1, seed=7, gmax=2, pad=PAD, zero_from_col=ZERO_FROM_COL,
                           samples=_samples())
        first, rows = case["first_idx"], case["rows"]
        assert int(first[1]) & 1 == 1 and int(first[5] - first[3]) * F % 4 != 0
        grad = torch.zeros(rows, F, dtype=torch.float64)
        c = case["coords"]
        for l in range(ZERO_FROM_COL // F):
            r = res[l]
            coeffs, idx = ohash.corner_setup(c, r, 2 ** BW)
            x = (c.double() * 0.5 + 0.5) * float(r)
            assert torch.equal(x.float().double(), x) and float(x.max()) < r - 1 and float(x.min()) >= 0.0
            pos = torch.floor(x)
            f = x - pos
            w = torch.ones(N, 8, dtype=torch.float64)
            for j in range(8):
                for a in range(3):
                    w[:, j] *= f[:, a] if (j >> (2 - a)) & 1 else 1.0 - f[:, a]
            assert torch.equal(coeffs.double(), w), f"a weight of res {r} rounds in fp32"
            u = 2.0 ** -12
            assert torch.equal(torch.round(w / u) * u, w)
            g = case["grad_out"][:, l * F:(l + 1) * F]
            rr = (int(first[l]) + idx).reshape(-1)
            assert int(rr.max()) < int(first[l + 1])
            contrib = (w[:, :, None] * g[:, None, :]).reshape(-1, F)
            grad.index_add_(0, rr, contrib)
            asum = torch.zeros(rows, F, dtype=torch.float64).index_add_(0, rr, contrib.abs())
            assert float(asum.max()) / u < 2.0 ** 17, "a sum (or a compact record) leaves its exact range"
        assert torch.equal(grad.float().double(), grad) and torch.equal((grad + case["seeds"]).float().double(), grad + case["seeds"])
        geo = H.bin_geometry(case)
        assert [g["owners"] for g in geo[:3]] == GEOMETRY[res]["owners"] and [g["buckets"] for g in geo[:3]] == GEOMETRY[res]["buckets"]
        td = H.DTYPES[dtype]
        dev = dict(coords=c.to(DEV), grad_out=case["grad_out"].float().to(td).to(DEV), first_idx=first.to(DEV))
        _cache[dtype, res] = (case, grad, dev)
    return _cache[dtype, res]


def _guarded(x, dtype=torch.float32, shift=0):
    n = x if isinstance(x, int) else x.shape[0]
    whole = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=dtype, device=DEV)[shift:]
    if not isinstance(x, int):
        whole[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return whole


def _in(whole):
    return whole[GUARD:whole.numel() - GUARD]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same(got, want, what, skip=None):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = (got != want) | (_bits(got.abs()) != _bits(want.abs()))
    if skip is not None:
        bad &= ~skip
    if bool(bad.any()):
        at = torch.nonzero(bad).flatten()
        lines = [f"element {i - GUARD}: got {float(got[i])!r}, want {float(want[i])!r}" for i in at[:6].tolist()]
        raise AssertionError(f"{what}: {at.numel()} elements differ\n  " + "\n  ".join(lines))


def _buffers(case, shift=0, shadow=True):
    n = case["rows"] * F
    x = O.inputs(n, 77, "fresh")
    W = {k: _guarded(x[k], shift=shift) for k in "pmv"}
    W["g"] = _guarded(np.zeros(n, np.float32), shift=shift)
    W["s"] = _guarded(n, torch.bfloat16, shift=shift) if shadow else None
    return W


def _launch(case, dev, W, step, grad_out=None):
    rows = case["rows"]
    view = lambda t: _in(t).view(rows, F)
    _, covered = _C().hashgrid_interpolate_backward(
        dev["coords"], dev["grad_out"] if grad_out is None else grad_out, (rows, F), dev["first_idx"], case["res"], case["bitwidth"],
        case["zero_from_col"], out=view(W["g"]),
        adamw=dict(param=view(W["p"]), exp_avg=view(W["m"]), exp_avg_sq=view(W["v"]), shadow=None if W["s"] is None else view(W["s"]),
                   step=step, grad_scale=GS, **O.FOLDED_HYPER))
    torch.cuda.synchronize()
    return covered


def _step_checked(dtype, W, step, seeded, what, grad64=None, grad_out=None, loose=None, res=RES):
    """one folded launch from the state in W against the restatement fed the exact gradient; loose: table elements (bool [rows * F])
    whose gradient is not finite (or NaN in the kernel and finite here, where a zero weight meets the inf): not compared"""
    case, g64, dev = _case(dtype, res)
    if grad64 is None:
        grad64 = g64
    seeds = case["seeds"] if seeded else torch.zeros_like(grad64)
    g_in = (grad64 + seeds).float().reshape(-1)
    _in(W["g"]).copy_(seeds.float().reshape(-1))
    before = {k: W[k].detach().cpu().clone() for k in "pmvgs" if W[k] is not None}
    before["g"][GUARD:-GUARD] = g_in
    covered = _launch(case, dev, W, step, grad_out)
    paths, host_covered = O.folded_paths(case)
    assert covered == host_covered, f"{what}: the launch covers {covered}, folded_paths says {host_covered}"
    assert GEOMETRY[res]["paths"] <= paths
    groups = O.folded_groups(case, covered)
    hy = O.FOLDED_HYPER
    host = {k: before[k][GUARD:-GUARD].numpy() for k in "pmv"}
    with np.errstate(all="ignore"):
        ref = O.adamw_groups(host["p"], host["m"], host["v"], g_in.numpy(), groups, hy["beta1"], hy["beta2"], hy["eps"], step, GS, zero_grad=True)
    skip = None
    if loose is not None:
        skip = torch.zeros(before["p"].numel(), dtype=torch.bool)
        skip[GUARD:-GUARD] = loose
    for k, nm in (("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("g", "gradient left in `out`")):
        want = before[k].clone()
        want[GUARD:-GUARD] = torch.from_numpy(ref[k])                  # (uncovered rows: state kept, the exact gradient in `out`)
        _same(W[k], want, f"{what}: {nm}", skip)
    if W["s"] is not None:
        want = before["s"].clone()
        for (b, ln, *_), sh in zip(groups, ref["shadows"]):
            want[GUARD + b:GUARD + b + ln] = sh
        _same(W["s"], want, f"{what}: bf16 shadow", skip)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_two_steps_on_aligned_buffers(dtype):
    """step 1 into a zero `out`, step 2 from the kernel's own state onto a non-zero gradient table"""
    W = _buffers(_case(dtype)[0])
    assert all(_in(W[k]).data_ptr() % 8 == 0 for k in "pmvg")
    for step, seeded in ((1, False), (2, True)):
        _step_checked(dtype, W, step, seeded, f"{dtype}, step {step}")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_a_dense_level_of_32_buckets_keeps_two_owners_and_stays_the_callers(dtype):
    """64^3 rows = 32 buckets: 64 workgroups per coarse level gave it 2 owners per bucket, and so must 16 (16 / 32 rounds to 0):
    covered_rows reports 0 for it (asserted against folded_paths in _step_checked), its rows keep p, m, v and hold the exact
    gradient - were it given one owner, the launch would step it and report its rows"""
    W = _buffers(_case(dtype, RES_SPLIT)[0])
    for step, seeded in ((1, False), (2, True)):
        _step_checked(dtype, W, step, seeded, f"{dtype}, res 64 split level, step {step}", res=RES_SPLIT)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_tensors_shifted_by_one_float_take_the_fallbacks(dtype):
    W = _buffers(_case(dtype)[0], shift=1)
    assert all(_in(W[k]).data_ptr() % 8 == 4 for k in "pmvg")
    _step_checked(dtype, W, 1, True, f"{dtype}, tensors 4 bytes off an 8-byte boundary")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_without_the_bf16_shadow(dtype):
    W = _buffers(_case(dtype)[0], shadow=False)
    _step_checked(dtype, W, 1, True, f"{dtype}, no shadow")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_overflowing_slots_leave_a_residue_that_the_flush_applies_and_zeroes(dtype):
    """record slots of 2 % of their size: most records of the single-owner levels overflow into the emit kernel's atomics, which
    write the gradient table in front of the reduce launch - the flush must see that residue, apply it and zero it.  That slots
    really overflowed is read from the launch's own slot statistics (wisp_hashgrid_bwd_slot_stats through _SlotFit: the fullest
    slot of a level against its capacity) - without that the case would pass as a copy of the aligned one."""
    C = _C()
    case, _, dev = _case(dtype)
    W = _buffers(case)
    _launch(case, dev, W, 1)                                              # (creates the slot fit of this shape)
    fits = [f for f in C._slot_fits.values() if tuple(f.key[3]) == RES and f.key[4] == BW and f.key[5] == ZERO_FROM_COL
            and f.key[1] == C._DTYPE_CODE[H.DTYPES[dtype]]]
    assert len(fits) == 1
    fit, W = fits[0], _buffers(case)
    old = list(fit.scale)
    try:
        fit.scale = [C._SlotFit.FLOOR] * fit.L
        fit.pending, fit.calls = None, 0                                  # (the launch after call 0 takes the slot statistics)
        _step_checked(dtype, W, 1, False, f"{dtype}, slots at {C._SlotFit.FLOOR} of their size")
        stats = fit.pending
        assert stats is not None, "the launch was not binned"
        stats["event"].synchronize()
        fill = fit.host_fill.tolist()[:fit.L]
        print(f"overflow case {dtype}: fullest slot per level {fill[:3]}, capacity {stats['cap'][:3]}, unscaled {stats['base'][:3]}")
        for l in (1, 2):                                                  # both single-owner levels: the flush has residue to apply
            assert stats["cap"][l] < stats["base"][l] and fill[l] >= stats["cap"][l], (l, fill, stats["cap"], stats["base"])
    finally:
        fit.scale, fit.pending = old, None                                # (the statistics of the shrunk slots are not adopted)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_one_infinite_gradient_takes_the_fp32_accumulators(dtype):
    case, grad64, dev = _case(dtype)
    at, col = 1234, 2 * F                                                 # a sample's first column of the hashed level
    go = dev["grad_out"].clone()
    go[at, col] = float("inf")
    first = case["first_idx"]
    _, idx = ohash.corner_setup(case["coords"][at:at + 1], RES[2], 2 ** BW)
    tile = slice(at // H.TILE * H.TILE, at // H.TILE * H.TILE + H.TILE)   # the samples one wave of the emit kernel merges over
    _, tile_idx = ohash.corner_setup(case["coords"][tile], RES[2], 2 ** BW)
    loose = torch.zeros(case["rows"], F, dtype=torch.bool)
    loose[int(first[2]) + tile_idx.reshape(-1), 0] = True                 # (w * inf: inf, NaN where w == 0, NaN leaked by the run merge)
    W = _buffers(case)
    g64 = grad64.clone()
    g64[loose] = float("inf")
    _step_checked(dtype, W, 1, False, f"{dtype}, one inf", grad64=g64, grad_out=go, loose=loose.reshape(-1))
    coeffs, _ = ohash.corner_setup(case["coords"][at:at + 1], RES[2], 2 ** BW)
    full = int(first[2]) + int(idx.reshape(-1)[int(coeffs.reshape(-1).argmax())])
    assert float(coeffs.max()) == 1.0 and not bool(torch.isfinite(_in(W["p"]).view(-1, F)[full, 0])), "the inf never reached the table"


def _native_run(record, steps):
    """a fresh trainer and fresh slot fits (every level's slots at their unscaled size: nothing overflows into the atomic path),
    `steps` native steps on the batches of test_native_step_equals_the_python_issued_step"""
    import test_gpu_1_selfcheck as S
    C = _C()
    C._slot_fits.clear()
    rng = np.random.default_rng(311)
    batches = [make_rays(3000, 312 + k) for k in range(3)]
    gts = [cuda(rng.uniform(size=(3000, 3)).astype(np.float32)) for _ in range(3)]
    tr, _ = S._native_pair()
    assert tr._native is not None
    C.TIMING = {} if record else None
    sink = {}
    try:
        losses, counts = S._run_steps(tr, batches, gts, steps, seed=77)
        if record:
            tr._native.drain_timing(sink)
    finally:
        C.TIMING = None
    assert tr._native.steps == steps and tr._native.fallbacks == 0
    f = tr.flat
    state = {k: getattr(f, a).detach().clone() for k, a in (("p", "data"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("s", "shadow"))}
    d = tr._direct
    off = next(o for p, o in f._grid_params if p is d.table)
    first = [int(v) for v in d._first_idx_host]
    covered = list(getattr(tr._native, "covered_last", []))               # (set when the table's AdamW is folded into the backward)
    # flat ranges that no float atomic enters: the decoder, and the table levels the reduce launch covers (one owner per bucket,
    # fixed-point sums; or stepped by the tail workgroups)
    owned = [tuple(f.ranges["decoder"])] + [(off + 2 * first[l], off + 2 * (first[l] + c)) for l, c in enumerate(covered) if c > 0]
    return dict(losses=losses, counts=counts, sink=sink, state=state, owned=owned, covered=covered,
                grid=tuple(f.ranges["grid"]), timed=tr._native.TIMED)


def _within(a, b, what, rel=1e-5):
    """the bound of test_native_step_equals_the_python_issued_step: 1e-5 of the largest entry"""
    top, diff = float(b.abs().max()), float((a - b).abs().max())
    print(f"{what}: largest difference {diff:.3e}, largest entry {top:.3e}, ratio {diff / top:.3e}")
    assert top > 0 and diff <= rel * top, (what, diff, top)


def test_native_step_times_four_kernels_with_six_events_and_changes_nothing():
    """record_timing = 1: four finite positive durations per step and the sample count as units (one event ends the lookup's interval
    and starts the decoder forward's, one ends the decoder backward's and starts the hash-grid backward's), and the step's outputs
    are those of record_timing = 0.
    Two runs of ONE build at this shape are not bit-identical as a whole: the table's coarse levels are summed with float atomics
    by several workgroups (test_native_step_equals_the_python_issued_step says the same of two Python-issued runs), and from the
    second step on every value depends on those levels through the lookup.  So, after ONE step, bit for bit everything that no
    atomic sum enters - the loss, the sample count, the decoder's parameters and moments (its kernels and the closing sums use no
    atomics), every table level the reduce launch reports as covered (one owner per bucket, fixed-point sums; slots at their
    unscaled size, so nothing overflows) with its moments and bf16 copy - and the rest of the table to the existing bound, 1e-5 of
    the largest entry for the moments, and for the parameters 2e-5 where the gradient is clearly non-zero (below).  (At this
    shape, 2^12 rows per level, every live level is one bucket shared by several workgroups: the launch covers the dead level
    alone, and the live table falls under the bounds.)  After THREE steps: the sample counts, the first loss bit for bit, the later losses to 1e-5 (_close of the selfcheck),
    both moments to 1e-5 of their largest entry."""
    import test_gpu_1_selfcheck as S
    a, b = _native_run(0, 1), _native_run(1, 1)
    assert a["counts"] == b["counts"] and a["losses"] == b["losses"], (a["losses"], b["losses"], a["counts"], b["counts"])
    assert a["covered"] == b["covered"] and a["owned"] == b["owned"], (a["covered"], b["covered"])
    print("covered rows per level:", a["covered"], "ranges compared bit for bit:", a["owned"])
    ga, gb = a["grid"]
    for k in "pmvs":
        x, y = a["state"][k], b["state"][k]
        for lo, hi in a["owned"]:
            if k == "s":                                                   # (the bf16 copy holds the grid range alone)
                if lo < ga:
                    continue
                lo, hi = lo - ga, hi - ga
            assert torch.equal(_bits(x[lo:hi]), _bits(y[lo:hi])), f"{k}[{lo}:{hi}] differs with record_timing = 1"
        if k in "mv":
            _within(x, y, f"one step, {k}")
    # (parameters: Adam's first step moves every parameter with a non-zero gradient by ~lr whatever its size, so add-order noise
    #  on a gradient next to zero moves it by up to 2 lr - compared as test_gradient_accumulation_equals_one_step_over_the_union_
    #  of_the_micro_batches compares them: where the gradient, 10 x the first moment, is clearly non-zero, to 2e-5)
    m, pa, pb = a["state"]["m"], a["state"]["p"], b["state"]["p"]
    sure = m.abs() > 1e-4 * float(m.abs().max())
    worst = float((pa - pb)[sure].abs().max())
    print(f"one step, p where the gradient is clearly non-zero ({int(sure.sum())} of {sure.numel()}): largest difference {worst:.3e}")
    assert int(sure.sum()) > 1000 and worst <= 2e-5
    assert float(b["state"]["m"][ga:gb].abs().max()) > 0
    a, b = _native_run(0, 3), _native_run(1, 3)
    print("three steps, losses:", a["losses"], b["losses"])
    assert a["counts"] == b["counts"] and a["losses"][0] == b["losses"][0] and S._close(b["losses"], a["losses"]), (a["losses"], b["losses"])
    for k in "mv":
        _within(b["state"][k], a["state"][k], f"three steps, {k}")
    sink, counts = b["sink"], b["counts"]
    assert sorted(sink) == sorted(b["timed"]) and len(b["timed"]) == 4
    for name, rows in sink.items():
        assert len(rows) == 3, (name, len(rows))
        for (start, end, units), S_k in zip(rows, counts):
            ms = start.elapsed_time(end)
            assert np.isfinite(ms) and ms > 0.0 and units == S_k, (name, ms, units, S_k)
