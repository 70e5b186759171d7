"""The caller's statement that the hash-grid gradient table is zero on entry of the folded backward (WISP_HG_BWD_GRAD_CLEAN of
include/wisp_hip.h; `grad_clean` of wisp._C.hashgrid_interpolate_backward; csrc/hashgrid.hip), on the GPU, bit for bit: a reduce
workgroup that owns a bucket and saw no overflowed slot of that bucket and no spill in the launch leaves the gradient of its rows alone
- bit 31 of the emitters' count words and largest-magnitude words says which - and every result stays what it is without the
statement.

Cases, case generator and float64 restatement are those of tests/test_gpu_reduce_exact.py (imported): 5000 samples, the smallest
launch that bins with more than one emitting piece, on the smallest table that has single-owner buckets at all - bin_plan gives a level
of up to 32 buckets at least two owners per bucket, so a level needs 33 buckets (more than 2^18 rows) before a flush with the
optimizer in it exists; smaller levels would only ever test the split path.  Every launch is compared with the restatement and, from
the same starting state, with a launch without the statement (integer views, torch.equal).

That a case is not vacuous is shown per case: slot overflow from the launch's own slot statistics; a spill index from the host's
bin_geometry; and that clean buckets were really skipped - or really read - by launching on a SEEDED table with the statement made
against the contract: skipped rows must then come out as if their seeds were zero, with the seeds still in place, and rows that
were read must have applied and zeroed them."""
import contextlib
import os

import numpy as np
import pytest
import torch

import hashgrid_exact_ref as H
import optim_exact_ref as O
import test_gpu_reduce_exact as R
from oracle import hashgrid as ohash
from gpu_helpers import DEV, _C, cuda, make_rays

pytestmark = pytest.mark.gpu

F, GS, GUARD = R.F, R.GS, R.GUARD
_spill_cache = {}
_library_switch = [None]                    # WISP_HG_GRAD_CLEAN for the launches of _launch


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


FORMS = {"plain": dict(clean=False), "clean": dict(clean=True)}


def _launch(case, dev, W, step, form, grad_out=None):
    rows = case["rows"]
    view = lambda t: R._in(t).view(rows, F)
    f = FORMS[form]
    with _env(WISP_HG_GRAD_CLEAN=_library_switch[0]):
        _, covered = _C().hashgrid_interpolate_backward(
            dev["coords"], dev["grad_out"] if grad_out is None else grad_out, (rows, F), dev["first_idx"], case["res"], case["bitwidth"],
            case["zero_from_col"], out=view(W["g"]),
            adamw=dict(param=view(W["p"]), exp_avg=view(W["m"]), exp_avg_sq=view(W["v"]), shadow=None if W["s"] is None else view(W["s"]),
                       step=step, grad_scale=GS, grad_clean=f["clean"], **O.FOLDED_HYPER))
    torch.cuda.synchronize()
    return covered


def _owned_slices(case, covered):
    """flat [begin, end) of the rows bucket owners flush: the covered part of the LIVE levels (dead levels are the tail workgroups')"""
    first = case["first_idx"]
    return [(l, int(first[l]) * F, (int(first[l]) + c) * F) for l, c in enumerate(covered) if c > 0 and l * F < case["zero_from_col"]]


def _checked(trio, W, step, form, what, seeds=None, skipped_seeds=False, grad64=None, grad_out=None, loose=None, plain=True):
    """one launch in `form` from the state in W against the restatement fed the exact gradient (+ seeds, float64 [rows, F], put into
    the gradient table first); skipped_seeds: the bucket owners must have IGNORED the seeds of their rows and left them in place.
    plain: the plain form from the same state must give the same bits.  -> covered"""
    case, g64, dev = trio
    if grad64 is None:
        grad64 = g64
    if seeds is None:
        seeds = torch.zeros_like(grad64)
    g_seed = seeds.float().reshape(-1)
    R._in(W["g"]).copy_(g_seed)
    W2 = {k: (None if t is None else t.clone()) for k, t in W.items()} if plain else None
    before = {k: W[k].detach().cpu().clone() for k in "pmvgs" if W[k] is not None}
    g_in = (grad64 + seeds).float().reshape(-1)
    covered = _launch(case, dev, W, step, form, grad_out)
    paths, host_covered = O.folded_paths(case)
    assert covered == host_covered, f"{what}: the launch covers {covered}, folded_paths says {host_covered}"
    groups = O.folded_groups(case, covered)
    hy = O.FOLDED_HYPER
    host = {k: before[k][GUARD:-GUARD].numpy() for k in "pmv"}
    with np.errstate(all="ignore"):
        ref = O.adamw_groups(host["p"], host["m"], host["v"], g_in.numpy(), groups, hy["beta1"], hy["beta2"], hy["eps"], step, GS, zero_grad=True)
        if skipped_seeds:
            ref0 = O.adamw_groups(host["p"], host["m"], host["v"], grad64.float().reshape(-1).numpy(), groups, hy["beta1"], hy["beta2"],
                                  hy["eps"], step, GS, zero_grad=True)
            owned = _owned_slices(case, covered)
            assert owned, "no bucket owner in this case"
            group_of = {b: i for i, (b, *_rest) in enumerate(groups)}
            for l, lo, hi in owned:
                assert float(g_seed[lo:hi].abs().max()) > 0
                for k in "pmv":
                    ref[k][lo:hi] = ref0[k][lo:hi]
                ref["g"][lo:hi] = g_seed[lo:hi].numpy()
                ref["shadows"][group_of[lo]] = ref0["shadows"][group_of[lo]]
    skip = None
    if loose is not None:
        skip = torch.zeros(before["p"].numel(), dtype=torch.bool)
        skip[GUARD:-GUARD] = loose
    for k, nm in (("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("g", "gradient left in `out`")):
        want = before[k].clone()
        want[GUARD:-GUARD] = torch.from_numpy(ref[k])
        R._same(W[k], want, f"{what}: {nm}", skip)
    if W["s"] is not None:
        want = before["s"].clone()
        for (b, ln, *_), sh in zip(groups, ref["shadows"]):
            want[GUARD + b:GUARD + b + ln] = sh
        R._same(W["s"], want, f"{what}: bf16 shadow", skip)
    if not skipped_seeds and loose is None:
        # with the statement true (or not made) every flush leaves its rows at zero: what is left is the uncovered rows' gradient
        g_after = R._in(W["g"]).detach().cpu()
        for l, lo, hi in _owned_slices(case, covered):
            assert not bool(g_after[lo:hi].any()), f"{what}: level {l} keeps a gradient behind its flush"
    if plain:
        _launch(case, dev, W2, step, "plain", grad_out)
        for k in "pmvgs":
            if W[k] is None:
                continue
            a, b = W[k].detach().cpu(), W2[k].detach().cpu()
            if skip is not None:
                a, b = a[~skip], b[~skip]
            assert torch.equal(R._bits(a), R._bits(b)), f"{what}: {k} differs from the plain form's"
    return covered


def _stats_of(dtype, res, bw, zfc, dim=3):
    C = _C()
    fits = [f for f in C._slot_fits.values() if tuple(f.key[3]) == tuple(res) and f.key[4] == bw and f.key[5] == zfc
            and f.key[1] == C._DTYPE_CODE[H.DTYPES[dtype]] and f.key[0] == dim]
    assert len(fits) == 1, len(fits)
    return fits[0]


def _fills(fit):
    stats = fit.pending
    assert stats is not None, "the launch was not binned"
    stats["event"].synchronize()
    return fit.host_fill.tolist()[:fit.L], stats["cap"], stats["base"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("form", ["plain", "clean"])
def test_two_steps_with_and_without_the_statement(dtype, form):
    """(b), (e): step 1 on a zero table; step 2 from the kernel's own state - on a zero table again where the statement is
    made (it must be true), on a seeded one where it is not"""
    trio = R._case(dtype)
    case = trio[0]
    assert not any(g["spill"] for g in H.bin_geometry(case)), "this case must have no spill index"
    W = R._buffers(case)
    for step in (1, 2):
        seeded = step == 2 and not FORMS[form]["clean"]
        covered = _checked(trio, W, step, form, f"{dtype}, {form}, step {step}", seeds=case["seeds"] if seeded else None)
    assert len(_owned_slices(case, covered)) == 2                       # the strip-dealt level and the hashed one


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_clean_buckets_are_really_skipped(dtype, form="clean"):
    """the statement made AGAINST the contract, on a seeded table, with slots at their unscaled size (no slot overflows - read from
    the launch's slot statistics - and no sample spills): every bucket owner must ignore the seeds of its rows and leave them in
    place, while the dead levels' workgroups and the caller's rows see them as ever.  Without this the clean cases above could pass
    with every gradient load still in place."""
    trio = R._case(dtype)
    case = trio[0]
    _launch(case, trio[2], R._buffers(case), 1, "plain")                 # (creates the slot fit of this shape)
    fit = _stats_of(dtype, R.RES, R.BW, R.ZERO_FROM_COL)
    old = list(fit.scale)
    try:
        fit.scale = [1.0] * fit.L
        fit.pending, fit.calls = None, 0                                  # (the launch after call 0 takes the slot statistics)
        W = R._buffers(case)
        _checked(trio, W, 1, form, f"{dtype}, {form}, seeded against the contract", seeds=case["seeds"], skipped_seeds=True, plain=False)
        fill, cap, base = _fills(fit)
        print(f"skip case {dtype}: fullest slot per level {fill[:3]}, capacity {cap[:3]}")
        for l in (1, 2):
            assert fill[l] < cap[l], (l, fill, cap)
    finally:
        fit.scale, fit.pending = old, None


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_a_bucket_with_an_overflowed_slot_reads_and_zeroes_its_rows(dtype, form="clean"):
    """(c): record slots of 2 % of their size - most records of the single-owner levels go through the emit kernel's atomics into the
    (zero) gradient table; the statement is true on entry, and the owners of those buckets must still read that residue, apply it and
    zero it: the restatement's bits are only reached when they do.  That slots overflowed is read from the slot statistics."""
    C = _C()
    trio = R._case(dtype)
    case = trio[0]
    _launch(case, trio[2], R._buffers(case), 1, "plain")
    fit = _stats_of(dtype, R.RES, R.BW, R.ZERO_FROM_COL)
    old = list(fit.scale)
    try:
        fit.scale = [C._SlotFit.FLOOR] * fit.L
        fit.pending, fit.calls = None, 0
        W = R._buffers(case)
        _checked(trio, W, 1, form, f"{dtype}, {form}, slots at {C._SlotFit.FLOOR} of their size", plain=False)
        fill, cap, base = _fills(fit)
        print(f"overflow case {dtype}: fullest slot per level {fill[:3]}, capacity {cap[:3]}, unscaled {base[:3]}")
        for l in (1, 2):
            assert cap[l] < base[l] and fill[l] >= cap[l], (l, fill, cap, base)
        fit.pending = None
        # (and the plain form on the same shrunk slots, for the comparison of forms)
        Wa, Wb = R._buffers(case), R._buffers(case)
        _launch(case, trio[2], Wa, 1, form)
        _launch(case, trio[2], Wb, 1, "plain")
        for k in "pmvgs":
            assert torch.equal(R._bits(Wa[k]), R._bits(Wb[k])), f"{dtype}, {form}, overflow: {k} differs from the plain form's"
    finally:
        fit.scale, fit.pending = old, None


def _spill_case(dtype):
    """2-D, res 512 / 1024 / 512 at bitwidth 21 with c = +1 on some samples (hashgrid_exact_ref's spill case): level 0 (32 buckets, two
    owners each) spills into the first rows of level 1 - 2^20 rows, 128 strip-dealt single-owner buckets - and level 1 into level 2"""
    if dtype not in _spill_cache:
        case = H.make_case(f"spill {dtype}", 2, (512, 1024, 512), 21, F, dtype, n=5000, plus_one=7)
        geo = H.bin_geometry(case)
        assert any(g["spill"] for g in geo) and [g["owners"] for g in geo] == [2, 1, 2] and geo[1]["buckets"] == 128
        grad = H.reference_backward(case)["grad"]
        td = H.DTYPES[dtype]
        dev = dict(coords=case["coords"].to(DEV), grad_out=case["grad_out"].float().to(td).to(DEV), first_idx=case["first_idx"].to(DEV))
        _spill_cache[dtype] = (case, grad, dev)
    return _spill_cache[dtype]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _spill_cache.clear()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_a_spill_index_makes_every_bucket_read_its_rows(dtype, form="clean"):
    """(d): samples on c = +1 name the row behind their level's last (weight 0, sent to the atomic path): the statement is true on
    entry and the results are the restatement's - and, made against the contract on a seeded table, NO bucket owner may skip: the
    seeds of every covered row are applied and zeroed, which only a launch that saw the spill bit does."""
    trio = _spill_case(dtype)
    case = trio[0]
    W = R._buffers(case)
    covered = _checked(trio, W, 1, form, f"{dtype}, {form}, spill, zero table")
    assert [l for l, _, _ in _owned_slices(case, covered)] == [1]
    _checked(trio, W, 2, form, f"{dtype}, {form}, spill, seeded against the contract", seeds=case["seeds"], plain=False)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_the_other_inputs_with_the_statement(dtype):
    """the remaining inputs of test_gpu_reduce_exact.py with the statement made: the res-64 level that stays split, tensors 4 bytes
    off an 8-byte boundary (the scalar fall-backs read the gradient as ever), no bf16 shadow, and an infinite gradient (fp32
    accumulators)"""
    form = "clean"
    split = R._case(dtype, R.RES_SPLIT)
    _checked(split, R._buffers(split[0]), 1, form, f"{dtype}, res 64 split level")
    trio = R._case(dtype)
    case, grad64, dev = trio
    W = R._buffers(case, shift=1)
    assert all(R._in(W[k]).data_ptr() % 8 == 4 for k in "pmvg")
    _checked(trio, W, 1, form, f"{dtype}, tensors 4 bytes off an 8-byte boundary")
    _checked(trio, R._buffers(case, shadow=False), 1, form, f"{dtype}, no shadow")
    at, col = 1234, 2 * F
    go = dev["grad_out"].clone()
    go[at, col] = float("inf")
    first = case["first_idx"]
    tile = slice(at // H.TILE * H.TILE, at // H.TILE * H.TILE + H.TILE)
    _, tile_idx = ohash.corner_setup(case["coords"][tile], R.RES[2], 2 ** R.BW)
    loose = torch.zeros(case["rows"], F, dtype=torch.bool)
    loose[int(first[2]) + tile_idx.reshape(-1), 0] = True
    g64 = grad64.clone()
    g64[loose] = float("inf")
    W = R._buffers(case)
    _checked(trio, W, 1, form, f"{dtype}, one inf", grad64=g64, grad_out=go, loose=loose.reshape(-1))
    coeffs, idx = ohash.corner_setup(case["coords"][at:at + 1], R.RES[2], 2 ** R.BW)
    full = int(first[2]) + int(idx.reshape(-1)[int(coeffs.reshape(-1).argmax())])
    assert float(coeffs.max()) == 1.0 and not bool(torch.isfinite(R._in(W["p"]).view(-1, F)[full, 0])), "the inf never reached the table"


def test_the_environment_switch_makes_the_library_ignore_the_statement():
    """WISP_HG_GRAD_CLEAN=0: the statement made against the contract on a seeded table changes nothing - every seed is applied"""
    trio = R._case("bf16")
    case = trio[0]
    W = R._buffers(case)
    _library_switch[0] = "0"
    try:
        _checked(trio, W, 1, "clean", "statement ignored", seeds=case["seeds"], plain=False)
    finally:
        _library_switch[0] = None


# ---------------------------------------------------------------------------------------------------- the native step
def _native_one_step(switch):
    """a fresh trainer, its handle built, the table gradient checked to be zero and the statement made for the FIRST step (a run's
    first step has no native step before it to make it), one native step on the batch of test_gpu_reduce_exact._native_run"""
    import test_gpu_1_selfcheck as S
    from wisp.core import Rays
    C = _C()
    C._slot_fits.clear()
    rng = np.random.default_rng(311)
    o, d = make_rays(3000, 312)
    gts = cuda(rng.uniform(size=(3000, 3)).astype(np.float32))
    tr, _ = S._native_pair()
    nat = tr._native
    assert nat is not None
    torch.manual_seed(77)
    rays = Rays(cuda(o), cuda(d), dist_min=1.0, dist_max=5.0)
    with _env(WISP_STEP_GRAD_CLEAN=switch):
        assert nat.applies(rays, None) and nat._ensure(rays)
        assert not bool(tr.flat.grad.any()), "a fresh trainer's gradient is zero"
        nat.grad_clean = True
        loss, count = tr.step(rays, gts)
        loss = float(loss.clone())
    tr.wait_for_parameters()
    torch.cuda.synchronize()
    assert nat.steps == 1 and nat.fallbacks == 0 and nat.grad_clean is True
    assert nat.clean_steps == (1 if switch == "1" else 0), nat.clean_steps
    f = tr.flat
    dd = tr._direct
    off = next(o_ for p, o_ in f._grid_params if p is dd.table)
    first = [int(v) for v in dd._first_idx_host]
    tab = (off, off + dd.table.numel())
    assert not bool(f.grad[tab[0]:tab[1]].any()), "a native folded step leaves the table gradient at zero"
    state = {k: getattr(f, a).detach().clone() for k, a in (("p", "data"), ("m", "exp_avg"), ("v", "exp_avg_sq"), ("s", "shadow"))}
    covered = list(nat.covered_last)
    owned = [tuple(f.ranges["decoder"])] + [(off + 2 * first[l], off + 2 * (first[l] + c)) for l, c in enumerate(covered) if c > 0]
    return dict(loss=loss, count=count, state=state, owned=owned, covered=covered, grid=tuple(f.ranges["grid"]))


def test_native_step_with_and_without_the_clean_gradient_statement():
    """one native step with WISP_STEP_GRAD_CLEAN=1 (the statement reaches the library: clean_steps) and one with =0, as
    test_native_step_times_four_kernels_with_six_events_and_changes_nothing compares two runs: bit for bit everything no float atomic
    enters - the loss, the sample count, the decoder's parameters and moments, every covered table range with moments and bf16 copy -
    and the rest within that test's bounds (1e-5 of the largest entry for the moments, 2e-5 for the parameters where the gradient is
    clearly non-zero)."""
    a, b = _native_one_step("0"), _native_one_step("1")
    assert a["count"] == b["count"] and a["loss"] == b["loss"], (a["loss"], b["loss"], a["count"], b["count"])
    assert a["covered"] == b["covered"] and a["owned"] == b["owned"] and len(a["owned"]) >= 2, (a["covered"], b["covered"])
    print("covered rows per level:", a["covered"], "ranges compared bit for bit:", a["owned"])
    ga, gb = a["grid"]
    for k in "pmvs":
        x, y = a["state"][k], b["state"][k]
        for lo, hi in a["owned"]:
            if k == "s":
                if lo < ga:
                    continue
                lo, hi = lo - ga, hi - ga
            assert torch.equal(R._bits(x[lo:hi]), R._bits(y[lo:hi])), f"{k}[{lo}:{hi}] differs with the statement made"
        if k in "mv":
            R._within(x, y, f"one step, {k}")
    m, pa, pb = a["state"]["m"], a["state"]["p"], b["state"]["p"]
    sure = m.abs() > 1e-4 * float(m.abs().max())
    worst = float((pa - pb)[sure].abs().max())
    print(f"one step, p where the gradient is clearly non-zero ({int(sure.sum())} of {sure.numel()}): largest difference {worst:.3e}")
    assert int(sure.sum()) > 1000 and worst <= 2e-5


def test_native_step_forgets_the_statement_after_a_fall_back(monkeypatch):
    """batches of 700 rays fit the (patched) capacity, the 3000-ray batch does not: native, fall-back (the Python-issued step writes
    the gradient: the statement must be gone), native without the statement, native with it"""
    import test_gpu_1_selfcheck as S
    from wisp.trainers._native_step import NativeHashStep
    rng = np.random.default_rng(321)
    batches = [make_rays(700, 323), make_rays(3000, 322), make_rays(700, 324), make_rays(700, 325)]
    gts = [cuda(rng.uniform(size=(len(o), 3)).astype(np.float32)) for o, _ in batches]
    tr, probe = S._native_pair()
    probe._native = None
    _, counts = S._run_steps(probe, batches[:2], gts[:2], 2, seed=78)
    cap = (min(counts) + max(counts)) // 2
    assert counts[0] < cap < counts[1]
    monkeypatch.setattr(NativeHashStep, "_capacity", lambda self: (int(self.t.max_rays), int(cap)))
    from wisp.core import Rays
    torch.manual_seed(78)
    rays = [Rays(cuda(o), cuda(d), dist_min=1.0, dist_max=5.0) for o, d in batches]
    nat = tr._native
    seen = []
    with _env(WISP_STEP_GRAD_CLEAN="1"):
        for r, g in zip(rays, gts):
            tr.step(r, g)
            seen.append((nat.steps, nat.fallbacks, nat.clean_steps, nat.grad_clean))
    tr.wait_for_parameters()
    torch.cuda.synchronize()
    # (clean_steps counts the statements made: the batch that fell back was handed over with one - true then, and used up by it)
    assert seen == [(1, 0, 0, True), (1, 1, 1, False), (2, 1, 1, True), (3, 1, 2, True)], seen
